// k_duplex.hip — the simplex-to-duplex alignment of `infer duplex_from_pod5_and_bam` (rmr_duplex_align, include/remora_hip.h):
// an exact, unbanded Gotoh DP (three states) with a stored 4-bit trace, and the traceback.  DESIGN.md section "Duplex".
//
// The DP kernel: one wave per alignment.  The simplex (query) rows are cut into strips of RMR_DUPLEX_STRIP_ROWS = 64 * R rows;
// lane l owns the R consecutive rows strip * 64R + l * R .. + R - 1 in registers (H and the deletion state of the column to
// its left) and the strip sweeps the duplex (ref) columns skewed by lane: at step t lane l is at column t - l.  What a lane
// needs from the row above its first one (H, the insertion state, and the duplex base of the column) is what lane l - 1 had at
// step t - 1: three __shfl_up per step.  Lane 0 takes them from the line buffer, the last row of the previous strip (row 0 of
// the matrix for the first one), which lane 63 rewrites in place 63 columns behind; the wave loads it 64 columns at a time,
// one chunk ahead, and lane 0 picks its column with a broadcast.  Every step a lane packs the 4 trace bits of its R = 8 cells
// into one dword: one coalesced 256-byte store per wave and step.
//
// The traceback kernel: one thread per alignment walks the trace from the end cell (dependent loads: slow per alignment,
// parallel over the alignments of a group), writes the runs back to front, strips the gap runs at both ends and turns the
// rest round in place.
//
// Checkpointed memory (rmr_duplex_align_mode, DUPLEX_LINES then DUPLEX_BACKTRACK): the forward pass is the same sweep without the
// trace stores, and instead of rewriting one line in place it keeps the line above every strip (lines[s], m (H, F) pairs;
// lines[0] is row 0).  The walk back is one wave per alignment: from the strip of the end row down it sweeps strip s again from
// lines[s] - the same code, so the same bits -, only the columns at or left of where the walk stands, into a trace buffer of one
// strip, and lane 0 walks that strip by the traceback kernel's rule.  The three are ONE kernel body in three instantiations: a
// sweep that is a function of its own is optimised apart from its caller and DUPLEX_FULL no longer compiles to the same code.
#include "rmr_internal.h"

using namespace rmr;

namespace {

constexpr int R = RMR_DUPLEX_ROWS_PER_LANE;
constexpr int S = RMR_DUPLEX_STRIP_ROWS;
constexpr int OPEN = RMR_DUPLEX_GAP_OPEN, EXT = RMR_DUPLEX_GAP_EXTEND;
constexpr int NEG = -(1 << 30);  // a state that cannot be entered; never accumulated, only NEG - EXT is ever formed
static_assert(S == 64 * R && R == 8, "a lane's trace bits of one step fill one dword");

// A C G T -> 0..3, N -> 4 (the entry point refuses every other letter before the launch)
__device__ __forceinline__ int base_code(uint8_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }

// NUC.4.4 restricted to A C G T N
__device__ __forceinline__ int subst(int q, int b) {
    const int acgt = q == b ? RMR_DUPLEX_MATCH : RMR_DUPLEX_MISMATCH;
    const int with_n = q == b ? RMR_DUPLEX_N_N : RMR_DUPLEX_N_BASE;
    return ((q | b) & 4) ? with_n : acgt;
}

// runs are BAM CIGAR words (length << 4 | op) with op M = 0, I = 1, D = 2
__device__ __forceinline__ void push_run(uint32_t *runs, int64_t &k, uint32_t op, uint32_t len) {
    if (k > 0 && (runs[k - 1] & 15u) == op) runs[k - 1] += len << 4;
    else runs[k++] = len << 4 | op;
}

// where a walk back stands: at cell (i, j) in `state` (0 H, 1 deletion, 2 insertion), k runs written (back to front)
struct Walk {
    int i, j, state;
    int64_t k;
};

// The walk while it stays below row `row_lo` and right of column 0.  ONE_STRIP: `tr` is the trace of the strip the walk is in (the
// caller stops it at the strip's first row), otherwise the trace of all strips, `steps` = m + 63 steps each.
template <bool ONE_STRIP>
__device__ __forceinline__ Walk walk_path(const uint32_t *tr, size_t steps, int row_lo, uint32_t *runs, Walk w) {
    while (w.j > 0 && w.i > row_lo) {
        const int s = (w.i - 1) / S, l = ((w.i - 1) % S) / R, r = (w.i - 1) % R;
        const size_t t = (ONE_STRIP ? (size_t)0 : (size_t)s * steps) + (size_t)(w.j - 1 + l);
        const uint32_t nib = tr[t * 64 + l] >> (4 * r);
        if (w.state == 0) {
            w.state = nib & 3;
            if (w.state == 0) push_run(runs, w.k, 0, 1), --w.i, --w.j;
        } else if (w.state == 1) {
            push_run(runs, w.k, 2, 1);
            if (!(nib & 4)) w.state = 0;
            --w.j;
        } else {
            push_run(runs, w.k, 1, 1);
            if (!(nib & 8)) w.state = 0;
            --w.i;
        }
    }
    return w;
}

// The end of a walk, at row 0 or column 0: what the path still owes, the trimming, the output fields.
__device__ __forceinline__ void finish_path(const DuplexJob &jb, uint32_t *runs, Walk w, int2 best, int32_t *out) {
    const int m = jb.m;
    int64_t k = w.k;
    if (w.j > 0) push_run(runs, k, 2, (uint32_t)w.j);  // row 0: the duplex bases left are one deletion
    // `runs` holds the path back to front.  Strip the gap runs at both ends (duplex_utils.trim_parasail_alignment)
    int64_t lo = 0, hi = k;  // kept: [lo, hi)
    int query_start = w.i, ref_start = 0, ref_end = m;
    while (lo < hi && (runs[lo] & 15u) != 0) {
        if ((runs[lo] & 15u) == 2) ref_end -= (int)(runs[lo] >> 4);
        ++lo;
    }
    while (hi > lo && (runs[hi - 1] & 15u) != 0) {
        if ((runs[hi - 1] & 15u) == 2) ref_start += (int)(runs[hi - 1] >> 4);
        else query_start += (int)(runs[hi - 1] >> 4);
        --hi;
    }
    const int64_t cnt = hi - lo;
    for (int64_t x = 0; x < cnt / 2; ++x) {
        const uint32_t u = runs[lo + x];
        runs[lo + x] = runs[hi - 1 - x];
        runs[hi - 1 - x] = u;
    }
    if (lo > 0)
        for (int64_t x = 0; x < cnt; ++x) runs[x] = runs[lo + x];
    int32_t *o = out + (size_t)jb.out_idx * RMR_DUPLEX_OUT_FIELDS;
    const bool ok = cnt > 0;  // nothing but the status is reported for a path without a match operation
    o[0] = ok ? RMR_DUPLEX_OK : RMR_DUPLEX_NO_MATCH;
    o[1] = ok ? best.x : 0;
    o[2] = ok ? best.y : 0;
    o[3] = ok ? query_start : 0;
    o[4] = ok ? ref_start : 0;
    o[5] = ok ? ref_end : 0;
    o[6] = (int32_t)cnt;
    o[7] = 0;
}

// DUPLEX_FULL: the forward pass of rmr_duplex_align.  `trace` takes the 4 bits of every cell, `line` is one line of m per job that
//   every strip rewrites in place, `best` receives (score, end row).
// DUPLEX_LINES: the forward pass in checkpointed memory.  Nothing is stored per cell; `line` is one line of m per strip and job
//   (strip s reads lines[s], lane 63 writes lines[s + 1]; none below the last strip).
// DUPLEX_BACKTRACK: the walk back in checkpointed memory from `best` and the lines of DUPLEX_LINES; `trace` is one strip of trace
//   per job, [m + 63][64] dwords.  (i, j) of the walk is the same in every lane between the strips; its state and runs are lane 0's.
enum { DUPLEX_FULL, DUPLEX_LINES, DUPLEX_BACKTRACK };

template <int MODE>
__global__ __launch_bounds__(64) void duplex_dp_kernel(const DuplexJob *jobs, const uint8_t *bases, uint32_t *trace, int2 *line, int2 *best,
                                                       uint32_t *runs_all, int32_t *out) {
    const DuplexJob jb = jobs[blockIdx.x];
    const int lane = threadIdx.x;
    const int n = jb.n, m = jb.m;
    const uint8_t *q = bases + jb.q_off, *rf = bases + jb.r_off;
    int2 *ln = line + jb.line_off;  // [m]: (H, insertion state) of the row above the strip, column j + 1 at index j
    if constexpr (MODE != DUPLEX_BACKTRACK) {
        // row 0: the duplex is global, so its leading bases are a penalised deletion
        for (int j = lane; j < m; j += 64) ln[j] = make_int2(-(OPEN + EXT * j), NEG);
        __threadfence();
    }
    int bs = -(OPEN + EXT * (m - 1)), bi = 0;  // the best end row so far: max H[i][m], the smallest i
    const int steps = m + 63;
    const int n_strips = (n + S - 1) / S;
    Walk w{0, m, 0, 0};
    if constexpr (MODE == DUPLEX_BACKTRACK) w.i = best[blockIdx.x].y;
    // forward: every strip, over all m columns.  Walking back: from the strip of the end row ((i - 1) / S holds row i; the strips
    // above it are never swept again) down, while there is path left, over the w.j columns at or left of the walk (a cell depends
    // on nothing to its right)
    for (int strip = MODE == DUPLEX_BACKTRACK ? (w.i - 1) / S : 0; MODE == DUPLEX_BACKTRACK ? w.i > 0 && w.j > 0 : strip < n_strips;
         strip += MODE == DUPLEX_BACKTRACK ? -1 : 1) {
        const int mc = MODE == DUPLEX_BACKTRACK ? w.j : m;
        const int stc = MODE == DUPLEX_BACKTRACK ? w.j + 63 : steps;
        int2 *above = MODE == DUPLEX_FULL ? ln : ln + (size_t)strip * m;
        const int row0 = strip * S + lane * R;
        int qc[R], hl[R], ed[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            qc[r] = row0 + r < n ? base_code(q[row0 + r]) : 0;
            hl[r] = 0;  // column 0: the simplex prefix is free
            ed[r] = NEG;
        }
        int diag = 0, h_bot = 0, f_bot = NEG, b_bot = 0;
        uint32_t *tr = trace + jb.trace_off + (MODE == DUPLEX_FULL ? (size_t)strip * steps * 64 : (size_t)0);
        int2 nxt = lane < mc ? above[lane] : make_int2(0, NEG);
        int bnxt = lane < mc ? base_code(rf[lane]) : 0;
        for (int t0 = 0; t0 < stc; t0 += 64) {
            const int2 cur = nxt;
            const int bcur = bnxt;
            const int jn = t0 + 64 + lane;
            nxt = jn < mc ? above[jn] : make_int2(0, NEG);
            bnxt = jn < mc ? base_code(rf[jn]) : 0;
            const int tt_end = stc - t0 < 64 ? stc - t0 : 64;
            for (int tt = 0; tt < tt_end; ++tt) {
                const int t = t0 + tt;
                int hu = __shfl_up(h_bot, 1), fu = __shfl_up(f_bot, 1), b = __shfl_up(b_bot, 1);
                const int ch = __shfl(cur.x, tt), cf = __shfl(cur.y, tt), cb = __shfl(bcur, tt);
                if (lane == 0) hu = ch, fu = cf, b = cb;
                const int j0 = t - lane;  // this lane's column, 0-based
                if (j0 >= 0 && j0 < mc) {
                    uint32_t bits = 0;
                    int dg = diag, hup = hu, fup = fu;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int eo = hl[r] - OPEN, ee = ed[r] - EXT;
                        const int en = eo > ee ? eo : ee;
                        const int fo = hup - OPEN, fe = fup - EXT;
                        const int fn = fo > fe ? fo : fe;
                        const int d = dg + subst(qc[r], b);
                        const int g = en > fn ? en : fn;
                        const int h = d > g ? d : g;
                        // H source: the diagonal first, then the deletion state, then the insertion state; a gap state is left for
                        // H as soon as the scores allow (its stay bit is set only where extending is strictly better)
                        const uint32_t src = d >= g ? 0u : (en >= fn ? 1u : 2u);
                        bits |= (src | (ee > eo ? 4u : 0u) | (fe > fo ? 8u : 0u)) << (4 * r);
                        dg = hl[r];
                        hl[r] = h, ed[r] = en;
                        hup = h, fup = fn;
                    }
                    diag = hu;
                    h_bot = hup, f_bot = fup, b_bot = b;
                    if constexpr (MODE != DUPLEX_LINES) tr[(size_t)t * 64 + lane] = bits;
                    if constexpr (MODE == DUPLEX_FULL) {
                        if (lane == 63) ln[j0] = make_int2(hup, fup);
                    } else if constexpr (MODE == DUPLEX_LINES) {
                        if (lane == 63 && strip + 1 < n_strips) above[(size_t)m + j0] = make_int2(hup, fup);
                    }
                    if constexpr (MODE != DUPLEX_BACKTRACK) {
                        if (j0 == m - 1) {
#pragma unroll
                            for (int r = 0; r < R; ++r)
                                if (row0 + r < n && hl[r] > bs) bs = hl[r], bi = row0 + r + 1;
                        }
                    }
                }
            }
        }
        __threadfence();  // the next strip reads the line that lane 63 wrote; lane 0 the trace that every lane wrote
        if constexpr (MODE == DUPLEX_BACKTRACK) {
            if (lane == 0) w = walk_path<true>(tr, 0, strip * S, runs_all + jb.run_off, w);
            w.i = __shfl(w.i, 0), w.j = __shfl(w.j, 0);
        }
    }
    if constexpr (MODE == DUPLEX_BACKTRACK) {
        if (lane == 0) finish_path(jb, runs_all + jb.run_off, w, best[blockIdx.x], out);
    } else {
        for (int off = 32; off > 0; off >>= 1) {
            const int os = __shfl_xor(bs, off), oi = __shfl_xor(bi, off);
            if (os > bs || (os == bs && oi < bi)) bs = os, bi = oi;
        }
        if (lane == 0) best[blockIdx.x] = make_int2(bs, bi);
    }
}

__global__ __launch_bounds__(64) void duplex_trace_kernel(const DuplexJob *jobs, int n_jobs, const uint32_t *trace, const int2 *best,
                                                          uint32_t *runs_all, int32_t *out) {
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= n_jobs) return;
    const DuplexJob jb = jobs[a];
    uint32_t *runs = runs_all + jb.run_off;  // room for 2 m + 2 runs: at most m runs consume the duplex, one I run between and around them
    const Walk w = walk_path<false>(trace + jb.trace_off, (size_t)jb.m + 63, 0, runs, Walk{best[a].y, jb.m, 0, 0});
    finish_path(jb, runs, w, best[a], out);
}

}  // namespace

namespace rmr {

int launch_duplex_group(rmr_engine *e, const DuplexJob *jobs, int n_jobs, const uint8_t *bases, uint32_t *trace, int2 *line, int2 *best,
                        uint32_t *runs, int32_t *out) {
    if (n_jobs <= 0) return 0;
    {
        ProfScope ps(e, K_DUPLEX_DP);
        hipLaunchKernelGGL(duplex_dp_kernel<DUPLEX_FULL>, dim3((unsigned)n_jobs), dim3(64), 0, e->stream, jobs, bases, trace, line, best,
                           (uint32_t *)nullptr, (int32_t *)nullptr);
        RMR_HIP(hipGetLastError());
    }
    ProfScope ps(e, K_DUPLEX_TRACE);
    hipLaunchKernelGGL(duplex_trace_kernel, dim3((unsigned)((n_jobs + 63) / 64)), dim3(64), 0, e->stream, jobs, n_jobs, trace, best, runs, out);
    RMR_HIP(hipGetLastError());
    return 0;
}

int launch_duplex_group_checkpoint(rmr_engine *e, const DuplexJob *jobs, int n_jobs, const uint8_t *bases, uint32_t *trace, int2 *line,
                                   int2 *best, uint32_t *runs, int32_t *out) {
    if (n_jobs <= 0) return 0;
    {
        ProfScope ps(e, K_DUPLEX_LINES);
        hipLaunchKernelGGL(duplex_dp_kernel<DUPLEX_LINES>, dim3((unsigned)n_jobs), dim3(64), 0, e->stream, jobs, bases, (uint32_t *)nullptr, line,
                           best, (uint32_t *)nullptr, (int32_t *)nullptr);
        RMR_HIP(hipGetLastError());
    }
    ProfScope ps(e, K_DUPLEX_BACKTRACK);
    hipLaunchKernelGGL(duplex_dp_kernel<DUPLEX_BACKTRACK>, dim3((unsigned)n_jobs), dim3(64), 0, e->stream, jobs, bases, trace, line, best, runs,
                       out);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
