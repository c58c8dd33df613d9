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

__global__ __launch_bounds__(64) void duplex_dp_kernel(const DuplexJob *jobs, const uint8_t *bases, uint32_t *trace, int2 *line,
                                                       int2 *best) {
    const DuplexJob jb = jobs[blockIdx.x];
    const int lane = threadIdx.x;
    const int n = jb.n, m = jb.m;
    const uint8_t *q = bases + jb.q_off, *rf = bases + jb.r_off;
    int2 *ln = line + jb.line_off;  // [m]: (H, insertion state) of the row above the strip, column j + 1 at index j
    // row 0: the duplex is global, so its leading bases are a penalised deletion
    for (int j = lane; j < m; j += 64) ln[j] = make_int2(-(OPEN + EXT * j), NEG);
    __threadfence();
    int bs = -(OPEN + EXT * (m - 1)), bi = 0;  // the best end row so far: max H[i][m], the smallest i
    const int steps = m + 63;
    const int n_strips = (n + S - 1) / S;
    for (int strip = 0; strip < n_strips; ++strip) {
        const int row0 = strip * S + lane * R;
        int qc[R], hl[R], ed[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            qc[r] = row0 + r < n ? base_code(q[row0 + r]) : 0;
            hl[r] = 0;  // column 0: the simplex prefix is free
            ed[r] = NEG;
        }
        int diag = 0, h_bot = 0, f_bot = NEG, b_bot = 0;
        uint32_t *tr = trace + jb.trace_off + (size_t)strip * steps * 64;
        int2 nxt = lane < m ? ln[lane] : make_int2(0, NEG);
        int bnxt = lane < m ? base_code(rf[lane]) : 0;
        for (int t0 = 0; t0 < steps; t0 += 64) {
            const int2 cur = nxt;
            const int bcur = bnxt;
            const int jn = t0 + 64 + lane;
            nxt = jn < m ? ln[jn] : make_int2(0, NEG);
            bnxt = jn < m ? base_code(rf[jn]) : 0;
            const int tt_end = steps - t0 < 64 ? steps - t0 : 64;
            for (int tt = 0; tt < tt_end; ++tt) {
                const int t = t0 + tt;
                int hu = __shfl_up(h_bot, 1), fu = __shfl_up(f_bot, 1), b = __shfl_up(b_bot, 1);
                const int ch = __shfl(cur.x, tt), cf = __shfl(cur.y, tt), cb = __shfl(bcur, tt);
                if (lane == 0) hu = ch, fu = cf, b = cb;
                const int j0 = t - lane;  // this lane's column, 0-based
                if (j0 >= 0 && j0 < m) {
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
                    tr[(size_t)t * 64 + lane] = bits;
                    if (lane == 63) ln[j0] = make_int2(hup, fup);
                    if (j0 == m - 1) {
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if (row0 + r < n && hl[r] > bs) bs = hl[r], bi = row0 + r + 1;
                    }
                }
            }
        }
        __threadfence();  // the next strip reads the line that lane 63 wrote
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int os = __shfl_xor(bs, off), oi = __shfl_xor(bi, off);
        if (os > bs || (os == bs && oi < bi)) bs = os, bi = oi;
    }
    if (lane == 0) best[blockIdx.x] = make_int2(bs, bi);
}

// runs are BAM CIGAR words (length << 4 | op) with op M = 0, I = 1, D = 2
__device__ __forceinline__ void push_run(uint32_t *runs, int64_t &k, uint32_t op, uint32_t len) {
    if (k > 0 && (runs[k - 1] & 15u) == op) runs[k - 1] += len << 4;
    else runs[k++] = len << 4 | op;
}

__global__ __launch_bounds__(64) void duplex_trace_kernel(const DuplexJob *jobs, int n_jobs, const uint32_t *trace, const int2 *best,
                                                          uint32_t *runs_all, int32_t *out) {
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= n_jobs) return;
    const DuplexJob jb = jobs[a];
    const int m = jb.m;
    const size_t steps = (size_t)m + 63;
    const uint32_t *tr = trace + jb.trace_off;
    uint32_t *runs = runs_all + jb.run_off;  // room for 2 m + 2 runs: at most m runs consume the duplex, one I run between and around them
    int i = best[a].y, j = m, state = 0;
    int64_t k = 0;
    while (j > 0) {
        if (i == 0) {  // row 0: the duplex bases left are one deletion
            push_run(runs, k, 2, (uint32_t)j);
            j = 0;
            break;
        }
        const int s = (i - 1) / S, l = ((i - 1) % S) / R, r = (i - 1) % R;
        const uint32_t nib = tr[((size_t)s * steps + (size_t)(j - 1 + l)) * 64 + l] >> (4 * r);
        if (state == 0) {
            state = nib & 3;
            if (state == 0) push_run(runs, k, 0, 1), --i, --j;
        } else if (state == 1) {
            push_run(runs, k, 2, 1);
            if (!(nib & 4)) state = 0;
            --j;
        } else {
            push_run(runs, k, 1, 1);
            if (!(nib & 8)) state = 0;
            --i;
        }
    }
    // `runs` holds the path back to front.  Strip the gap runs at both ends (duplex_utils.trim_parasail_alignment)
    int64_t lo = 0, hi = k;  // kept: [lo, hi)
    int query_start = i, ref_start = 0, ref_end = m;
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
    o[1] = ok ? best[a].x : 0;
    o[2] = ok ? best[a].y : 0;
    o[3] = ok ? query_start : 0;
    o[4] = ok ? ref_start : 0;
    o[5] = ok ? ref_end : 0;
    o[6] = (int32_t)cnt;
    o[7] = 0;
}

}  // namespace

namespace rmr {

int launch_duplex_group(rmr_engine *e, const DuplexJob *jobs, int n_jobs, const uint8_t *bases, uint32_t *trace, int2 *line, int2 *best,
                        uint32_t *runs, int32_t *out) {
    if (n_jobs <= 0) return 0;
    {
        ProfScope ps(e, K_DUPLEX_DP);
        hipLaunchKernelGGL(duplex_dp_kernel, dim3((unsigned)n_jobs), dim3(64), 0, e->stream, jobs, bases, trace, line, best);
        RMR_HIP(hipGetLastError());
    }
    ProfScope ps(e, K_DUPLEX_TRACE);
    hipLaunchKernelGGL(duplex_trace_kernel, dim3((unsigned)((n_jobs + 63) / 64)), dim3(64), 0, e->stream, jobs, n_jobs, trace, best, runs, out);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
