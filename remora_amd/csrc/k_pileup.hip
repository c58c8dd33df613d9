// k_pileup.hip — `analyze pileup_modbams`: the modified-base calls of BAM records counted per reference site on the device.
// No counterpart in the reference's command line: this is the per-site table (bedMethyl) its users build next, from the
// per-read probabilities of the output BAM, with a CPU pileup over a sorted and indexed file.
//
//   emit    the walk of rmr_modbam_walk.h without the truth lookup: every aligned call (inside the region) is classified in
//           integers - k = 512 p per column, class = argmax with ties to the lower column, kmax = the winner's k - and written
//           as one word   ref_id (24 bits) | pos (31) | strand (1) | code (4),   code = the class, or n_mods + 1 (`fail`) where
//           kmax < k_T.  Count pass, the caller's prefix sum, fill pass; the count pass can add the calls' kmax to a histogram
//           (513 LDS bins per block, one 64-bit integer atomic per non-zero bin and block: sums of integers, any order).
//   flush   the words of the call buffer, when it is full and at the end:
//             radix sort over the used bits (end_bit from the contig count);
//             heads   1 where a word's site differs from its predecessor's; exclusive scan -> the site's row;
//             runs    the thread at the head of a (site, code) run finds the run's end by binary search: end - start is that
//                     column of the site's row.  No atomics;
//           -> unique sites in ascending order, ncol = n_mods + 2 u32 counts each.
//   merge   into the resident table (ascending unique keys): every new row searches the table; a hit is added in place (keys
//           are unique on both sides: no two threads touch one row), the misses are compacted and merged by rank - a row's
//           place is its own index plus its lower bound in the other list - into a table allocated at its new size.
//   cover   after the table is finished (--coverage-columns): every record against the sites of the table inside its reference
//           span - a deletion there, another base than the canonical one, or the canonical base without a call - one block per
//           record, two binary searches in the table's keys, one integer atomic per (record, site) into u32[n_sites][3].
// Device memory: the work block (sized by the capacity of the call buffer) plus 8 + 4 ncol bytes per distinct site, twice
// that while a merge copies the table.  All arithmetic is integer; the table does not depend on how the calls were cut
// into batches or flushes.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "rmr_modbam_walk.h"
#include "rmr_stage.h"

using namespace rmr;

namespace {

template <bool FILL>
__global__ __launch_bounds__(MB_THREADS) void modbam_call_kernel(rmr_modbam_batch b, PileupEmit pe, int32_t *__restrict__ ords,
                                                                  int64_t *__restrict__ cig_q, int64_t *__restrict__ cig_r,
                                                                  int64_t *__restrict__ counts, int32_t *__restrict__ status,
                                                                  const int64_t *__restrict__ out_off) {
    __shared__ unsigned s_hist[FILL ? 1 : PILEUP_BINS];
    modbam_walk<FILL, true>(b, ords, cig_q, cig_r, counts, status, out_off, nullptr, nullptr, nullptr, nullptr, pe, s_hist);
}

constexpr unsigned PU_THREADS = 256;
inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + PU_THREADS - 1) / PU_THREADS)); }

// the first index in [lo, hi) whose key is not below x
__device__ inline int64_t lower_bound_u64(const uint64_t *__restrict__ a, int64_t lo, int64_t hi, uint64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PU_THREADS) void site_heads_kernel(const uint64_t *__restrict__ w, int64_t n, uint32_t *__restrict__ head) {
    const int64_t i = (int64_t)blockIdx.x * PU_THREADS + threadIdx.x;
    if (i < n) head[i] = i == 0 || (w[i] >> 4) != (w[i - 1] >> 4);
}

// w sorted; row = exclusive scan of head; counts zeroed for the n_sites rows
__global__ __launch_bounds__(PU_THREADS) void site_runs_kernel(const uint64_t *__restrict__ w, int64_t n, const uint32_t *__restrict__ head,
                                                                const uint32_t *__restrict__ row, int ncol, int64_t n_sites,
                                                                uint64_t *__restrict__ keys, uint32_t *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * PU_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t x = w[i];
    if (i > 0 && w[i - 1] == x) return;  // not the head of its (site, code) run
    const int64_t end = lower_bound_u64(w, i + 1, n, x + 1);  // (x + 1 does not wrap: a word uses 60 bits)
    const int64_t s = head[i] ? (int64_t)row[i] : (int64_t)row[i] - 1;
    if (s < 0 || s >= n_sites) return;  // (the rows were sized by the same scan: never true)
    const int code = (int)(x & 15u);
    if (code < ncol) counts[s * ncol + code] = (uint32_t)(end - i);
    if (head[i]) keys[s] = x >> 4;
}

// hits are added in place; *overflow = 1 + the largest key whose count would pass 2^32 - 1 (left as it was)
__global__ __launch_bounds__(PU_THREADS) void table_hits_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ counts, int64_t ns,
                                                                 int ncol, const uint64_t *__restrict__ t_keys, uint32_t *__restrict__ t_counts,
                                                                 int64_t nt, uint32_t *__restrict__ miss, unsigned long long *__restrict__ overflow) {
    const int64_t j = (int64_t)blockIdx.x * PU_THREADS + threadIdx.x;
    if (j >= ns) return;
    const uint64_t key = keys[j];
    const int64_t at = lower_bound_u64(t_keys, 0, nt, key);
    const bool hit = at < nt && t_keys[at] == key;
    miss[j] = hit ? 0u : 1u;
    if (!hit) return;
    for (int c = 0; c < ncol; ++c) {
        const uint64_t sum = (uint64_t)t_counts[at * ncol + c] + counts[j * ncol + c];
        if (sum > 0xffffffffull) atomicMax(overflow, (unsigned long long)key + 1ull);
        else t_counts[at * ncol + c] = (uint32_t)sum;
    }
}

__global__ __launch_bounds__(PU_THREADS) void compact_misses_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ miss,
                                                                     const uint32_t *__restrict__ rank, int64_t ns, int64_t m,
                                                                     uint64_t *__restrict__ miss_keys, uint32_t *__restrict__ miss_src) {
    const int64_t j = (int64_t)blockIdx.x * PU_THREADS + threadIdx.x;
    if (j >= ns || !miss[j]) return;
    const int64_t k = rank[j];
    if (k >= m) return;  // (m is the same scan's total: never true)
    miss_keys[k] = keys[j];
    miss_src[k] = (uint32_t)j;
}

// the rows of the old table to their places in the merged one
__global__ __launch_bounds__(PU_THREADS) void merge_old_kernel(const uint64_t *__restrict__ t_keys, const uint32_t *__restrict__ t_counts, int64_t nt,
                                                                const uint64_t *__restrict__ miss_keys, int64_t m, int ncol,
                                                                uint64_t *__restrict__ o_keys, uint32_t *__restrict__ o_counts) {
    const int64_t i = (int64_t)blockIdx.x * PU_THREADS + threadIdx.x;
    if (i >= nt) return;
    const uint64_t key = t_keys[i];
    const int64_t d = i + lower_bound_u64(miss_keys, 0, m, key);
    o_keys[d] = key;
    for (int c = 0; c < ncol; ++c) o_counts[d * ncol + c] = t_counts[i * ncol + c];
}

// the new sites to theirs
__global__ __launch_bounds__(PU_THREADS) void merge_new_kernel(const uint64_t *__restrict__ miss_keys, const uint32_t *__restrict__ miss_src, int64_t m,
                                                                const uint32_t *__restrict__ counts, const uint64_t *__restrict__ t_keys, int64_t nt,
                                                                int ncol, uint64_t *__restrict__ o_keys, uint32_t *__restrict__ o_counts) {
    const int64_t k = (int64_t)blockIdx.x * PU_THREADS + threadIdx.x;
    if (k >= m) return;
    const uint64_t key = miss_keys[k];
    const int64_t d = k + lower_bound_u64(t_keys, 0, nt, key), j = miss_src[k];
    o_keys[d] = key;
    for (int c = 0; c < ncol; ++c) o_counts[d * ncol + c] = counts[j * ncol + c];
}

// One block per record, its threads striding over the record's words like the emit's: the partition id into the bits above
// the contig index.  Records of partition 0 and records without words store nothing; no store at or behind words[n_words].
__global__ __launch_bounds__(PU_THREADS) void stamp_partition_kernel(const int64_t *__restrict__ out_off, const int32_t *__restrict__ part, int shift,
                                                                      uint64_t *__restrict__ words, int64_t n_words) {
    const int64_t r = blockIdx.x;
    const int32_t id = part[r];
    if (id <= 0) return;
    const int64_t lo = out_off[r] > 0 ? out_off[r] : 0, hi = out_off[r + 1] < n_words ? out_off[r + 1] : n_words;
    const uint64_t field = (uint64_t)(uint32_t)id << shift;
    for (int64_t i = lo + threadIdx.x; i < hi; i += PU_THREADS) words[i] |= field;
}

// ---- the coverage join ----
// what the join needs beside the batch and the reference part
struct CoverArgs {
    const int32_t *status;          // the emit's, per record
    const int64_t *cig_q, *cig_r;   // the count pass's prefix sums, indexed like b.cigar
    const int64_t *out_off;         // the record's slice of `words`
    const uint64_t *words;
    int64_t n_words;
    const int32_t *part;            // nullable
    int shift;                      // the partition field's first bit in a word
    int canonical;                  // 'A' 'C' 'G' 'T'
    int fold_window;
    const uint64_t *t_keys;
    int64_t nt;
    uint32_t *cover;                // u32[nt][3]: delete, diff, nocall
};

// does one of words[lo, hi) have the site key `key`?  The slice is monotone in its keys - ascending when !desc - up to `window`
// places (the folded '-' words of several motifs): a binary search for the place where the keys pass `key`, then the words
// within `window` of it.
__device__ inline bool slice_has_key(const uint64_t *__restrict__ words, int64_t lo, int64_t hi, uint64_t key, bool desc, int window) {
    int64_t a = lo, z = hi;
    while (a < z) {
        const int64_t mid = a + ((z - a) >> 1);
        const uint64_t k = words[mid] >> 4;
        if (desc ? k > key : k < key) a = mid + 1;
        else z = mid;
    }
    const int64_t from = a - window > lo ? a - window : lo, to = a + window + 1 < hi ? a + window + 1 : hi;
    for (int64_t i = from; i < to; ++i)
        if ((words[i] >> 4) == key) return true;
    return false;
}

// One block per record, its lanes striding over the sites of the resident table inside the record's span.  COMBINE: the table
// is that of a combined emit (`rf` is read).
template <bool COMBINE>
__global__ __launch_bounds__(PU_THREADS) void cover_kernel(rmr_modbam_batch b, CoverArgs ca, PileupRef rf) {
    const int64_t r = blockIdx.x;
    if (ca.status[r] != 0) return;
    const int64_t c0 = b.cigar_off[r], nc = b.cigar_off[r + 1] - c0;
    const int64_t s0 = b.seq_off[r], L = b.seq_off[r + 1] - s0;
    const int64_t rid = b.ref_id[r], pos = b.pos[r];
    if (nc <= 0 || rid < 0 || rid >= b.n_refs || pos < 0) return;
    const bool rev = (b.flag[r] & 0x10) != 0;
    const uint32_t last = b.cigar[c0 + nc - 1];
    const int last_op = (int)(last & 15u);
    const int64_t span = ca.cig_r[c0 + nc - 1] + ((last_op == 0 || last_op == 2 || last_op == 3 || last_op == 7 || last_op == 8) ? (int64_t)(last >> 4) : 0);
    if (span <= 0) return;
    // the sites that can be asked: positions [p_lo, p_hi) of the record's contig (and partition)
    const int64_t reach = COMBINE && rev ? RMR_PILEUP_MAX_MOTIF_LEN - 1 : 0;
    int64_t p_lo = pos - reach, p_hi = pos + span + reach;
    if (p_lo < 0) p_lo = 0;
    if (p_hi > ((int64_t)1 << 31)) p_hi = (int64_t)1 << 31;
    const uint64_t id = ca.part ? (uint64_t)(uint32_t)ca.part[r] : 0ull;
    const uint64_t prefix = (ca.part ? id << (ca.shift - 4) : 0ull) | ((uint64_t)rid << 32);
    const int64_t i_lo = lower_bound_u64(ca.t_keys, 0, ca.nt, prefix | ((uint64_t)p_lo << 1));
    const int64_t i_hi = lower_bound_u64(ca.t_keys, i_lo, ca.nt, prefix + ((uint64_t)p_hi << 1));  // (p_hi = 2^31 carries into the contig)
    const uint64_t want_strand = COMBINE ? 0ull : (rev ? 1ull : 0ull);
    int64_t w_lo = ca.out_off[r], w_hi = ca.out_off[r + 1];
    if (w_lo < 0) w_lo = 0;
    if (w_hi > ca.n_words) w_hi = ca.n_words;
    const int64_t off = COMBINE ? rf.off[rid] : 0, len = COMBINE ? rf.len[rid] : 0;
    for (int64_t i = i_lo + threadIdx.x; i < i_hi; i += PU_THREADS) {
        const uint64_t key = ca.t_keys[i];
        if ((key & 1ull) != want_strand) continue;
        const int64_t site = (int64_t)((key >> 1) & 0x7fffffffull);
        int64_t rp = site;
        if (COMBINE && rev) {  // the '-' focus of the first motif at the site
            bool found = false;
            for (int j = 0; j < rf.n_motifs && !found; ++j) {
                const rmr_pileup_motif &mo = rf.motifs[j];
                if (motif_window(rf.data, off, len, site - mo.focus, mo.len, mo.mask)) rp = site + (mo.len - 1 - 2 * mo.focus), found = true;
            }
            if (!found) continue;
        }
        const int64_t x = rp - pos;
        if (x < 0 || x >= span) continue;
        int64_t a = 0, z = nc;  // the last operation with cig_r <= x: the one that holds x
        while (a < z) {
            const int64_t mid = a + ((z - a) >> 1);
            if (ca.cig_r[c0 + mid] <= x) a = mid + 1;
            else z = mid;
        }
        if (a < 1) continue;
        const int64_t ci = a - 1;
        const uint32_t w = b.cigar[c0 + ci];
        const int op = (int)(w & 15u);
        const int64_t within = x - ca.cig_r[c0 + ci];
        if (within >= (int64_t)(w >> 4)) continue;  // (never for a CIGAR whose sums these are)
        int col;
        if (op == 2) col = 0;
        else if (op == 0 || op == 7 || op == 8) {
            const int64_t sp = ca.cig_q[c0 + ci] + within;
            if (sp < 0 || sp >= L) continue;
            int c = (int)b.seq[s0 + sp];
            if (c == 'U') c = 'T';
            if (rev) c = complement(c);
            col = c == ca.canonical ? 2 : 1;
        } else continue;  // an N skip
        if (slice_has_key(ca.words, w_lo, w_hi, key, rev, COMBINE && rev ? ca.fold_window : 0)) continue;  // a kept call: it is in the row
        atomicAdd(&ca.cover[i * 3 + col], 1u);
    }
}

// rocPRIM's scratch for the sort and the scan of n entries, whichever is larger
int scratch_bytes(int64_t n, int end_bit, size_t *bytes) {
    size_t sort_b = 0, scan_b = 0;
    rocprim::double_buffer<uint64_t> kb(nullptr, nullptr);
    uint32_t *v = nullptr;
    RMR_HIP(rocprim::radix_sort_keys(nullptr, sort_b, kb, (size_t)n, 0u, (unsigned)end_bit, nullptr));
    RMR_HIP(rocprim::exclusive_scan(nullptr, scan_b, v, v, 0u, (size_t)n, rocprim::plus<uint32_t>(), nullptr));
    *bytes = sort_b > scan_b ? sort_b : scan_b;
    return 0;
}

// exclusive scan of flags[0 .. n) into out, and the total
int scan_flags(rmr_pileup *p, const uint32_t *flags, uint32_t *out, int64_t n, int64_t *total) {
    rmr_engine *e = p->eng;
    size_t tb = p->tmp_bytes;
    RMR_HIP(rocprim::exclusive_scan(p->tmp, tb, flags, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), e->stream));
    uint32_t last[2] = {0, 0};
    D2H(&last[0], flags + (n - 1), 4);
    D2H(&last[1], out + (n - 1), 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    *total = (int64_t)last[0] + (int64_t)last[1];
    return 0;
}

}  // namespace

namespace rmr {

int launch_modbam_calls(rmr_engine *e, const rmr_modbam_batch &b, const PileupEmit &pe, int32_t *ords, int64_t *cig_q, int64_t *cig_r,
                        int64_t *counts, int32_t *status, const int64_t *out_off) {
    if (b.n_records <= 0) return 0;
    ProfScope ps(e, K_PILEUP_EMIT);
    if (out_off)
        hipLaunchKernelGGL(modbam_call_kernel<true>, dim3((unsigned)b.n_records), dim3(MB_THREADS), 0, e->stream, b, pe, ords, cig_q, cig_r, counts,
                           status, out_off);
    else
        hipLaunchKernelGGL(modbam_call_kernel<false>, dim3((unsigned)b.n_records), dim3(MB_THREADS), 0, e->stream, b, pe, ords, cig_q, cig_r, counts,
                           status, out_off);
    RMR_HIP(hipGetLastError());
    return 0;
}

int launch_pileup_stamp(rmr_engine *e, int64_t n_records, const int64_t *out_off, const int32_t *part, int shift, uint64_t *words,
                        int64_t n_words) {
    if (n_records <= 0) return 0;
    ProfScope ps(e, K_PILEUP_STAMP);
    hipLaunchKernelGGL(stamp_partition_kernel, dim3((unsigned)n_records), dim3(PU_THREADS), 0, e->stream, out_off, part, shift, words, n_words);
    RMR_HIP(hipGetLastError());
    return 0;
}

int launch_pileup_cover(rmr_pileup *p, const rmr_modbam_batch &b, const PileupRef &pr, bool combine, int fold_window, const int32_t *status,
                        const int64_t *cig_q, const int64_t *cig_r, const int64_t *out_off, const uint64_t *words, int64_t n_words,
                        const int32_t *part, int shift) {
    rmr_engine *e = p->eng;
    if (b.n_records <= 0 || p->nt <= 0 || !p->cover) return 0;
    ProfScope ps(e, K_PILEUP_COVER);
    const CoverArgs ca{status, cig_q, cig_r, out_off, words, n_words, part, shift, p->canonical, fold_window, p->t_keys, p->nt, p->cover};
    if (combine) hipLaunchKernelGGL(cover_kernel<true>, dim3((unsigned)b.n_records), dim3(PU_THREADS), 0, e->stream, b, ca, pr);
    else hipLaunchKernelGGL(cover_kernel<false>, dim3((unsigned)b.n_records), dim3(PU_THREADS), 0, e->stream, b, ca, pr);
    RMR_HIP(hipGetLastError());
    return 0;
}

// the work block of a pileup whose call buffer holds p->cap words: one allocation
int pileup_alloc(rmr_pileup *p) {
    const int64_t cap = p->cap;
    size_t scratch = 0;
    RMR_TRY(scratch_bytes(cap, p->end_bit, &scratch));
    p->tmp_bytes = scratch + 256;
    Stage st;  // (for its layout only)
    uint8_t *tmp;
    st.add(&p->buf[0], cap).add(&p->buf[1], cap).add(&p->head, cap).add(&p->row, cap).add(&p->keys, cap).add(&p->counts, (size_t)cap * p->ncol);
    st.add(&p->miss, cap).add(&p->miss_rank, cap).add(&p->miss_keys, cap).add(&p->miss_src, cap).add(&p->overflow, 1).add(&tmp, p->tmp_bytes);
    if (hipMalloc(&p->work, st.total) != hipSuccess) {
        (void)hipGetLastError();
        p->work = nullptr;
        RMR_FAIL(RMR_ERR_NOMEM, "a pileup buffer of %lld calls needs %zu bytes of device memory and they could not be allocated (lower the budget)",
                 (long long)cap, st.total);
    }
    for (const Stage::Slot &s : st.slots) s.set(s.where, static_cast<char *>(p->work) + s.off);
    p->tmp = tmp;
    p->work_bytes = st.total;
    p->peak_bytes = st.total;
    rmr_engine *e = p->eng;
    RMR_HIP(hipMemsetAsync(p->overflow, 0, 8, e->stream));
    return 0;
}

// sort, count and merge the p->used words of the call buffer
int pileup_flush(rmr_pileup *p) {
    rmr_engine *e = p->eng;
    const int64_t n = p->used;
    if (n <= 0) return 0;
    const int ncol = p->ncol;
    size_t need = 0;
    RMR_TRY(scratch_bytes(n, p->end_bit, &need));
    if (need > p->tmp_bytes) RMR_FAIL(RMR_ERR_HIP, "pileup: sorting %lld words needs %zu bytes of scratch, %zu were planned", (long long)n, need, p->tmp_bytes);
    ProfScope ps(e, K_PILEUP_FLUSH);
    rocprim::double_buffer<uint64_t> kb(p->buf[0], p->buf[1]);
    size_t tb = p->tmp_bytes;
    RMR_HIP(rocprim::radix_sort_keys(p->tmp, tb, kb, (size_t)n, 0u, (unsigned)p->end_bit, e->stream));
    const uint64_t *w = kb.current();
    hipLaunchKernelGGL(site_heads_kernel, grid_of(n), dim3(PU_THREADS), 0, e->stream, w, n, p->head);
    int64_t ns = 0;
    RMR_TRY(scan_flags(p, p->head, p->row, n, &ns));
    if (ns < 1 || ns > n) RMR_FAIL(RMR_ERR_HIP, "pileup: %lld sites out of %lld calls", (long long)ns, (long long)n);
    RMR_HIP(hipMemsetAsync(p->counts, 0, (size_t)ns * ncol * 4, e->stream));
    hipLaunchKernelGGL(site_runs_kernel, grid_of(n), dim3(PU_THREADS), 0, e->stream, w, n, p->head, p->row, ncol, ns, p->keys, p->counts);
    hipLaunchKernelGGL(table_hits_kernel, grid_of(ns), dim3(PU_THREADS), 0, e->stream, p->keys, p->counts, ns, ncol, p->t_keys, p->t_counts, p->nt,
                       p->miss, p->overflow);
    RMR_HIP(hipGetLastError());
    int64_t m = 0;
    RMR_TRY(scan_flags(p, p->miss, p->miss_rank, ns, &m));
    p->used = 0;  // the buffer's words are in the rows now
    p->n_flushes += 1;
    if (m == 0) return 0;
    const int64_t nn = p->nt + m;
    const size_t row_b = 8 + 4 * (size_t)ncol, keys_b = Stage::pad((size_t)nn * 8), bytes = keys_b + (size_t)nn * 4 * ncol;
    void *mem = nullptr;
    if (hipMalloc(&mem, bytes) != hipSuccess) {
        (void)hipGetLastError();
        RMR_FAIL(RMR_ERR_NOMEM, "the pileup table of %lld sites (%zu bytes each) needs %zu bytes of device memory and they could not be allocated",
                 (long long)nn, row_b, bytes);
    }
    uint64_t *o_keys = static_cast<uint64_t *>(mem);
    uint32_t *o_counts = reinterpret_cast<uint32_t *>(static_cast<char *>(mem) + keys_b);
    hipLaunchKernelGGL(compact_misses_kernel, grid_of(ns), dim3(PU_THREADS), 0, e->stream, p->keys, p->miss, p->miss_rank, ns, m, p->miss_keys,
                       p->miss_src);
    if (p->nt > 0)
        hipLaunchKernelGGL(merge_old_kernel, grid_of(p->nt), dim3(PU_THREADS), 0, e->stream, p->t_keys, p->t_counts, p->nt, p->miss_keys, m, ncol,
                           o_keys, o_counts);
    hipLaunchKernelGGL(merge_new_kernel, grid_of(m), dim3(PU_THREADS), 0, e->stream, p->miss_keys, p->miss_src, m, p->counts, p->t_keys, p->nt, ncol,
                       o_keys, o_counts);
    const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(e->stream);  // the old table goes when nothing reads it any more
    if (launched != hipSuccess || done != hipSuccess) {
        (void)hipFree(mem);
        RMR_FAIL(RMR_ERR_HIP, "HIP error %s in the pileup merge", hipGetErrorString(launched != hipSuccess ? launched : done));
    }
    if (p->work_bytes + p->t_bytes + bytes > p->peak_bytes) p->peak_bytes = p->work_bytes + p->t_bytes + bytes;
    if (p->t_mem) (void)hipFree(p->t_mem);
    p->t_mem = mem, p->t_bytes = bytes, p->t_keys = o_keys, p->t_counts = o_counts, p->nt = nn;
    return 0;
}

// n words (device) into the call buffer, flushing whenever it is full
int pileup_append(rmr_pileup *p, const uint64_t *words, int64_t n) {
    rmr_engine *e = p->eng;
    if (n > 0) {
        p->finished = false;
        if (p->cover) {  // counted against a table that is about to change: dropped once nothing writes it any more
            RMR_HIP(hipStreamSynchronize(e->stream));
            (void)hipFree(p->cover);
            p->cover = nullptr, p->cover_bytes = 0;
        }
    }
    for (int64_t at = 0; at < n;) {
        const int64_t take = std::min(n - at, p->cap - p->used);
        RMR_HIP(hipMemcpyAsync(p->buf[0] + p->used, words + at, (size_t)take * 8, hipMemcpyDeviceToDevice, e->stream));
        p->used += take, at += take, p->n_calls += take;
        if (p->used == p->cap) RMR_TRY(pileup_flush(p));
    }
    return 0;
}

}  // namespace rmr
