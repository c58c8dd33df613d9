// k_metrics.hip - per-base signal metrics of a batch of reads and the k-mer level table estimated from them:
//   rmr_base_metrics       src/remora/metrics.py:45-117 (METRIC_FUNCS) as io.Read.compute_per_base_metric applies them
//                          (src/remora/io.py:2394-2480), for every base of every read of a batch in one launch
//   rmr_region_base_metrics / rmr_region_signals   the same metrics, and the normalised samples, of only the bases of a read that lie
//                          in a reference region (io.get_ref_reg_sample_metrics :840-886, Read.extract_ref_reg :2342-2392), for a
//                          list of (read, region) pairs of a resident batch
//   rmr_site_kmer_levels   io.get_region_kmers (src/remora/io.py:930-982) + the aggregation of `remora analyze
//                          estimate_kmer_levels` (src/remora/parsers.py:2296-2331): median per reference site, then per k-mer
//
// base_metrics_kernel.  One wave owns 64 consecutive bases of ONE read, counted from the read's first base, so what a base's
// sums look like depends on its read alone and not on where the read stands in the batch (the results are the same bits for a
// read alone and inside any batch).  The wave does not walk its bases: it walks the SAMPLES those 64 bases own, 64 at a time,
// lane j taking sample j.  Each lane finds its sample's base by bisecting the wave's prefix sum of dwells in LDS (6 steps),
// normalises the sample in float64 (norm_sample_f64: the expression of normalise_kernel), and a segmented inclusive scan
// across the lanes, keyed by the base, leaves every base's partial sums in the last lane of its segment, which adds them
// to the base's accumulators in LDS.  A stalled base of 5000 samples is 79 such rounds shared by all lanes, not one lane's
// serial loop; a typical group (64 bases x 5-15 samples) is 5-15 rounds.  The sums are direct float64 sums of the base's own
// samples - no whole-read cumulative sum, whose rounding grows with the read.
// Traffic: 2 B per sample in (plus 8 B per base of mapping), 36 B per base out: HBM-bound by design, see DESIGN.md.
//
// The level table.  Every base of every reference-anchored read is one observation: (site, trimmean, base), `site` a 64-bit
// key that grows by one per base in READ orientation on both strands.  Two stable LSD radix sorts (rocPRIM, by value, then by
// site) order the observations by (site, value) with the non-finite values last in their site; a thread per site takes the
// median of the finite ones (numpy's: mean of the two middle values for an even count) and looks its k-mer window up among
// the sorted sites - the union of the reads of that strand, as get_ref_seq_from_reads assembles it; the same two sorts by
// (k-mer, site median) and a thread per k-mer give the table.  Nothing but the 4^k results crosses PCIe.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "rmr_geometry.h"
#include "rmr_internal.h"

namespace rmr {

struct BaseMetricsArgs {
    const int16_t *dacs;
    const int64_t *sig_off, *seq_to_sig, *seq_off;
    const double *shift, *scale;
    float *dwell;
    double *mean, *sd, *trimmean, *trimsd;
    int start_trim, end_trim;
};

// 64-bit values across lanes as two 32-bit shuffles
__device__ __forceinline__ double shfl_up_f64(double v, int off) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_up(lo, off);
    hi = __shfl_up(hi, off);
    return __hiloint2double(hi, lo);
}

// LDS hand-over between the lanes of ONE wave: what every lane wrote is visible to every lane behind it (the LDS serves a wave's
// instructions in order; the fences keep the compiler from moving accesses across)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

constexpr int BM_WAVES = 4;  // waves (groups of 64 bases) per block

// One wave, one group of 64 bases: bases g0 .. g0 + 63 of a read of nb bases whose mapping (nb + 1 entries) is `map` and whose
// own signal is dacs[0 .. sig_len).  The summation of base_metrics_kernel and region_metrics_kernel: what a base's sums look like
// depends on the read and on g0 alone, and both kernels hand over g0 = a multiple of 64 counted from the read's first base, so a
// base has the same bits wherever it is asked for.  `Sink::put(bi, dwell, mean, has, sum x^2, trimmean, has_t, trimmed sum x^2,
// trimmed dwell)` is called by the lane of every base bi < nb of the group and decides where (and whether) the results go; it
// forms the two sd itself (sd_of), and only where somebody wants them.  s_pre / s_start / s_acc: this wave's LDS.
template <class Sink>
__device__ __forceinline__ void base_group_metrics(const int16_t *dacs, int64_t sig_len, const int64_t *map, int64_t nb, int64_t g0, double sh,
                                                   double sc, int st, int en, int lane, int64_t *s_pre, int64_t *s_start, double (*s_acc)[64],
                                                   const Sink &sink) {
    const int64_t bi = g0 + lane;
    const bool live = bi < nb;
    int64_t ms = 0, me = 0;
    if (live) { ms = map[bi]; me = map[bi + 1]; }
    // the samples that are summed never leave the read's own signal, whatever the mapping says
    const int64_t cs = min(max(ms, (int64_t)0), sig_len), ce = min(max(me, cs), sig_len);
    const int64_t dw = ce - cs;
    int64_t inc = dw;  // inclusive prefix sum across the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int lo = (int)(uint32_t)inc, hi = (int)(inc >> 32);
        lo = __shfl_up(lo, off);
        hi = __shfl_up(hi, off);
        if (lane >= off) inc += (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    }
    s_pre[lane + 1] = inc;
    if (lane == 0) s_pre[0] = 0;
    s_start[lane] = cs;
#pragma unroll
    for (int q = 0; q < 4; ++q) s_acc[q][lane] = 0.0;
    wave_lds_sync();
    const int64_t total = s_pre[64];
    for (int64_t j0 = 0; j0 < total; j0 += 64) {
        const int64_t j = j0 + lane;
        const bool valid = j < total;
        int b = 64;
        double x = 0.0, xx = 0.0, tx = 0.0, txx = 0.0;
        if (valid) {
            int lo = 0, hi = 64;  // the base that owns sample j: the first b with pre[b + 1] > j
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_pre[mid + 1] <= j) lo = mid + 1; else hi = mid;
            }
            b = lo;
            const int64_t k = j - s_pre[b], n = s_pre[b + 1] - s_pre[b];
            x = norm_sample_f64(dacs[s_start[b] + k], sh, sc);
            xx = __dmul_rn(x, x);
            if (k >= st && k < n - en) { tx = x; txx = xx; }
        }
        // segmented inclusive scan: lanes of one base are neighbours, b never decreases with the lane
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int pb = __shfl_up(b, off);
            const double px = shfl_up_f64(x, off), pxx = shfl_up_f64(xx, off), ptx = shfl_up_f64(tx, off), ptxx = shfl_up_f64(txx, off);
            if (lane >= off && pb == b) { x = __dadd_rn(x, px); xx = __dadd_rn(xx, pxx); tx = __dadd_rn(tx, ptx); txx = __dadd_rn(txx, ptxx); }
        }
        const int nxt = __shfl_down(b, 1);
        if (valid && (lane == 63 || nxt != b)) {  // one lane per base and round: a plain read-modify-write
            s_acc[0][b] = __dadd_rn(s_acc[0][b], x);
            s_acc[1][b] = __dadd_rn(s_acc[1][b], xx);
            s_acc[2][b] = __dadd_rn(s_acc[2][b], tx);
            s_acc[3][b] = __dadd_rn(s_acc[3][b], txx);
        }
        wave_lds_sync();
    }
    if (!live) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const float dwell_f = (float)(me - ms);                     // np.diff(seq_to_sig).astype(float32)
    const float tdwell_f = fmaxf(0.f, dwell_f - (float)st - (float)en);  // np.maximum(0, dwells - st - en), float32 as there
    const bool has = dw > 0 && me - ms == dw, has_t = has && tdwell_f > 0.f;  // (a mapping that leaves the signal: NaN, nothing half-summed)
    const double sx = s_acc[0][lane], sxx = s_acc[1][lane], stx = s_acc[2][lane], stxx = s_acc[3][lane];
    const double m = has ? sx / (double)dwell_f : nan;
    const double tm = has_t ? stx / (double)tdwell_f : nan;
    sink.put(bi, dwell_f, m, has, sxx, tm, has_t, stxx, tdwell_f);
}

// sd = sqrt(max(0, E[x^2] - mean^2)), evaluated only where somebody wants it
__device__ __forceinline__ double sd_of(bool has, double sxx, double n, double m) {
    return has ? sqrt(fmax(__dsub_rn(sxx / n, __dmul_rn(m, m)), 0.0)) : __longlong_as_double(0x7ff8000000000000LL);
}

struct BatchSink {  // base bi of the read -> entry b0 + bi of the batch's per-base arrays
    const BaseMetricsArgs &a;
    int64_t b0;
    __device__ __forceinline__ void put(int64_t bi, float dwell_f, double m, bool has, double sxx, double tm, bool has_t, double stxx,
                                        float tdwell_f) const {
        const int64_t out = b0 + bi;
        if (a.dwell) a.dwell[out] = dwell_f;
        if (a.mean) a.mean[out] = m;
        if (a.trimmean) a.trimmean[out] = tm;
        if (a.sd) a.sd[out] = sd_of(has, sxx, (double)dwell_f, m);
        if (a.trimsd) a.trimsd[out] = sd_of(has_t, stxx, (double)tdwell_f, tm);
    }
};

__global__ __launch_bounds__(64 * BM_WAVES) void base_metrics_kernel(BaseMetricsArgs a) {
    __shared__ int64_t s_pre[BM_WAVES][65];    // prefix sum of the group's dwells; [64] = the group's samples
    __shared__ int64_t s_start[BM_WAVES][64];  // first sample of every base, read-local
    __shared__ double s_acc[BM_WAVES][4][64];  // per base: sum x, sum x^2, and the same inside the trims
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r = blockIdx.x;
    const int64_t b0 = a.seq_off[r], nb = a.seq_off[r + 1] - b0;
    const int64_t g0 = ((int64_t)blockIdx.y * BM_WAVES + wave) * 64;  // the group's first base, read-local
    if (g0 >= nb) return;                                               // (wave-uniform; no block barrier below)
    const int64_t s0 = a.sig_off[r];
    base_group_metrics(a.dacs + s0, a.sig_off[r + 1] - s0, a.seq_to_sig + b0 + r, nb, g0, a.shift[r], a.scale[r], a.start_trim, a.end_trim, lane,
                       s_pre[wave], s_start[wave], s_acc[wave], BatchSink{a, b0});
}

int launch_base_metrics(rmr_engine *e, int64_t n_reads, int64_t max_read_bases, const BaseMetricsArgs &a) {
    const int64_t per_block = 64 * BM_WAVES;
    const int64_t gy = (max_read_bases + per_block - 1) / per_block;
    if (gy > 65535) RMR_FAIL(RMR_ERR_INVALID, "rmr_base_metrics: a read of %lld bases is beyond the launch grid (16.7 M)", (long long)max_read_bases);
    ProfScope ps(e, K_BASE_METRICS);
    hipLaunchKernelGGL(base_metrics_kernel, dim3((unsigned)n_reads, (unsigned)gy), dim3(64 * BM_WAVES), 0, e->stream, a);
    RMR_HIP(hipGetLastError());
    return 0;
}

// ======================================================================================
// regions: the bases (and the samples) of a read that lie in a reference region, for a list of (read, region) pairs
// ======================================================================================
// A pair, 8 x int64: the read (index into the batch), [first, last) its bases inside the region (read-local), `lead` region
// positions in front of the read's first base, the pair's `row` of the output, the region's length, `flip` (the row is written
// back to front: reference orientation on the reverse strand), one spare.  The host plans the pairs (io.plan_region_pairs).
constexpr int RP_READ = 0, RP_FIRST = 1, RP_LAST = 2, RP_LEAD = 3, RP_ROW = 4, RP_RLEN = 5, RP_FLIP = 6, RP_WORDS = 8;

struct RegionMetricsArgs {
    const int16_t *dacs;
    const int64_t *sig_off, *seq_to_sig, *seq_off;
    const double *shift, *scale;
    const int64_t *pairs;
    int64_t n_reads, rows, width;
    double *dwell, *mean, *sd, *trimmean, *trimsd;  // [rows][width] each, any may be NULL
    int32_t *status;
    int start_trim, end_trim;
};

struct RegionPair {
    int64_t read, first, last, lead, row, rlen;
    bool flip;
};
__device__ __forceinline__ RegionPair load_pair(const int64_t *pairs, int64_t p) {
    const int64_t *w = pairs + p * RP_WORDS;
    return RegionPair{w[RP_READ], w[RP_FIRST], w[RP_LAST], w[RP_LEAD], w[RP_ROW], w[RP_RLEN], w[RP_FLIP] != 0};
}
// what the wrapper checks before the launch, once more where an index would be formed from it: the pair's span inside its read
// (all rmr_region_signals uses of a pair beside its flip), and its place in the region and in the output
__device__ __forceinline__ bool span_fits(const RegionPair &q, int64_t n_reads, const int64_t *seq_off) {
    if (q.read < 0 || q.read >= n_reads) return false;
    const int64_t nb = seq_off[q.read + 1] - seq_off[q.read];
    return q.first >= 0 && q.first < q.last && q.last <= nb;
}
__device__ __forceinline__ bool pair_fits(const RegionPair &q, int64_t n_reads, const int64_t *seq_off, int64_t rows, int64_t width) {
    return span_fits(q, n_reads, seq_off) && q.lead >= 0 && q.rlen > 0 && q.rlen <= width && q.last - q.first <= q.rlen &&
           q.lead <= q.rlen - (q.last - q.first) && q.row >= 0 && q.row < rows;
}

struct RegionSink {  // base bi of the read -> column lead + bi - first of the pair's row (counted from the row's end when flipped)
    const RegionMetricsArgs &a;
    const RegionPair &q;
    __device__ __forceinline__ void put(int64_t bi, float dwell_f, double m, bool has, double sxx, double tm, bool has_t, double stxx,
                                        float tdwell_f) const {
        if (bi < q.first || bi >= q.last) return;  // (the rest of the 64-base group: summed for the grouping's sake, not asked for)
        const int64_t pos = q.lead + (bi - q.first);
        const int64_t out = q.row * a.width + (q.flip ? q.rlen - 1 - pos : pos);
        if (a.dwell) a.dwell[out] = (double)dwell_f;
        if (a.mean) a.mean[out] = m;
        if (a.trimmean) a.trimmean[out] = tm;
        if (a.sd) a.sd[out] = sd_of(has, sxx, (double)dwell_f, m);
        if (a.trimsd) a.trimsd[out] = sd_of(has_t, stxx, (double)tdwell_f, tm);
    }
};

// grid (pairs, groups of BM_WAVES 64-base groups): wave w of block y runs group first / 64 + y * BM_WAVES + w of the pair's read.
// Block y = 0 also writes the NaN of every column of the row that the read does not cover, and the pair's status word.
__global__ __launch_bounds__(64 * BM_WAVES) void region_metrics_kernel(RegionMetricsArgs a) {
    __shared__ int64_t s_pre[BM_WAVES][65];
    __shared__ int64_t s_start[BM_WAVES][64];
    __shared__ double s_acc[BM_WAVES][4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const RegionPair q = load_pair(a.pairs, blockIdx.x);
    const bool fits = pair_fits(q, a.n_reads, a.seq_off, a.rows, a.width);
    if (blockIdx.y == 0 && threadIdx.x == 0) a.status[blockIdx.x] = fits ? 0 : 1;
    if (!fits) return;  // (block-uniform) a pair that does not fit writes nothing
    if (blockIdx.y == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        const int64_t covered = q.last - q.first;
        for (int64_t c = threadIdx.x; c < a.width; c += 64 * BM_WAVES) {
            const int64_t pos = c < q.rlen ? (q.flip ? q.rlen - 1 - c : c) : -1;
            if (pos >= q.lead && pos < q.lead + covered) continue;
            const int64_t out = q.row * a.width + c;
            if (a.dwell) a.dwell[out] = nan;
            if (a.mean) a.mean[out] = nan;
            if (a.sd) a.sd[out] = nan;
            if (a.trimmean) a.trimmean[out] = nan;
            if (a.trimsd) a.trimsd[out] = nan;
        }
    }
    const int64_t r = q.read;
    const int64_t b0 = a.seq_off[r], nb = a.seq_off[r + 1] - b0;
    const int64_t g0 = (q.first / 64 + (int64_t)blockIdx.y * BM_WAVES + wave) * 64;  // a group of base_metrics_kernel: counted from base 0
    if (g0 >= q.last) return;                                                          // (wave-uniform; no block barrier below)
    const int64_t s0 = a.sig_off[r];
    base_group_metrics(a.dacs + s0, a.sig_off[r + 1] - s0, a.seq_to_sig + b0 + r, nb, g0, a.shift[r], a.scale[r], a.start_trim, a.end_trim, lane,
                       s_pre[wave], s_start[wave], s_acc[wave], RegionSink{a, q});
}

struct RegionSignalsArgs {
    const int16_t *dacs;
    const int64_t *sig_off, *seq_to_sig, *seq_off;
    const double *shift, *scale;
    const int64_t *pairs, *sig_out_off, *map_out_off;  // offsets: [n_pairs + 1], the pairs' samples / map entries back to back
    int64_t n_reads, sig_capacity, map_capacity;
    void *sig_out;  // f64 (normalised) or i16 (RAW)
    int64_t *map_out, *sig_start;
    int32_t *status;
};

// grid (pairs, slices): the samples map[first] .. map[last] of the pair's read, (dacs - shift) / scale in float64 (RAW: the int16
// samples themselves), and the last - first + 1 mapping entries re-based on the first sample; flipped: samples back to front and
// map[-1] - map[::-1].  status 1: the pair or its slots do not fit; 2: the mapping leaves the read's signal there.
template <bool RAW>
__global__ __launch_bounds__(256) void region_signals_kernel(RegionSignalsArgs a) {
    const int64_t p = blockIdx.x;
    const RegionPair q = load_pair(a.pairs, p);
    int st = 0;
    int64_t ms = 0, me = 0, so = 0, mo = 0;
    const int64_t *map = nullptr;
    const int16_t *dacs = nullptr;
    if (!span_fits(q, a.n_reads, a.seq_off)) st = 1;  // (lead, row and region length are the metrics kernel's business)
    if (!st) {
        const int64_t r = q.read, b0 = a.seq_off[r], s0 = a.sig_off[r], sig_len = a.sig_off[r + 1] - s0;
        map = a.seq_to_sig + b0 + r;
        dacs = a.dacs + s0;
        ms = map[q.first];
        me = map[q.last];
        so = a.sig_out_off[p];
        mo = a.map_out_off[p];
        if (ms < 0 || me < ms || me > sig_len) st = 2;
        else if (so < 0 || a.sig_out_off[p + 1] - so != me - ms || a.sig_out_off[p + 1] > a.sig_capacity || mo < 0 ||
                 a.map_out_off[p + 1] - mo != q.last - q.first + 1 || a.map_out_off[p + 1] > a.map_capacity)
            st = 1;
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        a.status[p] = st;
        if (!st) a.sig_start[p] = ms;
    }
    if (st) return;
    const int64_t n = me - ms, nm = q.last - q.first + 1;
    const int64_t t0 = (int64_t)blockIdx.y * blockDim.x + threadIdx.x, step = (int64_t)gridDim.y * blockDim.x;
    const double sh = a.shift[q.read], sc = a.scale[q.read];
    for (int64_t i = t0; i < n; i += step) {
        const int16_t d = dacs[ms + (q.flip ? n - 1 - i : i)];
        if (RAW) ((int16_t *)a.sig_out)[so + i] = d;
        else ((double *)a.sig_out)[so + i] = norm_sample_f64(d, sh, sc);
    }
    for (int64_t k = t0; k < nm; k += step) a.map_out[mo + k] = q.flip ? me - map[q.last - k] : map[q.first + k] - ms;
}

// ======================================================================================
// site and k-mer aggregation
// ======================================================================================
// float64 -> uint64 whose unsigned order is the order of the values; every non-finite value becomes the largest key
__device__ __forceinline__ uint64_t sortable_f64(double v) {
    if (!(fabs(v) <= 1.7976931348623157e308)) return ~0ULL;
    const uint64_t u = (uint64_t)__double_as_longlong(v + 0.0);  // (-0.0 + 0.0 = +0.0: one key for both zeros)
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double unsortable_f64(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
    return __longlong_as_double((long long)u);
}
constexpr uint64_t NOT_A_SITE = ~0ULL;

// observation i (base i of the concatenated reads): key of its value, its own index as payload
__global__ void obs_value_keys_kernel(const double *__restrict__ vals, int64_t n, uint64_t *__restrict__ vkey, uint64_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    vkey[i] = sortable_f64(vals[i]);
    idx[i] = (uint64_t)i;
}
// the site of observation idx[p]: site0 of its read + its place in the read
__global__ void obs_site_keys_kernel(const uint64_t *__restrict__ idx, int64_t n, const int64_t *__restrict__ seq_off, int64_t n_reads,
                                     const int64_t *__restrict__ site0, uint64_t *__restrict__ skey) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t i = (int64_t)idx[p];
    const int64_t r = ub_right(seq_off, n_reads + 1, i) - 1;  // last read with seq_off[r] <= i (empty reads are passed over)
    skey[p] = (uint64_t)(site0[r] + (i - seq_off[r]));
}

__device__ __forceinline__ int64_t lb_u64(const uint64_t *a, int64_t n, uint64_t v) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

// skey / idx: the observations ordered by (site, value).  The first observation of every site writes the site's k-mer and the
// key of its median; every other position (and a site that is not reported) writes NOT_A_SITE.
__global__ void site_median_kernel(const uint64_t *__restrict__ skey, const uint64_t *__restrict__ idx, int64_t n, const double *__restrict__ vals,
                                   const int8_t *__restrict__ int_seq, int kb, int ka, int64_t min_cov, uint64_t key_lo, uint64_t key_hi,
                                   uint64_t *__restrict__ kkey, uint64_t *__restrict__ mkey) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    uint64_t kk = NOT_A_SITE, mk = NOT_A_SITE;
    const uint64_t key = skey[p];
    // a site outside [key_lo, key_hi) is a margin of a range: its observations serve the k-mers of its neighbours only
    if ((p == 0 || skey[p - 1] != key) && key >= key_lo && key < key_hi) {
        const int64_t end = lb_u64(skey, n, key + 1);
        int64_t lo = p, hi = end;  // the finite values stand in front: first position of the site whose value is not finite
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (sortable_f64(vals[idx[mid]]) != ~0ULL) lo = mid + 1; else hi = mid; }
        const int64_t c = lo - p;
        if (c >= 1 && c >= min_cov) {
            uint64_t code = 0;
            bool ok = true;
            for (int j = -kb; j <= ka && ok; ++j) {  // the bases around the site in read orientation, from whichever read covers them
                const uint64_t want = key + (uint64_t)(int64_t)j;
                const int64_t q = (j == 0) ? p : lb_u64(skey, n, want);
                if (q >= n || skey[q] != want) { ok = false; break; }
                const int b = int_seq[idx[q]];
                if (b < 0 || b > 3) { ok = false; break; }
                code = code * 4 + (uint64_t)b;
            }
            if (ok) {
                const double lo_v = vals[idx[p + (c - 1) / 2]], hi_v = vals[idx[p + c / 2]];
                kk = code;
                mk = sortable_f64((c & 1) ? lo_v : __dadd_rn(lo_v, hi_v) / 2.0);
            }
        }
    }
    kkey[p] = kk;
    mkey[p] = mk;
}

// kkey / mkey ordered by (k-mer, site median), holding every site of the k-mers [m0, m1): a thread per k-mer of them
__global__ void kmer_median_kernel(const uint64_t *__restrict__ kkey, const uint64_t *__restrict__ mkey, int64_t n, int64_t m0, int64_t m1,
                                   double *__restrict__ levels, int64_t *__restrict__ counts) {
    const int64_t m = m0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m1) return;
    const int64_t lo = lb_u64(kkey, n, (uint64_t)m), hi = lb_u64(kkey, n, (uint64_t)m + 1);
    const int64_t c = hi - lo;
    double lv = __longlong_as_double(0x7ff8000000000000LL);
    if (c > 0) {
        const double a = unsortable_f64(mkey[lo + (c - 1) / 2]), b = unsortable_f64(mkey[lo + c / 2]);
        lv = (c & 1) ? a : __dadd_rn(a, b) / 2.0;
    }
    levels[m] = lv;
    if (counts) counts[m] = c;
}

// the reported sites in the order of the table: site_kmer / site_level [n_sites]
__global__ void site_list_kernel(const uint64_t *__restrict__ kkey, const uint64_t *__restrict__ mkey, int64_t n_sites, int32_t *__restrict__ site_kmer,
                                 double *__restrict__ site_level) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_sites) return;
    site_kmer[p] = (int32_t)kkey[p];
    site_level[p] = unsortable_f64(mkey[p]);
}

// A slot of an output list for every lane with `mine`, drawn from one cursor with one integer atomic per wave.  The order of the
// list is whatever the waves' arrival makes it; what is made of the list is sorted by the whole entry, so no result depends on it.
// Every lane of the wave has to get here.
__device__ __forceinline__ int64_t wave_slot(bool mine, unsigned long long *cursor) {
    const unsigned long long mask = __ballot(mine);
    if (!mask) return -1;
    const int lane = (int)(threadIdx.x & 63), leader = __ffsll((long long)mask) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader);
    return mine ? (int64_t)(base + (unsigned long long)__popcll(mask & ((1ULL << lane) - 1))) : -1;
}

// the reported sites among kkey / mkey [n] (site_median_kernel) appended to list_kmer / list_level; a slot beyond `capacity` is
// counted by the cursor and not written
__global__ void site_append_kernel(const uint64_t *__restrict__ kkey, const uint64_t *__restrict__ mkey, int64_t n, unsigned long long *cursor,
                                   int64_t capacity, int32_t *__restrict__ list_kmer, double *__restrict__ list_level) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t kk = p < n ? kkey[p] : NOT_A_SITE;
    const int64_t slot = wave_slot(kk != NOT_A_SITE, cursor);
    if (slot < 0 || slot >= capacity) return;
    list_kmer[slot] = (int32_t)kk;
    list_level[slot] = unsortable_f64(mkey[p]);
}

// counts[m] += the entries of kmer[n] equal to m (all in [0, n_kmers)): integer atomics, per block in LDS while the table fits
constexpr int KMER_COUNT_LDS = 4096, KMER_COUNT_BLOCKS = 1024;
__global__ void kmer_count_kernel(const int32_t *__restrict__ kmer, int64_t n, int64_t n_kmers, unsigned long long *__restrict__ counts) {
    __shared__ unsigned int h[KMER_COUNT_LDS];
    const bool in_lds = n_kmers <= KMER_COUNT_LDS;  // a block sees n / gridDim.x < 2^32 entries (n <= 2^39, KMER_COUNT_BLOCKS blocks)
    if (in_lds) {
        for (int64_t m = threadIdx.x; m < n_kmers; m += blockDim.x) h[m] = 0;
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = kmer[i];
        if (m < 0 || m >= n_kmers) continue;
        if (in_lds) atomicAdd(&h[m], 1u);
        else atomicAdd(&counts[m], 1ULL);
    }
    if (in_lds) {
        __syncthreads();
        for (int64_t m = threadIdx.x; m < n_kmers; m += blockDim.x)
            if (h[m]) atomicAdd(&counts[m], (unsigned long long)h[m]);
    }
}

// the sites of the k-mers [m0, m1) out of the lists, as sort keys: kkey / mkey [capacity]
__global__ void kmer_group_gather_kernel(const int32_t *__restrict__ list_kmer, const double *__restrict__ list_level, int64_t n, int64_t m0, int64_t m1,
                                         unsigned long long *cursor, int64_t capacity, uint64_t *__restrict__ kkey, uint64_t *__restrict__ mkey) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t m = p < n ? (int64_t)list_kmer[p] : -1;
    const int64_t slot = wave_slot(m >= m0 && m < m1, cursor);
    if (slot < 0 || slot >= capacity) return;
    kkey[slot] = (uint64_t)m;
    mkey[slot] = sortable_f64(list_level[p]);
}

// keys / vals sorted by bits [0, end_bit) of `keys` (stable) into keys_out / vals_out
static int sort_pairs(rmr_engine *e, void *tmp, size_t tmp_bytes, uint64_t *keys, uint64_t *keys_out, uint64_t *vals, uint64_t *vals_out, int64_t n,
                      unsigned end_bit = 64) {
    RMR_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, keys, keys_out, vals, vals_out, (size_t)n, 0, end_bit, e->stream));
    return 0;
}

struct DevFree {  // the temporaries of one call
    std::vector<void *> ptrs;
    ~DevFree() { for (void *p : ptrs) (void)hipFree(p); }
    int get(void **out, size_t bytes) {
        RMR_HIP(hipMalloc(out, bytes ? bytes : 1));
        ptrs.push_back(*out);
        return 0;
    }
};

struct SortBufs {  // four key / payload arrays of `n` 8-byte items and the radix sort's own scratch
    uint64_t *A = nullptr, *B = nullptr, *C = nullptr, *D = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    int get(rmr_engine *e, DevFree &pool, int64_t n) {
        RMR_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, A, B, C, D, (size_t)n, 0, 64, e->stream));
        RMR_TRY(pool.get((void **)&A, n * 8));
        RMR_TRY(pool.get((void **)&B, n * 8));
        RMR_TRY(pool.get((void **)&C, n * 8));
        RMR_TRY(pool.get((void **)&D, n * 8));
        RMR_TRY(pool.get(&tmp, tmp_bytes));
        return 0;
    }
};

// Stage 1, n > 0 observations: the median of every site with a key in [key_lo, key_hi).  -> s.A[p]: the k-mer of the site whose
// first observation stands at p of the (site, value) order, s.D[p]: the key of its median; NOT_A_SITE everywhere else.
static int site_stage(rmr_engine *e, SortBufs &s, int64_t n_reads, const int64_t *seq_off, const int64_t *site0, int64_t n, const double *vals,
                      const int8_t *int_seq, int kb, int ka, int64_t min_cov, uint64_t key_lo, uint64_t key_hi) {
    const unsigned T = 256;
    const dim3 grid((unsigned)((n + T - 1) / T));
    // by value (A: value keys, C: indices -> B, D), then by site (A: site keys of D -> C keys, B indices)
    hipLaunchKernelGGL(obs_value_keys_kernel, grid, dim3(T), 0, e->stream, vals, n, s.A, s.C);
    RMR_TRY(sort_pairs(e, s.tmp, s.tmp_bytes, s.A, s.B, s.C, s.D, n));
    hipLaunchKernelGGL(obs_site_keys_kernel, grid, dim3(T), 0, e->stream, s.D, n, seq_off, n_reads, site0, s.A);
    RMR_TRY(sort_pairs(e, s.tmp, s.tmp_bytes, s.A, s.C, s.D, s.B, n));
    // C: sites, B: indices, ordered by (site, value) -> A: k-mer of every site, D: key of its median
    hipLaunchKernelGGL(site_median_kernel, grid, dim3(T), 0, e->stream, s.C, s.B, n, vals, int_seq, kb, ka, min_cov, key_lo, key_hi, s.A, s.D);
    RMR_HIP(hipGetLastError());
    return 0;
}

int run_site_kmer_levels(rmr_engine *e, int64_t n_reads, const int64_t *seq_off, const int64_t *site0, int64_t n, const double *vals,
                         const int8_t *int_seq, int kb, int ka, int64_t min_cov, double *levels, int64_t *counts, int32_t *site_kmer,
                         double *site_level, int64_t *n_sites) {
    const int64_t n_kmers = (int64_t)1 << (2 * (kb + ka + 1));
    const unsigned T = 256;
    SortBufs s;
    DevFree pool;
    int64_t sites = 0;
    if (n > 0) {
        RMR_TRY(s.get(e, pool, n));
        ProfScope ps(e, K_SITE_KMER_LEVELS);
        RMR_TRY(site_stage(e, s, n_reads, seq_off, site0, n, vals, int_seq, kb, ka, min_cov, 0, NOT_A_SITE));
        // by median (D keys, A payload -> B, C), then by k-mer (C keys, B payload -> A, D)
        RMR_TRY(sort_pairs(e, s.tmp, s.tmp_bytes, s.D, s.B, s.A, s.C, n));
        RMR_TRY(sort_pairs(e, s.tmp, s.tmp_bytes, s.C, s.A, s.B, s.D, n));
        RMR_HIP(hipGetLastError());
    }
    // A: k-mers ascending (NOT_A_SITE last), D: their sites' medians ascending inside each k-mer
    int64_t *cnt = counts;
    if (!cnt) RMR_TRY(pool.get((void **)&cnt, n_kmers * 8));
    {
        ProfScope ps(e, K_SITE_KMER_LEVELS);
        hipLaunchKernelGGL(kmer_median_kernel, dim3((unsigned)((n_kmers + T - 1) / T)), dim3(T), 0, e->stream, s.A, s.D, n, (int64_t)0, n_kmers, levels,
                           cnt);
        RMR_HIP(hipGetLastError());
    }
    if (n > 0 && (site_kmer || n_sites)) {  // the reported sites stand in front of A / D: as many as the k-mers count together
        std::vector<int64_t> h((size_t)n_kmers);
        RMR_HIP(hipMemcpyAsync(h.data(), cnt, n_kmers * 8, hipMemcpyDeviceToHost, e->stream));
        RMR_HIP(hipStreamSynchronize(e->stream));
        for (int64_t c : h) sites += c;
        if (site_kmer && sites > 0) {
            hipLaunchKernelGGL(site_list_kernel, dim3((unsigned)((sites + T - 1) / T)), dim3(T), 0, e->stream, s.A, s.D, sites, site_kmer, site_level);
            RMR_HIP(hipGetLastError());
        }
    }
    if (n_sites) *n_sites = sites;
    RMR_HIP(hipStreamSynchronize(e->stream));  // the temporaries are freed on return
    return 0;
}

// Stage 1 alone, for one range of the key space: the sites of [key_lo, key_hi) join the caller's lists and its counts per k-mer
int run_site_medians(rmr_engine *e, int64_t n_reads, const int64_t *seq_off, const int64_t *site0, int64_t n, const double *vals,
                     const int8_t *int_seq, int kb, int ka, int64_t min_cov, uint64_t key_lo, uint64_t key_hi, int32_t *list_kmer,
                     double *list_level, int64_t list_len, int64_t capacity, int64_t *site_counts, int64_t *n_appended) {
    const int64_t n_kmers = (int64_t)1 << (2 * (kb + ka + 1));
    const unsigned T = 256;
    *n_appended = 0;
    if (n == 0) return 0;
    SortBufs s;
    DevFree pool;
    unsigned long long *cursor = nullptr, took = 0;
    RMR_TRY(s.get(e, pool, n));
    RMR_TRY(pool.get((void **)&cursor, 8));
    {
        ProfScope ps(e, K_SITE_KMER_LEVELS);
        RMR_HIP(hipMemsetAsync(cursor, 0, 8, e->stream));
        RMR_TRY(site_stage(e, s, n_reads, seq_off, site0, n, vals, int_seq, kb, ka, min_cov, key_lo, key_hi));
        hipLaunchKernelGGL(site_append_kernel, dim3((unsigned)((n + T - 1) / T)), dim3(T), 0, e->stream, s.A, s.D, n, cursor, capacity - list_len,
                           list_kmer + list_len, list_level + list_len);
        RMR_HIP(hipGetLastError());
    }
    RMR_HIP(hipMemcpyAsync(&took, cursor, 8, hipMemcpyDeviceToHost, e->stream));
    RMR_HIP(hipStreamSynchronize(e->stream));
    if ((int64_t)took > capacity - list_len)
        RMR_FAIL(RMR_ERR_INVALID, "rmr_site_medians: the range reports %lld sites, the lists have room for %lld", (long long)took,
                 (long long)(capacity - list_len));
    if (took) {
        ProfScope ps(e, K_SITE_KMER_LEVELS);
        const int64_t blocks = std::min<int64_t>(((int64_t)took + T - 1) / T, KMER_COUNT_BLOCKS);
        hipLaunchKernelGGL(kmer_count_kernel, dim3((unsigned)blocks), dim3(T), 0, e->stream, list_kmer + list_len, (int64_t)took, n_kmers,
                           (unsigned long long *)site_counts);
        RMR_HIP(hipGetLastError());
    }
    *n_appended = (int64_t)took;
    RMR_HIP(hipStreamSynchronize(e->stream));  // the temporaries are freed on return
    return 0;
}

static void kmer_letters(int64_t m, int k, char *out) {
    for (int j = k - 1; j >= 0; --j, m >>= 2) out[j] = "ACGT"[m & 3];
    out[k] = 0;
}

// Stage 2: the lists of every range -> the table, group by group of consecutive k-mers whose sites fit `max_bytes` of sort buffers
int run_kmer_levels_from_sites(rmr_engine *e, int64_t n_sites, const int32_t *list_kmer, const double *list_level, int k, const int64_t *site_counts,
                               int64_t max_bytes, double *levels, int64_t *kmer_sites, int32_t *site_kmer, double *site_level, int64_t *n_groups) {
    const int64_t n_kmers = (int64_t)1 << (2 * k), BYTES_PER_SITE = 32;
    const unsigned T = 256;
    std::vector<int64_t> h((size_t)n_kmers);
    RMR_HIP(hipMemcpyAsync(h.data(), site_counts, n_kmers * 8, hipMemcpyDeviceToHost, e->stream));
    RMR_HIP(hipStreamSynchronize(e->stream));
    int64_t total = 0;
    for (int64_t c : h) {
        if (c < 0 || c > n_sites) RMR_FAIL(RMR_ERR_INVALID, "rmr_kmer_levels_from_sites: a site count of %lld among %lld sites", (long long)c, (long long)n_sites);
        total += c;
    }
    if (total != n_sites)
        RMR_FAIL(RMR_ERR_INVALID, "rmr_kmer_levels_from_sites: the counts hold %lld sites, the lists %lld", (long long)total, (long long)n_sites);
    const int64_t room = max_bytes > 0 ? max_bytes / BYTES_PER_SITE : n_sites;
    std::vector<int64_t> cut{0};  // k-mers [cut[g], cut[g + 1]) are sorted together
    int64_t most = 0;
    for (int64_t m0 = 0; m0 < n_kmers;) {
        int64_t m1 = m0, g = 0;
        while (m1 < n_kmers && g + h[m1] <= room) g += h[m1++];
        if (m1 == m0) {
            char name[RMR_MAX_LEVEL_KMER + 1];
            kmer_letters(m0, k, name);
            RMR_FAIL(RMR_ERR_INVALID, "k-mer levels: the %lld sites of k-mer %s (index %lld) need %lld bytes of sort buffers, the budget is %lld",
                     (long long)h[m0], name, (long long)m0, (long long)(h[m0] * BYTES_PER_SITE), (long long)max_bytes);
        }
        most = std::max(most, g);
        cut.push_back(m1);
        m0 = m1;
    }
    if (n_groups) *n_groups = (int64_t)cut.size() - 1;
    SortBufs s;
    DevFree pool;
    unsigned long long *cursor = nullptr;
    if (most > 0) RMR_TRY(s.get(e, pool, most));
    RMR_TRY(pool.get((void **)&cursor, 8));
    int64_t base = 0;
    for (size_t gi = 0; gi + 1 < cut.size(); ++gi) {
        const int64_t m0 = cut[gi], m1 = cut[gi + 1];
        int64_t g = 0;
        for (int64_t m = m0; m < m1; ++m) g += h[m];
        if (g > 0) {
            unsigned long long took = 0;
            {
                ProfScope ps(e, K_SITE_KMER_LEVELS);
                RMR_HIP(hipMemsetAsync(cursor, 0, 8, e->stream));
                hipLaunchKernelGGL(kmer_group_gather_kernel, dim3((unsigned)((n_sites + T - 1) / T)), dim3(T), 0, e->stream, list_kmer, list_level, n_sites,
                                   m0, m1, cursor, g, s.A, s.C);
                RMR_HIP(hipGetLastError());
            }
            RMR_HIP(hipMemcpyAsync(&took, cursor, 8, hipMemcpyDeviceToHost, e->stream));
            RMR_HIP(hipStreamSynchronize(e->stream));
            if ((int64_t)took != g)
                RMR_FAIL(RMR_ERR_INVALID, "rmr_kmer_levels_from_sites: the lists hold %lld sites of k-mers %lld..%lld, the counts %lld", (long long)took,
                         (long long)m0, (long long)m1 - 1, (long long)g);
        }
        ProfScope ps(e, K_SITE_KMER_LEVELS);
        if (g > 0) {
            // A: k-mers, C: keys of the medians.  By median (C keys, A payload -> B, D), then by k-mer (D keys, B payload -> A, C)
            RMR_TRY(sort_pairs(e, s.tmp, s.tmp_bytes, s.C, s.B, s.A, s.D, g));
            RMR_TRY(sort_pairs(e, s.tmp, s.tmp_bytes, s.D, s.A, s.B, s.C, g, (unsigned)(2 * k)));
        }
        hipLaunchKernelGGL(kmer_median_kernel, dim3((unsigned)((m1 - m0 + T - 1) / T)), dim3(T), 0, e->stream, s.A, s.C, g, m0, m1, levels, kmer_sites);
        if (site_kmer && g > 0)
            hipLaunchKernelGGL(site_list_kernel, dim3((unsigned)((g + T - 1) / T)), dim3(T), 0, e->stream, s.A, s.C, g, site_kmer + base, site_level + base);
        RMR_HIP(hipGetLastError());
        base += g;
    }
    RMR_HIP(hipStreamSynchronize(e->stream));  // the temporaries are freed on return
    return 0;
}

}  // namespace rmr

using namespace rmr;

extern "C" {

int rmr_base_metrics(rmr_engine *e, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off, const int64_t *seq_to_sig,
                     const int64_t *seq_off, const double *shift, const double *scale, int64_t max_read_bases, int start_trim,
                     int end_trim, float *dwell, double *mean, double *sd, double *trimmean, double *trimsd) {
    if (!e || !dacs || !sig_off || !seq_to_sig || !seq_off || !shift || !scale) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > 0x7fffffffLL) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads");
    if (max_read_bases < 0) RMR_FAIL(RMR_ERR_INVALID, "bad max_read_bases");
    if (start_trim < 0 || end_trim < 0) RMR_FAIL(RMR_ERR_INVALID, "trims must not be negative");
    if (n_reads == 0 || max_read_bases == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    BaseMetricsArgs a{dacs, sig_off, seq_to_sig, seq_off, shift, scale, dwell, mean, sd, trimmean, trimsd, start_trim, end_trim};
    return launch_base_metrics(e, n_reads, max_read_bases, a);
}

int rmr_region_base_metrics(rmr_engine *e, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off, const int64_t *seq_to_sig,
                            const int64_t *seq_off, const double *shift, const double *scale, int64_t n_pairs, const int64_t *pairs,
                            int64_t max_pair_bases, int start_trim, int end_trim, int64_t rows, int64_t width, double *dwell, double *mean,
                            double *sd, double *trimmean, double *trimsd, int32_t *status) {
    if (!e || !dacs || !sig_off || !seq_to_sig || !seq_off || !shift || !scale) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > 0x7fffffffLL || n_pairs < 0 || n_pairs > 0x7fffffffLL) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads / n_pairs");
    if (start_trim < 0 || end_trim < 0) RMR_FAIL(RMR_ERR_INVALID, "trims must not be negative");
    if (n_pairs == 0) return 0;
    if (!pairs || !status || n_reads == 0) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (rows <= 0 || width <= 0 || max_pair_bases <= 0) RMR_FAIL(RMR_ERR_INVALID, "bad rows / width / max_pair_bases");
    // a span of n bases touches at most (n + 62) / 64 + 1 groups of 64 counted from the read's first base
    const int64_t groups = (max_pair_bases + 62) / 64 + 1, gy = (groups + BM_WAVES - 1) / BM_WAVES;
    if (gy > 65535) RMR_FAIL(RMR_ERR_INVALID, "rmr_region_base_metrics: a region of %lld bases is beyond the launch grid", (long long)max_pair_bases);
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    RegionMetricsArgs a{dacs, sig_off, seq_to_sig, seq_off, shift, scale, pairs, n_reads, rows, width, dwell, mean, sd, trimmean, trimsd, status,
                        start_trim, end_trim};
    ProfScope ps(e, K_REGION_METRICS);
    hipLaunchKernelGGL(region_metrics_kernel, dim3((unsigned)n_pairs, (unsigned)gy), dim3(64 * BM_WAVES), 0, e->stream, a);
    RMR_HIP(hipGetLastError());
    return 0;
}

int rmr_region_signals(rmr_engine *e, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off, const int64_t *seq_to_sig,
                       const int64_t *seq_off, const double *shift, const double *scale, int64_t n_pairs, const int64_t *pairs,
                       const int64_t *sig_out_off, const int64_t *map_out_off, int raw, void *sig_out, int64_t sig_capacity, int64_t *map_out,
                       int64_t map_capacity, int64_t *sig_start, int32_t *status) {
    if (!e || !dacs || !sig_off || !seq_to_sig || !seq_off || !shift || !scale) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > 0x7fffffffLL || n_pairs < 0 || n_pairs > 0x7fffffffLL) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads / n_pairs");
    if (n_pairs == 0) return 0;
    if (!pairs || !sig_out_off || !map_out_off || !sig_out || !map_out || !sig_start || !status || n_reads == 0)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (sig_capacity < 0 || map_capacity < 0) RMR_FAIL(RMR_ERR_INVALID, "bad capacity");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    RegionSignalsArgs a{dacs, sig_off, seq_to_sig, seq_off, shift, scale, pairs, sig_out_off, map_out_off, n_reads, sig_capacity, map_capacity,
                        sig_out, map_out, sig_start, status};
    ProfScope ps(e, K_REGION_SIGNALS);
    const dim3 grid((unsigned)n_pairs, 8), block(256);
    if (raw) hipLaunchKernelGGL(region_signals_kernel<true>, grid, block, 0, e->stream, a);
    else hipLaunchKernelGGL(region_signals_kernel<false>, grid, block, 0, e->stream, a);
    RMR_HIP(hipGetLastError());
    return 0;
}

int rmr_site_kmer_levels(rmr_engine *e, int64_t n_reads, const int64_t *seq_off, const int64_t *site0, int64_t n_bases,
                         const double *trimmean, const int8_t *int_seq, int kmer_before, int kmer_after, int64_t min_cov,
                         double *levels, int64_t *kmer_sites, int32_t *site_kmer, double *site_level, int64_t *n_sites) {
    if (!e || !levels) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (kmer_before < 0 || kmer_after < 0 || kmer_before + kmer_after + 1 > RMR_MAX_LEVEL_KMER)
        RMR_FAIL(RMR_ERR_INVALID, "k-mers of 1 to %d bases are supported, got %d + 1 + %d", RMR_MAX_LEVEL_KMER, kmer_before, kmer_after);
    if (n_reads < 0 || n_bases < 0 || n_bases > 0x7fffffffLL * 256) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads / n_bases");
    if (n_bases > 0 && (!seq_off || !site0 || !trimmean || !int_seq || n_reads == 0)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if ((site_kmer == nullptr) != (site_level == nullptr)) RMR_FAIL(RMR_ERR_INVALID, "site_kmer and site_level go together");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return run_site_kmer_levels(e, n_reads, seq_off, site0, n_bases, trimmean, int_seq, kmer_before, kmer_after, min_cov, levels, kmer_sites,
                                site_kmer, site_level, n_sites);
}

int rmr_site_medians(rmr_engine *e, int64_t n_reads, const int64_t *seq_off, const int64_t *site0, int64_t n_bases, const double *trimmean,
                     const int8_t *int_seq, int kmer_before, int kmer_after, int64_t min_cov, int64_t key_lo, int64_t key_hi,
                     int32_t *list_kmer, double *list_level, int64_t list_len, int64_t list_capacity, int64_t *site_counts,
                     int64_t *n_appended) {
    if (!e || !site_counts || !n_appended) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (kmer_before < 0 || kmer_after < 0 || kmer_before + kmer_after + 1 > RMR_MAX_LEVEL_KMER)
        RMR_FAIL(RMR_ERR_INVALID, "k-mers of 1 to %d bases are supported, got %d + 1 + %d", RMR_MAX_LEVEL_KMER, kmer_before, kmer_after);
    if (n_reads < 0 || n_bases < 0 || n_bases > 0x7fffffffLL * 256) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads / n_bases");
    if (n_bases > 0 && (!seq_off || !site0 || !trimmean || !int_seq || n_reads == 0)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (key_lo < 0 || key_hi < key_lo) RMR_FAIL(RMR_ERR_INVALID, "bad key range [%lld, %lld)", (long long)key_lo, (long long)key_hi);
    if (list_len < 0 || list_capacity < list_len) RMR_FAIL(RMR_ERR_INVALID, "bad list_len / list_capacity");
    if (list_capacity > list_len && (!list_kmer || !list_level)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return run_site_medians(e, n_reads, seq_off, site0, n_bases, trimmean, int_seq, kmer_before, kmer_after, min_cov, (uint64_t)key_lo,
                            (uint64_t)key_hi, list_kmer, list_level, list_len, list_capacity, site_counts, n_appended);
}

int rmr_kmer_levels_from_sites(rmr_engine *e, int64_t n_sites, const int32_t *list_kmer, const double *list_level, int kmer_len,
                               const int64_t *site_counts, int64_t max_bytes, double *levels, int64_t *kmer_sites, int32_t *site_kmer,
                               double *site_level, int64_t *n_groups) {
    if (!e || !levels || !site_counts) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (kmer_len < 1 || kmer_len > RMR_MAX_LEVEL_KMER) RMR_FAIL(RMR_ERR_INVALID, "k-mers of 1 to %d bases are supported, got %d", RMR_MAX_LEVEL_KMER, kmer_len);
    if (n_sites < 0 || n_sites > 0x7fffffffLL * 256 || max_bytes < 0) RMR_FAIL(RMR_ERR_INVALID, "bad n_sites / max_bytes");
    if (n_sites > 0 && (!list_kmer || !list_level)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if ((site_kmer == nullptr) != (site_level == nullptr)) RMR_FAIL(RMR_ERR_INVALID, "site_kmer and site_level go together");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return run_kmer_levels_from_sites(e, n_sites, list_kmer, list_level, kmer_len, site_counts, max_bytes, levels, kmer_sites, site_kmer, site_level,
                                      n_groups);
}

}  // extern "C"
