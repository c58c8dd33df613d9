// k_pileup_duplex.hip — `analyze pileup_modbams --duplex / --hemi`: the emit that counts the '-'-strand MM entries of duplex
// records, and the pairing of the two strands' calls of one record at one motif site.
//
//   emit    k_pileup.hip's modbam_call_kernel / k_ref_genome.hip's modbam_call_ref_kernel with the DUPLEX flag of the walk
//           (rmr_modbam_walk.h): an entry of strand '-' counts, its call lies on the reference strand opposite to the record's.
//           Kernels of their own: the four emit kernels without the flag keep their code and their argument blocks.
//           Hemi mode of the fill (pr.combine == 2): a '-' call is written at the '+' position of its motif window and keeps
//           its strand bit - the two calls of one site of one record then differ in the strand bit alone (and the code).
//   pair    one block per record over its slice of the filled words, two passes (count, the caller's prefix sum, fill).  The
//           words of a record stand in walk order, so their reference positions are monotone and the '-' word of a '+' word's
//           site lies at most RMR_PILEUP_MAX_MOTIF_LEN - 1 words away, on either side; it is the first word of that window, in
//           index order, with an equal word >> 5 and strand bit 1.  The search never leaves the record's slice: calls of
//           different records are never paired.  A pair word is the '+' word with the code a n_codes + b (a, b: the classes
//           of the '+' and of the '-' call), written in the order of the '+' words (block prefix count, as the walk's).
// Plain loads and stores; every index is bounded by n_words and by the record's slice.
#include "rmr_modbam_walk.h"

using namespace rmr;

namespace {

template <bool FILL, bool REF>
__global__ __launch_bounds__(MB_THREADS) void modbam_call_duplex_kernel(rmr_modbam_batch b, PileupEmit pe, PileupRef pr, int32_t *__restrict__ ords,
                                                                         int64_t *__restrict__ cig_q, int64_t *__restrict__ cig_r,
                                                                         int64_t *__restrict__ counts, int32_t *__restrict__ status,
                                                                         const int64_t *__restrict__ out_off) {
    __shared__ unsigned s_hist[FILL ? 1 : PILEUP_BINS];
    modbam_walk<FILL, true, REF, true>(b, ords, cig_q, cig_r, counts, status, out_off, nullptr, nullptr, nullptr, nullptr, pe, s_hist, pr);
}

constexpr int PAIR_THREADS = 256, PAIR_WAVES = PAIR_THREADS / 64;
constexpr int64_t PAIR_REACH = RMR_PILEUP_MAX_MOTIF_LEN - 1;  // words between a '+' word and its partner, at the most

// FILL: pair_words[pair_off[r] ..) gets the record's pair words (nothing at or behind pair_off[r + 1]); else pairs[r] = their number
template <bool FILL>
__global__ __launch_bounds__(PAIR_THREADS) void pair_kernel(const int64_t *__restrict__ out_off, const uint64_t *__restrict__ words, int64_t n_words,
                                                             int n_codes, int64_t *__restrict__ pairs, const int64_t *__restrict__ pair_off,
                                                             uint64_t *__restrict__ pair_words) {
    __shared__ int s_emit[2][PAIR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    const int64_t lo = out_off[r] > 0 ? out_off[r] : 0, hi = out_off[r + 1] < n_words ? out_off[r + 1] : n_words;
    const int64_t p_lo = FILL ? pair_off[r] : 0, p_hi = FILL ? pair_off[r + 1] : 0;
    if (FILL && p_hi <= p_lo) return;  // (uniform over the block)
    const unsigned long long lt = (1ull << lane) - 1ull;
    int64_t emitted = 0;
    int par = 0;
    for (int64_t i0 = lo; i0 < hi; i0 += PAIR_THREADS, par ^= 1) {
        const int64_t i = i0 + tid;
        bool paired = false;
        uint64_t w = 0, x = 0;
        if (i < hi) {
            w = words[i];
            if (((w >> 4) & 1u) == 0) {
                const int64_t j_lo = i - PAIR_REACH > lo ? i - PAIR_REACH : lo, j_hi = i + PAIR_REACH + 1 < hi ? i + PAIR_REACH + 1 : hi;
                for (int64_t j = j_lo; j < j_hi && !paired; ++j) {
                    x = words[j];
                    paired = (x >> 5) == (w >> 5) && ((x >> 4) & 1u) != 0;
                }
            }
        }
        const unsigned long long km = __ballot(paired);
        if (lane == 0) s_emit[par][wave] = __popcll(km);
        __syncthreads();  // (the other half of s_emit is written next round: nobody still reads it, every thread has passed this barrier)
        int before = 0, tot = 0;
#pragma unroll
        for (int v = 0; v < PAIR_WAVES; ++v) {
            if (v < wave) before += s_emit[par][v];
            tot += s_emit[par][v];
        }
        if (FILL && paired) {
            const int64_t o = p_lo + emitted + before + __popcll(km & lt);
            if (o >= 0 && o >= p_lo && o < p_hi) {  // (offsets that are not this batch's counts write nothing outside the record's slice)
                int a = (int)(w & 15u), c = (int)(x & 15u);  // (a code the alphabet does not have: `fail`)
                a = a < n_codes ? a : n_codes - 1, c = c < n_codes ? c : n_codes - 1;
                pair_words[o] = (w & ~(uint64_t)31) | (uint64_t)(a * n_codes + c);
            }
        }
        emitted += tot;
    }
    if (!FILL && tid == 0) pairs[r] = emitted;
}

}  // namespace

namespace rmr {

int launch_modbam_calls_duplex(rmr_engine *e, const rmr_modbam_batch &b, const PileupEmit &pe, const PileupRef &pr, bool has_ref, int32_t *ords,
                               int64_t *cig_q, int64_t *cig_r, int64_t *counts, int32_t *status, const int64_t *out_off) {
    if (b.n_records <= 0) return 0;
    ProfScope ps(e, K_PILEUP_EMIT);
    const dim3 grid((unsigned)b.n_records), block(MB_THREADS);
    if (out_off && has_ref)
        hipLaunchKernelGGL((modbam_call_duplex_kernel<true, true>), grid, block, 0, e->stream, b, pe, pr, ords, cig_q, cig_r, counts, status, out_off);
    else if (out_off)
        hipLaunchKernelGGL((modbam_call_duplex_kernel<true, false>), grid, block, 0, e->stream, b, pe, pr, ords, cig_q, cig_r, counts, status, out_off);
    else if (has_ref)
        hipLaunchKernelGGL((modbam_call_duplex_kernel<false, true>), grid, block, 0, e->stream, b, pe, pr, ords, cig_q, cig_r, counts, status, out_off);
    else
        hipLaunchKernelGGL((modbam_call_duplex_kernel<false, false>), grid, block, 0, e->stream, b, pe, pr, ords, cig_q, cig_r, counts, status, out_off);
    RMR_HIP(hipGetLastError());
    return 0;
}

// the count pass (pair_words == nullptr: pairs[r]) or the fill pass
int launch_pileup_pairs(rmr_engine *e, int64_t n_records, const int64_t *out_off, const uint64_t *words, int64_t n_words, int n_codes,
                        int64_t *pairs, const int64_t *pair_off, uint64_t *pair_words) {
    if (n_records <= 0) return 0;
    ProfScope ps(e, K_PILEUP_PAIR);
    const dim3 grid((unsigned)n_records), block(PAIR_THREADS);
    if (pair_words)
        hipLaunchKernelGGL(pair_kernel<true>, grid, block, 0, e->stream, out_off, words, n_words, n_codes, pairs, pair_off, pair_words);
    else
        hipLaunchKernelGGL(pair_kernel<false>, grid, block, 0, e->stream, out_off, words, n_words, n_codes, pairs, pair_off, pair_words);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
