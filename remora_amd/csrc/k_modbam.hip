// k_modbam.hip — the site join of `validate from_modbams`: the modified-base calls of a batch of BAM records (the tokenised
// MM / ML tags, mod_tags.cpp) laid along the reads' bases, carried through the CIGARs to reference positions and looked up in
// the ground-truth table.  Replaces validate.check_mod_strand + validate.parse_mod_read (src/remora/validate.py:296-446): a
// Python loop over pysam's get_aligned_pairs(with_seq=True) with a dictionary lookup per aligned pair, on top of htslib's
// walk along the bases inside AlignedSegment.modified_bases.
//
// The walk itself is rmr_modbam_walk.h's (shared with the pileup, k_pileup.hip); this file is its truth-join instantiation.
#include "rmr_modbam_walk.h"

using namespace rmr;

namespace {

template <bool FILL>
__global__ __launch_bounds__(MB_THREADS) void modbam_site_kernel(rmr_modbam_batch b, int32_t *__restrict__ ords, int64_t *__restrict__ cig_q,
                                                                  int64_t *__restrict__ cig_r, int64_t *__restrict__ counts,
                                                                  int32_t *__restrict__ status, const int64_t *__restrict__ out_off,
                                                                  float *__restrict__ probs, uint8_t *__restrict__ label,
                                                                  int64_t *__restrict__ qpos, int64_t *__restrict__ rpos) {
    modbam_walk<FILL, false>(b, ords, cig_q, cig_r, counts, status, out_off, probs, label, qpos, rpos, PileupEmit{}, nullptr);
}

}  // namespace

namespace rmr {

int launch_modbam_sites(rmr_engine *e, const rmr_modbam_batch &b, int32_t *ords, int64_t *cig_q, int64_t *cig_r, int64_t *counts,
                        int32_t *status, const int64_t *out_off, float *probs, uint8_t *label, int64_t *qpos, int64_t *rpos) {
    if (b.n_records <= 0) return 0;
    ProfScope ps(e, K_MODBAM_SITES);
    if (out_off)
        hipLaunchKernelGGL(modbam_site_kernel<true>, dim3((unsigned)b.n_records), dim3(MB_THREADS), 0, e->stream, b, ords, cig_q, cig_r, counts,
                           status, out_off, probs, label, qpos, rpos);
    else
        hipLaunchKernelGGL(modbam_site_kernel<false>, dim3((unsigned)b.n_records), dim3(MB_THREADS), 0, e->stream, b, ords, cig_q, cig_r, counts,
                           status, out_off, probs, label, qpos, rpos);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
