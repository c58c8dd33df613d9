// k_ref_genome.hip — the reference genome of `analyze pileup_modbams --ref` resident on the device (rmr_ref_genome_*), in the
// form the emit's motif test reads (rmr_modbam_walk.h, ref_code): one nibble per base, two bases per byte, low nibble first,
// every contig from a byte boundary.  A code is the IUPAC set of its letter as a mask - A 1, C 2, G 4, T / U 8, an ambiguity
// letter the union of its bases, N 15; lower case as upper case; 0 is no letter - so the complement of a code is its four
// bits reversed, and "everything the reference allows, the motif allows" is (r & ~m) == 0.
//
//   pack    one launch per piece of a contig's FASTA text (the sequence lines as they stand in the file, terminators
//           included).  The thread of output byte t reads bases 2t and 2t + 1 at (i / line_bases) * line_width + i % line_bases,
//           codes them and writes one byte: no atomics on the data.  The same threads check what the host never looked at:
//           a base byte that is no IUPAC letter, or a byte in a terminator column (behind the last base of a line) that is
//           not the terminator, puts its byte offset into one word by an integer atomicMin - the first violation, whatever
//           the order of the threads and the pieces.
//   unpack  codes [lo, hi) of a contig, one per byte (rmr_ref_genome_read: for the tests).
//   emit    the pileup's walk (rmr_modbam_walk.h, REF = true) with the motif test and the strand fold.  These kernels stand
//           here and not beside k_pileup.hip's: that file then compiles, instruction for instruction, the emit it compiled
//           before there was a reference (a second pair of callers in one translation unit changed how the walk's helpers
//           were inlined into the first: 1924 instead of 1884 instructions in the count pass, profiles/NOTES_r18.md).
#include "rmr_internal.h"
#include "rmr_modbam_walk.h"
#include "rmr_ref_pack.h"

using namespace rmr;

namespace {

constexpr unsigned RG_THREADS = 256;

// text: the piece's bytes, text[0] = byte text_lo of the contig's span of span_bytes bytes; it holds bases [base_lo, base_hi),
// base_lo even; out: the contig's packed bytes from base base_lo on.  The thread's work is rmr_ref_pack.h's ref_pack_pair.
__global__ __launch_bounds__(RG_THREADS) void pack_kernel(const uint8_t *__restrict__ text, int64_t text_lo, int64_t text_bytes, int64_t span_bytes,
                                                           int64_t base_lo, int64_t base_hi, int64_t line_bases, int64_t line_width,
                                                           uint8_t *__restrict__ out, unsigned long long *__restrict__ first_bad) {
    const int64_t t = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    const int64_t i0 = base_lo + 2 * t;
    if (i0 >= base_hi) return;
    unsigned long long bad;
    out[t] = (uint8_t)ref_pack_pair(text, text_lo, text_bytes, span_bytes, i0, base_hi, line_bases, line_width, &bad);
    if (bad != ~0ull) atomicMin(first_bad, bad);
}

__global__ __launch_bounds__(RG_THREADS) void unpack_kernel(const uint8_t *__restrict__ data, int64_t off, int64_t len, int64_t lo, int64_t hi,
                                                             uint8_t *__restrict__ codes) {
    const int64_t i = lo + (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (i < hi) codes[i - lo] = (uint8_t)ref_code(data, off, len, i);
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)((n + RG_THREADS - 1) / RG_THREADS)); }

// k_pileup.hip's modbam_call_kernel with a reference: the motifs travel by value in the kernel arguments
template <bool FILL>
__global__ __launch_bounds__(MB_THREADS) void modbam_call_ref_kernel(rmr_modbam_batch b, PileupEmit pe, PileupRef pr, int32_t *__restrict__ ords,
                                                                      int64_t *__restrict__ cig_q, int64_t *__restrict__ cig_r,
                                                                      int64_t *__restrict__ counts, int32_t *__restrict__ status,
                                                                      const int64_t *__restrict__ out_off) {
    __shared__ unsigned s_hist[FILL ? 1 : PILEUP_BINS];
    modbam_walk<FILL, true, true>(b, ords, cig_q, cig_r, counts, status, out_off, nullptr, nullptr, nullptr, nullptr, pe, s_hist, pr);
}

}  // namespace

namespace rmr {

int launch_ref_pack(rmr_engine *e, const uint8_t *text, int64_t text_lo, int64_t text_bytes, int64_t span_bytes, int64_t base_lo, int64_t base_hi,
                    int64_t line_bases, int64_t line_width, uint8_t *out, unsigned long long *first_bad) {
    const int64_t n_out = (base_hi - base_lo + 1) / 2;
    if (n_out <= 0) return 0;
    ProfScope ps(e, K_REF_GENOME_PACK);
    hipLaunchKernelGGL(pack_kernel, grid_of(n_out), dim3(RG_THREADS), 0, e->stream, text, text_lo, text_bytes, span_bytes, base_lo, base_hi,
                       line_bases, line_width, out, first_bad);
    RMR_HIP(hipGetLastError());
    return 0;
}

int launch_modbam_calls_ref(rmr_engine *e, const rmr_modbam_batch &b, const PileupEmit &pe, const PileupRef &pr, int32_t *ords, int64_t *cig_q,
                            int64_t *cig_r, int64_t *counts, int32_t *status, const int64_t *out_off) {
    if (b.n_records <= 0) return 0;
    ProfScope ps(e, K_PILEUP_EMIT);
    const dim3 grid((unsigned)b.n_records), block(MB_THREADS);
    if (out_off)
        hipLaunchKernelGGL(modbam_call_ref_kernel<true>, grid, block, 0, e->stream, b, pe, pr, ords, cig_q, cig_r, counts, status, out_off);
    else
        hipLaunchKernelGGL(modbam_call_ref_kernel<false>, grid, block, 0, e->stream, b, pe, pr, ords, cig_q, cig_r, counts, status, out_off);
    RMR_HIP(hipGetLastError());
    return 0;
}

int launch_ref_unpack(rmr_engine *e, const rmr_ref_genome *g, int64_t contig, int64_t lo, int64_t hi, uint8_t *codes) {
    if (hi <= lo) return 0;
    hipLaunchKernelGGL(unpack_kernel, grid_of(hi - lo), dim3(RG_THREADS), 0, e->stream, g->data, g->h_off[contig], g->h_len[contig], lo, hi, codes);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
