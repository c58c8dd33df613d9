// Internal declarations shared by the translation units of libremora_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/remora_hip.h"
#include "rmr_pack.h"

namespace rmr {

// ---- error plumbing (set_error, RMR_FAIL, RMR_TRY: rmr_pack.h) ----------------------------
#define RMR_HIP(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            ::rmr::set_error("HIP error %s at %s:%d (%s)", hipGetErrorString(_e), __FILE__, \
                             __LINE__, #expr);                                            \
            return RMR_ERR_HIP;                                                           \
        }                                                                                 \
    } while (0)

// ---- kernel ids for the profiling table ------------------------------------------------
enum KernelId {
    K_ENCODE = 0,
    K_TRIM,
    K_MOVES,
    K_NORMALISE,
    K_GEOMETRY,
    K_FILL,
    K_FRONT_SIG,
    K_FRONT_SEQ,
    K_SEQ1_DENSE,
    K_CONV_SIG3,
    K_CONV_SEQ2,
    K_CONV_SEQ3,
    K_CONV_MERGE1,
    K_CONV_MERGE2,
    K_CONV_MERGE3,
    K_CONV_MERGE4,
    K_LSTM_HEAD,
    K_FC_HEAD,
    K_COUNT,
    K_MOTIF,
    K_VBZ,
    K_REFINE_BAND,
    K_REFINE_DP,
    K_REFINE_ROWWISE,
    K_FUSED_FRONT,
    K_RESCALE_Q,
    K_SIG3_FRONT,
    K_SEQ2_FRONT,
    K_PROBE_DIFF,
    K_PROBE_NONFINITE,
    K_WINO_FORM,  // a launch count without a time: every kernel launched in a Winograd form is ALSO counted here (its time stays under its layer's id)
    K_BASE_METRICS,
    K_REGION_METRICS,
    K_REGION_SIGNALS,
    K_SITE_KMER_LEVELS,  // its kernels and the four radix sorts between them, bracketed in two pieces
    K_MODBAM_SITES,
    K_RESCALE_POINTS,
    K_THEIL_SEN,
    K_DUPLEX_DP,
    K_DUPLEX_TRACE,
    K_DUPLEX_LINES,      // the forward pass that keeps one line per strip instead of the trace
    K_DUPLEX_BACKTRACK,  // the walk back that recomputes the trace one strip at a time
    // the training step (k_train.hip)
    K_TRAIN_GEMM,    // forward, data-gradient and LSTM products on the fp32 matrix cores
    K_TRAIN_WGRAD,   // weight-gradient products (per-slice partials)
    K_TRAIN_REDUCE,  // the fixed-order second passes of the weight gradients and column sums
    K_TRAIN_BN,      // BatchNorm column sums, normalise + swish, backward apply
    K_TRAIN_LSTM,    // the LSTM steps (recurrent product + cell), forward and backward
    K_TRAIN_LOSS,    // fc, cross-entropy and its gradient
    K_TRAIN_ADAMW,   // the optimiser and max |grad|
    K_TRAIN_AUX,     // weight repacks, sig_conv1, the k-mer transpose, fills
    // the read-id index of a POD5 dataset (k_read_index.hip)
    K_READ_INDEX_BUILD,   // its kernels, the two radix sorts and the scan between them, bracketed in two pieces
    K_READ_INDEX_LOOKUP,
    // `analyze pileup_modbams` (k_pileup.hip)
    K_PILEUP_EMIT,   // the walk that writes site words (or the confidence histogram)
    K_PILEUP_FLUSH,  // one flush: the radix sort, the run counts and the merge into the table
    K_REF_GENOME_PACK,  // one piece of a contig's FASTA text into nibbles, verified (k_ref_genome.hip)
    K_PILEUP_STAMP,  // the partition id into the words of a batch (k_pileup.hip)
    K_PILEUP_PAIR,   // the two strands' calls of a record paired into pattern words (k_pileup_duplex.hip)
    K_PILEUP_COVER,  // the coverage join: every record against the sites of the resident table it spans (k_pileup.hip)
    K_NUM
};
const char *kernel_name(int id);

}  // namespace rmr

// ---- engine ------------------------------------------------------------------------------
struct rmr_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    hipStream_t aux = nullptr;  // upload stream of rmr_infer_chunks (the pinned slots and ev_h2d below)
    hipEvent_t ev_handoff = nullptr;  // rmr_engine_wait_for: recorded on this engine's stream, waited for by another's
    int num_cus = 256;
    std::mutex mu;
    int64_t subbatch = 0;
    // RCCL communicator of rmr_comm_init (opaque ncclComm_t), this rank and the job size
    void *comm = nullptr;
    int comm_rank = 0, comm_world = 1;

    // grow-only device scratch arenas
    struct Arena {
        void *ptr = nullptr;
        size_t cap = 0;
    };
    Arena act;      // activations of the fused pipeline
    Arena staging;  // host<->device staging for RMR_MEM_HOST calls
    int ensure(Arena &a, size_t bytes);
    // pinned host bounce buffers (two slots) + copy-done events: large RMR_MEM_HOST batches are uploaded
    // sub-batch by sub-batch on the aux stream under the kernels of the previous sub-batch
    void *pinned = nullptr;
    size_t pinned_cap = 0;
    hipEvent_t ev_h2d[2] = {nullptr, nullptr};
    int ensure_pinned(size_t bytes);
    // pinned staging of rmr_call_read (one read in, its logits out): its own small buffer, so that a single-read call
    // never re-allocates the two big slots above under an upload
    void *pin_call = nullptr;
    size_t pin_call_cap = 0;
    int ensure_pin_call(size_t bytes);

    // kernels whose dynamic-LDS limit was raised ON THIS DEVICE (hipFuncSetAttribute is per device: a flag per
    // process would skip the second engine of a multi-GPU process); guarded by `mu` like every launch
    std::vector<const void *> lds_attr_set;
    int allow_big_lds(const void *kernel, size_t bytes = 160 * 1024);  // `bytes`: the dynamic share (a kernel with static LDS asks for less)
    // numRegs of a kernel (256 where it cannot be read), the input of its launch plan (rmr_plan.h); guarded by `mu` as well
    std::vector<std::pair<const void *, int>> regs_seen;
    int kernel_regs(const void *kernel);

    // profiling
    bool profiling = false;
    struct Rec {
        int id;
        hipEvent_t t0, t1;
    };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    double acc_ms[rmr::K_NUM] = {};
    int64_t acc_n[rmr::K_NUM] = {};
    int prof_begin(int id, hipEvent_t *t1, hipStream_t s);
    void prof_count(int id) { if (profiling) acc_n[id] += 1; }  // a launch counted beside its timed record (K_WINO_FORM)
    int prof_collect();
};

namespace rmr {
void rccl_comm_free(void *comm);  // comm.cpp: rmr_engine_destroy drops the communicator of rmr_comm_init through it
// Diagnostics (RMR_POISON=1): in front of EVERY kernel launch of the library a kernel fills the LDS and most of the vector
// registers of every CU with 0xFFFFFFFF (NaN as fp32 / bf16 / half, -1 as an integer).  LDS and registers keep what the
// previous workgroup left; a kernel that reads a word it never wrote normally finds the leftovers of its own kind (often
// the very values it would have written) and only fails next to OTHER kernels - e.g. another process's on the same GPU.
// With the poison such a read shows up in a single process: tools/poison_check.py.
void poison_before_launch(rmr_engine *e, hipStream_t s);
}  // namespace rmr

// RAII-less helper: brackets one launch with events when profiling is on
struct ProfScope {
    rmr_engine *e;
    hipEvent_t t1 = nullptr;
    bool on = false;
    hipStream_t s;
    ProfScope(rmr_engine *eng, int id, hipStream_t st = nullptr, bool use_st = false)
        : e(eng), s(use_st ? st : eng->stream) {
        rmr::poison_before_launch(e, s);
        if (e->profiling) on = (e->prof_begin(id, &t1, s) == 0);
    }
    ~ProfScope() {
        if (on) (void)hipEventRecord(t1, s);
    }
};

// ---- model -------------------------------------------------------------------------------
// the packed weights and geometry (rmr_pack.h) plus what lives with the device copies
struct rmr_model : rmr::ModelWeights {
    rmr_engine *eng = nullptr;
    int true_size = 0;      // the network's own `size` (model_params["size"]); channels beyond it carry zero weights
    std::vector<void *> dev_allocs;
    // the Winograd guard (include/remora_hip.h, rmr_model_numerics): the decision of the load-time probe.  `use_winograd` is what
    // the forward entries read beside RMR_WINOGRAD; it stays true for a model that is not screened (none of its layers has a
    // Winograd kernel, so nothing reads it), whose record says checked = 0, winograd = 0
    bool use_winograd = true;
    rmr_model_numerics numerics{};
};

// ---- read-id index (k_read_index.hip) ------------------------------------------------------
// the table of rmr_read_index_create: n distinct ids in ascending (hi, lo) order, one device allocation of 24 n bytes
struct rmr_read_index {
    rmr_engine *eng = nullptr;
    int64_t n = 0;
    void *mem = nullptr;
    uint64_t *hi = nullptr, *lo = nullptr;  // an id's bytes 0-7 and 8-15 as big-endian words
    int64_t *val = nullptr;
};

// ---- per-site pileup (k_pileup.hip) --------------------------------------------------------
// the state of rmr_pileup_create: the call buffer with the work arrays of a flush (one allocation, `work`) and the resident
// table of nt distinct sites in ascending key order (one allocation, `t_mem`: keys, then ncol u32 counts per site)
struct rmr_pileup {
    rmr_engine *eng = nullptr;
    int ncol = 0, end_bit = 0;       // columns of a row (classes + fail); the bits of a word in use
    int64_t cap = 0, used = 0;       // words the buffer holds / holds now
    void *work = nullptr;
    size_t work_bytes = 0, tmp_bytes = 0;
    uint64_t *buf[2] = {nullptr, nullptr};  // the call buffer and its sort double
    uint32_t *head = nullptr, *row = nullptr, *counts = nullptr, *miss = nullptr, *miss_rank = nullptr, *miss_src = nullptr;
    uint64_t *keys = nullptr, *miss_keys = nullptr;
    unsigned long long *overflow = nullptr;
    void *tmp = nullptr;             // rocPRIM's scratch
    void *t_mem = nullptr;
    size_t t_bytes = 0;
    uint64_t *t_keys = nullptr;
    uint32_t *t_counts = nullptr;
    int64_t nt = 0, n_calls = 0, n_flushes = 0;
    size_t peak_bytes = 0;
    // the coverage join (rmr_pileup_cover): u32[nt][3] - delete, diff, nocall - beside the table, allocated and zeroed by the
    // first join after a finish and dropped when words are added again
    bool finished = false;           // rmr_pileup_finish has run and no word was added since
    int canonical = 0;               // rmr_pileup_set_canonical: 'A' 'C' 'G' 'T', 0 while unset
    uint32_t *cover = nullptr;
    size_t cover_bytes = 0;
};

// ---- reference genome (k_ref_genome.hip) ---------------------------------------------------
// the state of rmr_ref_genome_create: the contigs' nibbles in one device allocation (`data`: contig c at byte d_off[c], h_len[c]
// bases in ceil(h_len[c] / 2) bytes), the offsets and lengths on both sides, and the word of the pack kernel's first violation
struct rmr_ref_genome {
    rmr_engine *eng = nullptr;
    int64_t n_contigs = 0;
    void *mem = nullptr;
    size_t bytes = 0;               // of `mem`
    uint8_t *data = nullptr;
    int64_t *d_off = nullptr, *d_len = nullptr;
    unsigned long long *first_bad = nullptr;
    std::vector<int64_t> h_off, h_len;
};

// ---- kernel launchers (defined in k_*.hip) ------------------------------------------------
namespace rmr {

// k_ref_genome.hip: one piece of a contig's text (device copy `text` of bytes [text_lo, text_lo + text_bytes) of its span) ->
// the packed bytes of bases [base_lo, base_hi) at `out`;  codes [lo, hi) of a contig, one per byte
int launch_ref_pack(rmr_engine *e, const uint8_t *text, int64_t text_lo, int64_t text_bytes, int64_t span_bytes, int64_t base_lo, int64_t base_hi,
                    int64_t line_bases, int64_t line_width, uint8_t *out, unsigned long long *first_bad);
int launch_ref_unpack(rmr_engine *e, const rmr_ref_genome *g, int64_t contig, int64_t lo, int64_t hi, uint8_t *codes);

// k_pileup.hip: the emit of `analyze pileup_modbams` (count pass: out_off == nullptr) and the pileup's three steps
constexpr int PILEUP_BINS = RMR_PILEUP_BINS;  // 512 x the winning probability of a call: 0 .. 512
// what the pileup's end of the walk (rmr_modbam_walk.h) needs beside the batch; unused by the truth join
struct PileupEmit {
    int32_t region_ref;             // < 0: every contig, every position
    int64_t region_lo, region_hi;   // [lo, hi) on contig region_ref
    int32_t k_t;                    // fill pass: a call whose 512 x winning probability is below it gets the code `fail`
    unsigned long long *hist;       // count pass: u64[PILEUP_BINS], or nullptr
    uint64_t *words;                // fill pass: one word per kept call
};
// The reference part of an emit (rmr_pileup_emit_counts / _fill with opt->ref): the motif test and the fold of rmr_modbam_walk.h.
// It is a kernel argument of its own, by value, and only of the kernels with a reference (k_ref_genome.hip): PileupEmit and
// with it the argument block of the kernels without one stay byte for byte what they were, and so does their code (one
// pointer more in PileupEmit moved the scalar loads and the register allocation of those kernels, profiles/NOTES_r18.md).
struct PileupRef {
    const uint8_t *data;            // the genome's nibbles
    const int64_t *off, *len;       // per contig: its first byte in `data`, its bases (0: not loaded - nothing matches)
    int32_t n_motifs, combine;      // 1 .. RMR_PILEUP_MAX_MOTIFS; combine: a kept '-' call is written on '+' at pos - (L - 1 - 2 focus)
    rmr_pileup_motif motifs[RMR_PILEUP_MAX_MOTIFS];
};
int launch_modbam_calls(rmr_engine *e, const rmr_modbam_batch &b, const PileupEmit &pe, int32_t *ords, int64_t *cig_q, int64_t *cig_r,
                        int64_t *counts, int32_t *status, const int64_t *out_off);
// k_ref_genome.hip: the same emit with the reference part
int launch_modbam_calls_ref(rmr_engine *e, const rmr_modbam_batch &b, const PileupEmit &pe, const PileupRef &pr, int32_t *ords, int64_t *cig_q,
                            int64_t *cig_r, int64_t *counts, int32_t *status, const int64_t *out_off);
int pileup_alloc(rmr_pileup *p);
int pileup_append(rmr_pileup *p, const uint64_t *words, int64_t n);
int pileup_flush(rmr_pileup *p);
int launch_pileup_stamp(rmr_engine *e, int64_t n_records, const int64_t *out_off, const int32_t *part, int shift, uint64_t *words, int64_t n_words);
// the coverage join of one batch against the table of `p` (finished, nt > 0, p->cover allocated).  combine: `pr` is read and a
// '-' record is asked at the '-' focus of the first motif at a site; fold_window: how many words before and behind the place a
// binary search ends at are compared with a site's key (0 where a record's words are strictly monotone)
int launch_pileup_cover(rmr_pileup *p, const rmr_modbam_batch &b, const PileupRef &pr, bool combine, int fold_window, const int32_t *status,
                        const int64_t *cig_q, const int64_t *cig_r, const int64_t *out_off, const uint64_t *words, int64_t n_words,
                        const int32_t *part, int shift);
// k_pileup_duplex.hip: the emit that counts '-'-strand entries too (has_ref: with the reference part `pr`; pr.combine == 2 is
// the hemi mode of the fill: folded positions, strand bits kept), and the two passes that pair a record's '+' and '-' words
int launch_modbam_calls_duplex(rmr_engine *e, const rmr_modbam_batch &b, const PileupEmit &pe, const PileupRef &pr, bool has_ref, int32_t *ords,
                               int64_t *cig_q, int64_t *cig_r, int64_t *counts, int32_t *status, const int64_t *out_off);
int launch_pileup_pairs(rmr_engine *e, int64_t n_records, const int64_t *out_off, const uint64_t *words, int64_t n_words, int n_codes,
                        int64_t *pairs, const int64_t *pair_off, uint64_t *pair_words);

// k_read_index.hip: keys u8[n][16], values i64[n] on the host (n >= 1) -> the table of `ix`;  names / name_off / out on the
// device, the text of name i at names[name_off[i] - base ...]
int read_index_build(rmr_engine *e, const uint8_t *keys, const int64_t *values, int64_t n, rmr_read_index *ix);
int launch_read_index_lookup(rmr_engine *e, const rmr_read_index *ix, const char *names, const int64_t *name_off, int64_t base, int64_t m,
                             int64_t *out);

int launch_encode(rmr_engine *e, int kb, int ka, const int8_t *seqs, int seq_w,
                  const int16_t *maps, int map_w, const int16_t *lens, int64_t n, int sig_len,
                  float *out);
int launch_trim(rmr_engine *e, int sb, int sa, int cb, int ca, int tsc, int8_t *seqs, int seq_w,
                int16_t *maps, int map_w, int16_t *lens, int64_t n);
int launch_moves(rmr_engine *e, const int8_t *mv_tag, int64_t mv_tag_len, int64_t sig_len,
                 int reverse, int64_t *q2s, int64_t *d_count);
int launch_moves_batch(rmr_engine *e, const int8_t *mv_tags, const int64_t *mv_off, const int64_t *sig_len,
                       const int64_t *seq_len, int64_t n, int check, int reverse, int64_t *q2s, int64_t *counts,
                       int32_t *status);
int launch_signal_range(rmr_engine *e, const int16_t *signal, const int64_t *start, const int64_t *len, int64_t n, int32_t *lo, int32_t *hi);
int launch_signal_hist(rmr_engine *e, const int16_t *signal, const int64_t *start, const int64_t *len, const int32_t *lo,
                       const int64_t *hist_off, int64_t n, unsigned int *hist);
int launch_assemble_lengths(rmr_engine *e, const int64_t *q2s, const int64_t *q2s_off, const int64_t *seq_len, const int64_t *span_len,
                            int64_t n, int64_t *len_out);
int launch_assemble_reads(rmr_engine *e, const int16_t *signal, const int64_t *src_start, const int64_t *span_len, const int64_t *q2s,
                          const int64_t *q2s_off, const int64_t *sig_off, const int64_t *seq_off, int64_t n, int16_t *dacs, int64_t *s2s);
int launch_geometry(rmr_engine *e, const rmr_reads &d, int64_t n_chunks, const int32_t *chunk_read,
                    float *sig_out, int64_t total_sig, const int32_t *sig_read, int64_t *geo,
                    int *d_max_seq_len);
int launch_fill(rmr_engine *e, const rmr_reads &d, int64_t n_chunks, const int32_t *chunk_read,
                const float *sig, const int64_t *geo, float *signal, int8_t *seqs, int seq_w,
                int16_t *maps, int map_w, int16_t *lens, int64_t *rfb);
int launch_chunk_read(rmr_engine *e, const int64_t *focus_off, int64_t n_reads, int64_t n_chunks, int32_t *out);
int launch_count(rmr_engine *e, const float *logits, int64_t n, int num_out, int64_t *counts);
// k_probe.hip: out[0] = bits of max |a - b| over the entries finite in both, out[1] = non-finite entries of a and b
int launch_probe_compare(rmr_engine *e, const float *a, const float *b, int64_t n, unsigned *out);
int launch_validation_tally(rmr_engine *e, const float *logits, const int64_t *labels, int64_t n, int km, int kf, const int *colmap,
                            int64_t *conf, float *win, uint8_t *pred, double *loss_sum);
int launch_vbz(rmr_engine *e, const uint8_t *svb, const int64_t *row_off, const int32_t *row_n, const int64_t *out_off,
               int64_t n_rows, int16_t *out, int32_t *status);
int launch_motif_focus(rmr_engine *e, const int8_t *seq, const int64_t *seq_off, int n_reads, const rmr_motif_set &ms,
                       int64_t *counts, const int64_t *foc_off, int64_t *focus);
// k_modbam.hip: the site join of `validate from_modbams` (count pass: out_off == nullptr)
int launch_modbam_sites(rmr_engine *e, const rmr_modbam_batch &b, int32_t *ords, int64_t *cig_q, int64_t *cig_r, int64_t *counts,
                        int32_t *status, const int64_t *out_off, float *probs, uint8_t *label, int64_t *qpos, int64_t *rpos);
// k_duplex.hip: one group of simplex-to-duplex alignments whose traces share `trace` (rmr_duplex_align).  A job's offsets: bases in
// `bases`, dwords in `trace`, entries in `line` (m of them) and in `runs` (2 m + 2); its result goes to out[out_idx].
struct DuplexJob {
    int64_t q_off, r_off, trace_off, line_off, run_off;
    int32_t n, m, out_idx, pad;
};
int launch_duplex_group(rmr_engine *e, const DuplexJob *jobs, int n_jobs, const uint8_t *bases, uint32_t *trace, int2 *line, int2 *best,
                        uint32_t *runs, int32_t *out);
// The same group in checkpointed memory (rmr_duplex_align_mode): a job's `line` entries are one line of m per strip
// (ceil(n / STRIP_ROWS) * m of them) and its `trace` dwords the trace of ONE strip ((m + 63) * 64).
int launch_duplex_group_checkpoint(rmr_engine *e, const DuplexJob *jobs, int n_jobs, const uint8_t *bases, uint32_t *trace, int2 *line,
                                   int2 *best, uint32_t *runs, int32_t *out);
int launch_motif(rmr_engine *e, const int8_t *seq, const int64_t *seq_off, int n_reads, int64_t total,
                 const rmr_motif_set &ms, uint8_t *flags);

// the inputs of a forward call as the front kernels read them: the signal and either a dense one-hot tensor or the chunk arrays
struct ChunkArrays {
    const float *signal;  // [n][L]
    const float *enc;     // [n][EC][L], or nullptr: the k-mers are gathered from (seqs, maps, lens)
    const int8_t *seqs;  int seq_w;  // [n][seq_w]
    const int16_t *maps; int map_w;  // [n][map_w]
    const int16_t *lens; int kb, ka;  // [n]
    // the same arrays from chunk c0 on
    ChunkArrays at(int64_t c0, int L, int EC) const {
        if (enc) return ChunkArrays{signal + (size_t)c0 * L, enc + (size_t)c0 * EC * L, nullptr, 0, nullptr, 0, nullptr, 0, 0};
        return ChunkArrays{signal + (size_t)c0 * L, nullptr, seqs + (size_t)c0 * seq_w, seq_w, maps + (size_t)c0 * map_w, map_w, lens + c0, kb, ka};
    }
};

// fused pipeline stages; all tensors channel-last in device scratch
int launch_front(rmr_model *m, hipStream_t st, const ChunkArrays &c, int64_t n, float *sig2, float *seq1 /* nullptr: skip seq path */);
int launch_seq1_dense(rmr_model *m, const float *enc, int64_t n, float *seq1);
// whether the two entries run seq_conv1 of this model at all (what they refuse, they refuse by name before any launch)
bool front_seq_supported(const rmr_model *m, int seq_w, int map_w);
bool seq1_dense_supported(const rmr_model *m);
int check_seq1_dense(const rmr_model *m);  // the dense entry's refusal, by name
// the kernel switches of the fp32 path: read from the environment once per forward call (run_pipeline, api_forward.hip) and passed
// down, so that a change between two calls on the same model takes effect
struct FwdSwitches {
    bool fused;       // RMR_FUSED
    bool conv_front;  // RMR_CONV_FRONT
    bool winograd;    // RMR_WINOGRAD and the model's own decision (rmr_model::use_winograd)
    bool sig3_mfma;   // RMR_SIG3_MFMA
};
// k_conv_front.hip: fp32 sig_conv3 / seq_conv2 with their producers (sig_conv1/2, seq_conv1) folded into the staging
bool conv_front_supported(const rmr_model *m, int kb, int ka, int seq_w, int map_w);
// the signal half alone with sig_conv2 on the matrix cores (both architectures, 5 or 11 taps): signal -> cat channels [0, 64)
bool sig3_front_mfma_supported(const rmr_model *m);
int launch_sig3_front_mfma(rmr_model *m, const float *signal, int64_t n, float *cat, bool winograd);
// whether the plans of the two folded fronts take their Winograd kernels for a batch of n chunks (the guard's question)
bool sig3_front_takes_winograd(const rmr_model *m, int64_t n);
bool seq2_front_takes_winograd(const rmr_model *m, int seq_w, int map_w, int64_t n);
int launch_conv_front(rmr_model *m, const ChunkArrays &c, int64_t n, float *cat, const FwdSwitches &sw);
int launch_conv(rmr_engine *e, const ConvLayer &c, const float *in, int in_row, int pin,
                float *out, int out_row, int out_coff, int pout, int64_t n, bool winograd);
int launch_lstm_head(rmr_model *m, const float *x, int64_t n, float *logits);
// k_wino.hip: the 5-tap stride-1 layers of 64 output channels as a Winograd F(4, 5) convolution (0.4 of the direct form's MFMAs)
bool conv_wino_supported(const ConvLayer &c, int pin, int pout);
int launch_conv_wino(rmr_engine *e, const ConvLayer &c, const float *in, int in_row, int pin, float *out, int out_row, int out_coff,
                     int pout, int64_t n);
// the stride-3 layers from 16 to 64 channels (sig_conv3, seq_conv2) as polyphase Winograd convolutions
bool conv_wino_s3_supported(const ConvLayer &c, int pin, int pout);
int launch_conv_wino_s3(rmr_engine *e, const ConvLayer &c, const float *in, int in_row, int pin, float *out, int out_row, int out_coff,
                        int pout, int64_t n);
// k_stream.hip: the same layers with the weights streamed from L2 (channel counts above 64, any multiple of 16 up to 256)
int launch_conv_stream(rmr_engine *e, const ConvLayer &c, const float *in, int in_row, int pin, float *out, int out_row, int out_coff,
                       int pout, int64_t n);
int launch_lstm_stream(rmr_model *m, const float *x, int64_t n, float *logits);
// k_stream16.hip: the same network in the 16-bit dtypes (activations 16-bit in HBM between the launches)
int launch_conv_stream16(rmr_model *m, const ConvLayer &c, const void *in, bool in16, int pin, uint16_t *out, int out_row, int out_coff, int pout,
                         int64_t n);
int check_conv_stream16(const ConvLayer &c, int pin);  // whether one chunk of `pin` input rows fits a block's LDS (else the refusal by name)
int launch_lstm_stream16(rmr_model *m, const uint16_t *x, int64_t n, float *logits);
int launch_lstm_head_split(rmr_model *m, const float *x, int64_t n, float *logits);
int launch_conv_split(rmr_engine *e, const ConvLayer &c, int np, const float *in, int in_row, int pin,
                      float *out, int out_row, int out_coff, int pout, int64_t n);
int launch_fc_head(rmr_model *m, const float *m4, int64_t n, float *logits);
// fused bf16 front (k_fused.hip): chunk arrays -> x bf16[n][T][64];  lstm on that tensor (k_lstm_bf16s.hip)
bool fused_front_supported(const rmr_model *m, int seq_w, int map_w);
int launch_fused_front(rmr_model *m, const ChunkArrays &c, int64_t n, uint16_t *x);
bool lstm_x16s_supported(const rmr_model *m);
int launch_lstm_head_x16s(rmr_model *m, const float *x, int64_t n, float *logits);
int launch_lstm_head_x16(rmr_model *m, const uint16_t *x, int64_t n, float *logits);

// k_train.hip: the training step (api_train.hip).  Row r of a product is `rs`-spaced inside chunk r / rpc: its first float is
// (r / rpc) * cs + (r % rpc) * rs + off of the buffer, and floats outside [0, valid) of the chunk read as zero / are not written
struct TrainSpan {
    int rpc;
    long long cs;
    int rs, off;
    long long valid;
};
int train_gemm(rmr_engine *e, const float *A, const TrainSpan &sa, const float *B, int ldb, int K, float *C, const TrainSpan &sc, int NC,
               long long R, const float *bias);
int train_wgrad(rmr_engine *e, const float *A, const TrainSpan &sa, const float *D, const TrainSpan &sd, int K, int NC, long long R, int IC,
                int KW, float *part, size_t part_floats, const int *refused, float *grad);
int train_repack(rmr_engine *e, const float *W, int OC, int IC, int KW, int P, int J, int mode, float *out);
int train_colsum_blocks(long long R);
int train_bn_forward(rmr_engine *e, const float *Y, int C, long long R, float *stat, const float *gamma, const float *beta, float *run_mean,
                     float *run_var, float *part, const int *refused, float *out, int aw, int coff);
int train_bn_backward(rmr_engine *e, const float *Y, int C, long long R, float *stat, const float *gamma, const float *beta, const float *dA, int aw,
                      int coff, float *part, const int *refused, float *dgamma, float *dbeta, float *dY, float *dbias);
int train_bias_grad(rmr_engine *e, const float *D, int C, long long R, float *part, const int *refused, float *out, float *out2);
int train_sig1(rmr_engine *e, const float *sig, int L, int Lout, int OC, int KW, const float *w, const float *b, long long n, float *y);
int train_seq_transpose(rmr_engine *e, const float *in, int EC, int L, long long n, float *out);
int train_fill(rmr_engine *e, float *p, long long n, float v, const int *refused);
int train_lstm_step(rmr_engine *e, float *G, float *Cs, float *H, float *Z, const float *WhhT, int S, int T, int t, long long n);
int train_lstm_step_bwd(rmr_engine *e, float *G, const float *Cs, const float *H, const float *Whh, const float *dz1, float *dc, int S, int T, int t,
                        long long n);
int train_lstm2(rmr_engine *e, float *G2, float *C2, float *H2, float *Z2, int S, long long n);
int train_lstm2_bwd(rmr_engine *e, float *G2, const float *C2, const float *H2, const float *dlog, const float *fcw, int num_out, int S, long long n);
int train_count_rows(rmr_engine *e, const uint8_t *mask, const int64_t *labels, int num_out, long long n, int *count);
int train_fc_loss(rmr_engine *e, const float *Z2, const float *fcw, const float *fcb, int S, int num_out, const int64_t *labels, const uint8_t *mask,
                  const int *count, long long n, float *logits, float *dlog, float *loss_part, float *logits_out, float *loss);
int train_adamw(rmr_engine *e, float *p, float *g, float *m, float *v, const uint8_t *tensor_of, long long n, float lr_wd, float omb1, float b2,
                float omb2, float eps, float step_size, float bc2_sqrt, const float *clip);
int train_absmax(rmr_engine *e, const float *g, const long long *off, const long long *size, int n_tensors, float *out);

// integer switch from the environment (DESIGN.md has the table of every name the product reads)
inline int tune_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}
// the same for the knobs of the experiment build (make abl: -DRMR_TIMING_ABLATIONS); the shipped library returns the default
// without looking at the environment, so none of them is a configuration of the product
inline int abl_int(const char *name, int dflt) {
#ifdef RMR_TIMING_ABLATIONS
    return tune_int(name, dflt);
#else
    (void)name;
    return dflt;
#endif
}

// fast integer division by a small runtime constant (exact for 0 <= x < 2^24, d < 2^12)
struct FastDiv {
    int d;
    float inv;
};
inline FastDiv make_fastdiv(int d) { return FastDiv{d, 1.0f / (float)d}; }

}  // namespace rmr
