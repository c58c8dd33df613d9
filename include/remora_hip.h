/*
 * remora_hip.h — C ABI of libremora_hip.so, the MI355X (gfx950) engine for the per-read
 * modified-base-call hot path of nanoporetech/remora (v3.2.0).
 *
 * Every entry point replaces one reference interface on that path; the reference
 * file:line it stands in for is cited on each declaration (paths relative to the
 * reference checkout).  Plain pointers and sizes only — no torch / numpy types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative rmr_status otherwise; the message
 *     is available (thread-local) from rmr_last_error().  Nothing aborts the process.
 *     The Python host turns non-zero into remora_amd.RemoraError — the one exception type
 *     the reference's callers catch (src/remora/__init__.py:4-7, inference.py:88).
 *   - `mem` says where the caller's data buffers live: RMR_MEM_HOST (numpy / malloc; the
 *     engine stages them through device scratch and copies results back before returning;
 *     rmr_infer_chunks uploads large batches sub-batch by sub-batch through pinned slots on
 *     a second stream, under the kernels of the previous sub-batch)
 *     or RMR_MEM_DEVICE (hipMalloc / torch `data_ptr()`; work is enqueued on the engine
 *     stream and the call returns without synchronising — call rmr_engine_synchronize).
 *   - the caller owns every input and output buffer; the engine owns only weights,
 *     scratch and its stream; no caller pointer is retained past return
 *     (mirrors the Cython memoryview borrow semantics, src/remora/encoded_kmers.pyx:16-18).
 *   - chunk arrays use the CoreRemoraDataset layout (src/remora/data_chunks.py:786-816,
 *     :942-948): signal f32[n,1,L]; sequence i8[n,seq_w]; sequence_to_signal_mapping
 *     i16[n,map_w]; sequence_lengths i16[n]; all C-contiguous.
 *   - an engine (and the models created on it) may be used from several host threads; calls
 *     on one engine are serialised by an internal mutex (reference runs the model from a
 *     Thread: src/remora/inference.py:544-550, :973-982).
 */
#ifndef REMORA_HIP_H
#define REMORA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#pragma GCC visibility push(default)

typedef struct rmr_engine rmr_engine;
typedef struct rmr_model rmr_model;

enum rmr_status {
    RMR_OK = 0,
    RMR_ERR_INVALID = -1,     /* bad argument / unsupported configuration */
    RMR_ERR_HIP = -2,         /* HIP runtime error (message carries hipGetErrorString) */
    RMR_ERR_NOMEM = -3,
    RMR_ERR_DISCORDANT_SEQ = -4, /* "Move table discordant with basecalls" io.py:403-404 */
    RMR_ERR_DISCORDANT_SIG = -5  /* "Move table discordant with signal"    io.py:405-406 */
};

enum rmr_mem { RMR_MEM_HOST = 0, RMR_MEM_DEVICE = 1 };
enum rmr_arch {
    RMR_ARCH_CONV_LSTM = 0, /* models/ConvLSTM_w_ref.py */
    RMR_ARCH_CONV_ONLY = 1  /* models/Conv_w_ref.py     */
};

const char *rmr_last_error(void);
const char *rmr_version(void); /* "remora_hip <major>.<minor> (gfx950)"; the minor number changes with every struct or entry-point change */

/* ---- engine ------------------------------------------------------------------------ */

/* One engine per process per GPU.  With RMR_ENGINE_USE_STREAM in `flags` the engine enqueues
 * on the caller's hipStream_t `stream` (NULL = the legacy default stream; e.g. torch's current
 * stream, so that ordering with the caller's tensors is implicit); otherwise `stream` is
 * ignored and the engine creates its own non-blocking stream.
 * replaces: `tensor.to(device)` single-device plumbing, src/remora/inference.py:311-314,
 *           src/remora/util.py:81-92 (parse_device). */
enum rmr_engine_flags { RMR_ENGINE_OWN_STREAM = 0, RMR_ENGINE_USE_STREAM = 1 };
int rmr_engine_create(int device, void *stream, int flags, rmr_engine **out);
void rmr_engine_destroy(rmr_engine *e);
int rmr_engine_synchronize(rmr_engine *e);
/* Stream-ordered hand-over between two engines of one device: everything queued on `producer` so far is finished before
 * anything queued on `waiter` from now on starts - an event, no host wait.  (A caller that extracts chunks on one engine
 * and runs the network on another - the reads pipeline - needs no hipStreamSynchronize in between.)
 * replaces: nothing in the reference (one stream, one thread: src/remora/inference.py:277-316). */
int rmr_engine_wait_for(rmr_engine *waiter, rmr_engine *producer);
/* chunks per internal sub-batch of the fused pipeline (scratch = ~33 KB/chunk); 0 = default */
int rmr_engine_set_subbatch(rmr_engine *e, int64_t chunks);

/* ---- model (L4: model_util.load_model hands the weights over) ------------------------ */

typedef struct {
    int32_t arch;       /* rmr_arch */
    int32_t size;       /* model_params["size"]: any int >= 1 (src/remora/parsers.py:858-862; constants.py:1 default 64).  The
                           kernels run at 16 / 32 / 64 channels (weight slices resident in registers) or, above 64, at the next
                           multiple of 16 up to 256 (weights streamed from L2, fp32 only); a size in between is run at the next
                           of those with zero-weight channels added (rmr_model_padded_size) - same logits */
    int32_t kmer_len;   /* kmer_context_bases[0] + [1] + 1 */
    int32_t num_out;    /* len(mod_bases) + 1, <= 16 */
    int32_t chunk_len;  /* sum(chunk_context) */
    int32_t dtype;      /* 0 = fp32 MFMA (exact fp32); bf16 MFMA with fp32 accumulate and split operands:
                           1 = bf16, 2 = bf16x3 (2-part split, ~2^-16), 3 = bf16x6 (3-part split, fp32 class);
                           4 = f16: IEEE-half operands, fp32 accumulate, on the fused kernels (conv_lstm, size 64,
                           k-mer length 9 or 6; rmr_infer_chunks only) - the 16-bit pipeline with 10 mantissa bits;
                           5 = f16x3: operands split into two IEEE-half parts, three products (hi hi, hi lo, lo hi) on the
                           half MFMA, fp32 accumulate - 22 significand bits (fp32 class) at bf16x3's cost, in IEEE half's
                           RANGE: an input or folded weight beyond +-65504 becomes infinity (NaN logits), values below
                           2^-3 keep fewer than 22 bits (the low part is a half subnormal); bf16x6 has fp32's exponent range */
} rmr_model_desc;

/* `weights`: host fp32 blob, the torch state_dict tensors flattened in forward order —
 *   for each conv layer: conv.weight[oc][ic][k], conv.bias, bn.weight, bn.bias,
 *   bn.running_mean, bn.running_var; conv layers in the order
 *     conv_lstm: sig_conv1..3, seq_conv1..2, merge_conv1
 *     conv_only: sig_conv1..3, seq_conv1..3, merge_conv1..4
 *   then (conv_lstm) lstm1 {weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0}, lstm2 {same};
 *   then fc.weight, fc.bias.
 * The engine folds BatchNorm (eval, eps 1e-5) into the convolutions and repacks everything
 * into MFMA fragment order on the device.
 * replaces: torch.jit.load + ScriptModule.state_dict(), src/remora/model_util.py:468-481,
 *           :532-563; layer sets as in :231-263. */
int rmr_model_create(rmr_engine *e, const rmr_model_desc *desc, const float *weights,
                     size_t n_floats, rmr_model **out);
void rmr_model_destroy(rmr_model *m);
/* number of floats rmr_model_create expects for `desc` (0 if desc is unsupported) */
size_t rmr_model_weight_count(const rmr_model_desc *desc);
/* The channel count the kernels run a network of desc->size channels at (0 if desc is unsupported), and the network's blob
 * at that size: `weights` (rmr_model_weight_count(desc) floats) with zero-weight channels added -> `out` (out == NULL: only
 * *out_n and *padded_desc are set).  rmr_model_create applies this itself; the entry exists so that a host can see - and a
 * test can check against the reference's forward - exactly which network the kernels evaluate.
 * replaces: nothing (models/ConvLSTM_w_ref.py:11-37 builds layers of any `size`; torch needs no padding). */
int rmr_model_padded_size(const rmr_model_desc *desc);
int rmr_model_pad_weights(const rmr_model_desc *desc, const float *weights, size_t n_floats, rmr_model_desc *padded_desc,
                          float *out, size_t out_cap, size_t *out_n);

/* The form the fp32 kernels run this model's Winograd-capable layers in.  A fp32 model of which at least one layer has a
 * Winograd kernel (merge_conv1 / merge_conv2 as F(4,5), sig_conv3 / seq_conv2 / seq_conv3 as polyphase F(4,3) / F(4,5)) is
 * screened by rmr_model_create: a fixed batch of probe chunks at the model's own chunk and k-mer length goes through the
 * network twice on the device, once in the Winograd and once in the direct form, and the Winograd kernels stay in use only
 * if every logit of both runs is finite and the two differ by at most `tol` (default 2e-5).  Every forward entry of the
 * model (rmr_forward, rmr_infer_chunks, rmr_call_read) follows the decision; RMR_WINOGRAD=0 still selects the direct form
 * per call.  A screen on 256 chunks, not a proof.  Models without a Winograd layer (the 16-bit and split dtypes, sizes
 * other than 64) are not screened: checked = 0, winograd = 0.  The probe is handed over as chunk arrays; a k-mer length
 * above 21, which rmr_infer_chunks refuses, takes the same batch as a one-hot tensor through rmr_forward's path, and a model
 * that neither entry runs (the one-hot tensor of one chunk beyond the LDS) is not screened.
 * replaces: nothing (torch.nn.Conv1d has one form; the layers concerned are models/ConvLSTM_w_ref.py:36-37,50 and
 *           models/Conv_w_ref.py:35-38,54-55). */
typedef struct rmr_model_numerics {
    int32_t checked;        /* 1: the probe ran for this model */
    int32_t winograd;       /* 1: fp32 Winograd kernels in use; 0: direct forms */
    int32_t probe_chunks;
    int32_t nonfinite;      /* non-finite logits seen in either form */
    float   max_abs_diff;   /* max |winograd - direct| over the probe's logits (entries finite in both forms) */
    float   tol;
} rmr_model_numerics;
int rmr_model_numerics_get(const rmr_model *m, rmr_model_numerics *out);
/* re-run the probe with another tolerance and adopt its decision; tol < 0 restores the default.  tol = 0 forces the direct
 * forms unless the two are bit-equal; tol = INFINITY forces Winograd (non-finite logits still select the direct forms).  A
 * model that is not screened keeps checked = 0.  Synchronises the engine's stream; leaves its sub-batch setting and its
 * profiler counters as they were.
 * replaces: nothing (as above). */
int rmr_model_check_winograd(rmr_model *m, float tol, rmr_model_numerics *out);

/* ---- E1: k-mer one-hot encode with move-table expansion ------------------------------ */
/* replaces: encoded_kmers.compute_encoded_kmer_batch, src/remora/encoded_kmers.pyx:13-45.
 * out: f32[n, 4*(kb+ka+1), sig_len].  The reference takes sig_len from chunk 0
 * (:23, maps[0, lens[0]]); the host wrapper does the same and passes it in. */
int rmr_encode_kmers(rmr_engine *e, int kb, int ka, const int8_t *seqs, int seq_w,
                     const int16_t *maps, int map_w, const int16_t *lens, int64_t n,
                     int sig_len, float *out, int mem);

/* ---- T1: trim stored chunk context to the model's (in place) -------------------------- */
/* replaces: data_chunks_core.trim_sb_chunk_context_core, src/remora/data_chunks_core.pyx:10-45.
 * As in the reference the caller has already subtracted (stored_before - cc_before) from
 * `maps` (src/remora/data_chunks.py:1555-1563). */
int rmr_trim_chunk_context(rmr_engine *e, int stored_before, int stored_after, int cc_before,
                           int cc_after, int total_seq_context, int8_t *seqs, int seq_w,
                           int16_t *maps, int map_w, int16_t *lens, int64_t n, int mem);

/* ---- M1: move-table expansion ---------------------------------------------------------- */
/* replaces: io.parse_move_tag, src/remora/io.py:394-407.  mv_tag = [stride, m0, m1, ...]
 * (int8, host or device).  q2s capacity must be >= mv_tag_len.  *n_out = #moves + 1.
 * seq_len < 0 means None.  Errors: RMR_ERR_DISCORDANT_SEQ / _SIG when `check`. */
int rmr_parse_moves(rmr_engine *e, const int8_t *mv_tag, int64_t mv_tag_len, int64_t sig_len,
                    int64_t seq_len, int check, int reverse_signal, int64_t *q2s,
                    int64_t *n_out, int mem);
/* The same for a batch of reads in one launch (one block per move table): `mv_tags` is the concatenation of
 * the tables, table i at [mv_off[i], mv_off[i+1]); its coordinates are written to q2s[mv_off[i] ...] (a table of
 * m entries yields at most m), counts[i] of them; status[i] = 0 or the code rmr_parse_moves would return for
 * that read (RMR_ERR_DISCORDANT_SEQ / _SIG when `check`, RMR_ERR_INVALID for an empty table or stride <= 0).
 * The call itself fails only on argument errors.  Used by the POD5+BAM ingest, which parses the move tables of
 * a whole batch of alignments at once instead of one kernel launch per read. */
int rmr_parse_moves_batch(rmr_engine *e, const int8_t *mv_tags, const int64_t *mv_off,
                          const int64_t *sig_len, const int64_t *seq_len, int64_t n_reads, int check,
                          int reverse_signal, int64_t *q2s, int64_t *counts, int32_t *status, int mem);
/* Counting half of the median / MAD scaling of reads without sm / sd tags (io.Read.compute_pa_to_norm_scaling,
 * src/remora/io.py:1851-1856: np.median of the pA signal and of its absolute deviations - order statistics of a function of the
 * int16 samples, so counts are all the GPU has to deliver).  `signal`: device-resident decoded samples; span i = signal[start[i]
 * .. start[i] + len[i]) (start, len: host arrays).  Called twice, like the motif scan: with hist == NULL it writes the smallest
 * and largest sample of every span to lo / hi (host int32[n]; an empty span gets lo > hi); with hist != NULL the caller passes
 * those lo / hi back, hist_off (host int64[n + 1], the running sum of hi - lo + 1, 0 for empty spans) and receives
 * hist[hist_off[i] + (v - lo[i])] = the number of samples of span i equal to v (host uint32[hist_off[n]]).  Synchronous. */
int rmr_signal_histograms(rmr_engine *e, const int16_t *signal, const int64_t *start, const int64_t *len, int64_t n, int32_t *lo,
                          int32_t *hi, const int64_t *hist_off, uint32_t *hist);

/* replaces: for a whole batch, the tail of io.Read.add_alignment and Read.into_remora_read (src/remora/io.py:2003-2012:
 * the signal of an alignment is dacs[sp:][ts:ns]; :2123-2177: the read keeps dacs[q2s[0]:q2s[-1]] and the mapping q2s -
 * q2s[0]) on arrays that are already resident: `signal` (device) holds the decoded samples of the batch back to back,
 * read i's trimmed signal starts at signal[src_start[i]]; its move-table coordinates are the seq_len[i] + 1 values at
 * q2s[q2s_off[i] ...] (device, as rmr_parse_moves_batch wrote them).  Written (device): dacs, s2s [sum(seq_len) + n_reads],
 * d_sig_off / d_seq_off [n_reads + 1] - the rmr_reads layout; sig_off (host) receives the sample offsets.  src_start,
 * q2s_off, seq_len are host arrays.  Lets the POD5 + BAM ingest hand batches to the extraction without per-read host work. */
int rmr_assemble_reads(rmr_engine *e, int64_t n_reads, const int16_t *signal, const int64_t *src_start, const int64_t *q2s,
                       const int64_t *q2s_off, const int64_t *seq_len, int16_t *dacs, int64_t dacs_cap, int64_t *s2s,
                       int64_t *d_sig_off, int64_t *d_seq_off, int64_t *sig_off);
/* The same with a direction.  replaces: the `reverse_signal` branches of that tail (src/remora/io.py:2001-2010: the signal of
 * an alignment is dacs[::-1][sp:][ts:ns][::-1] of the already reversed dacs, i.e. the SAME window of the raw signal, reversed;
 * :401-402: query_to_signal = sig_len - q2s[::-1]; :2123-2177 as above) - the reads of models whose metadata says
 * reverse_signal (direct RNA).  span_len[i] (host) is the length of read i's trimmed window, signal[src_start[i] ..
 * src_start[i] + span_len[i]); with reverse_signal != 0 the coordinates q = q2s[q2s_off[i] ...] are those of the reversed
 * window (rmr_parse_moves_batch with reverse_signal = 1, or the composition rmr_ref_anchor_batch_dir wrote) and the read keeps
 *     dacs_i[k] = signal[src_start[i] + span_len[i] - 1 - (q[0] + k)],  0 <= k < q[last] - q[0];   s2s_i[k] = q[k] - q[0].
 * A mapping outside [0, span_len[i]] fails the call (RMR_ERR_INVALID) before anything is copied.  With reverse_signal == 0
 * span_len is not read (NULL allowed) and the call IS rmr_assemble_reads, which forwards here. */
int rmr_assemble_reads_dir(rmr_engine *e, int64_t n_reads, const int16_t *signal, const int64_t *src_start, const int64_t *span_len,
                           int reverse_signal, const int64_t *q2s, const int64_t *q2s_off, const int64_t *seq_len, int16_t *dacs,
                           int64_t dacs_cap, int64_t *s2s, int64_t *d_sig_off, int64_t *d_seq_off, int64_t *sig_off);

/* ---- N1: BAM records for the POD5+BAM ingest (host code: BGZF inflate + record / tag decode) ---------- */
/* replaces: what ReadIndexedBam / pysam hand to io.Read.add_alignment (src/remora/io.py:184-358, :1972-2084):
 * per alignment the flag, reference id / start, mapping quality, name, CIGAR, sequence, the tags mv, ts, ns, sp,
 * sm, sd, pi, MD, the record bytes as stored (for writing the record back with MM/ML tags), and - when
 * `want_ref` - the reference bases spanned by the alignment rebuilt from query + CIGAR + MD
 * (pysam.AlignedSegment.get_reference_sequence: mismatches lower case; ref_ok = 0 without MD / when MD and
 * CIGAR disagree).  Records arrive `max_records` at a time as flat arrays with [n+1] offset tables; every
 * pointer of the batch stays valid until the next rmr_bam_read_batch / rmr_bam_close on the same handle.
 * `has` bit i set = tag present: 0 mv (B:c), 1 ts, 2 ns, 3 sp, 4 sm, 5 sd, 6 pi, 7 MD.  `mv` excludes nothing:
 * [stride, m0, m1, ...] as stored.  n_records < max_records means end of file.
 * want_ref: bit 0 = rebuild the reference bases; bit 1 = identifiers only (flags, positions, names, the scalar tags, pi and
 * `has`; record bytes, bases, CIGAR, move table, MD and reference stay empty - their offset tables are all zero): what a
 * pass that only counts records against the signal file needs (get_read_ids, src/remora/io.py:362-391). */
typedef struct rmr_bam rmr_bam;
typedef struct rmr_bam_batch {
    int64_t n_records;
    const int32_t *flag, *ref_id, *pos, *mapq, *l_seq, *n_cigar;
    const int64_t *raw_off;   const uint8_t *raw;      /* record bytes (without the leading block_size) */
    const int64_t *name_off;  const char *names;
    const int64_t *seq_off;   const char *seq;         /* ASCII bases */
    const int64_t *cigar_off; const uint32_t *cigar;   /* BAM CIGAR words: len << 4 | op */
    const int64_t *tags_off;                           /* [n] offset of the tag region inside the record */
    const uint8_t *has;
    const int64_t *mv_off;    const int8_t *mv;
    const int32_t *ts, *ns, *sp;
    const float *sm, *sd;
    const int64_t *pi_off;    const char *pi;
    const int64_t *md_off;    const char *md;
    const uint8_t *ref_ok;
    const int64_t *refseq_off; const char *refseq;
    const int64_t *voffset;                            /* [n] BGZF virtual offset of the record (for rmr_bam_seek) */
} rmr_bam_batch;
int rmr_bam_open(const char *path, rmr_bam **out);
/* the same with the number of BGZF inflate workers of this handle given by the caller (>= 1; 0 = rmr_bam_open's default:
 * RMR_BAM_INFLATE_THREADS, else 8) - a caller that sizes its thread pools per rank passes the count instead of setting
 * an environment variable in a process whose native threads read the environment (pysam's `threads=` of
 * AlignmentFile, src/remora/io.py:236) */
int rmr_bam_open_threads(const char *path, int inflate_threads, rmr_bam **out);
void rmr_bam_close(rmr_bam *b);
/* everything before the first record (magic, header text, reference dictionary), uncompressed */
int rmr_bam_header(rmr_bam *b, const uint8_t **bytes, int64_t *n_bytes, int64_t *n_refs);
const char *rmr_bam_ref_name(rmr_bam *b, int64_t ref_id); /* NULL when out of range */
int rmr_bam_read_batch(rmr_bam *b, int64_t max_records, int want_ref, rmr_bam_batch *out);
/* continue reading at a record's virtual offset (compressed block offset << 16 | offset inside the inflated block),
 * as returned in rmr_bam_batch.voffset - the random access ReadIndexedBam.get_alignments needs
 * (src/remora/io.py:303-325) */
int rmr_bam_seek(rmr_bam *b, int64_t voffset);
/* From the current position to the end of the file: count the records and note the virtual offset of records 0, every,
 * 2*every, ... in voffsets[0..cap) (only block_size fields are read).  What a worker of a multi-GPU run needs to take a
 * contiguous share of the alignments by itself (one process per GPU, each seeks to its own range; north_star: "reads
 * shard embarrassingly across the GPUs") - the reference hands reads out from ONE reader process instead
 * (src/remora/inference.py:488-519).  Leaves the handle at end of file: rmr_bam_seek before reading. */
int rmr_bam_scan(rmr_bam *b, int64_t every, int64_t *voffsets, int64_t cap, int64_t *n_records);
/* The virtual offset of the first record that starts in a BGZF member at or behind byte `file_offset` of the file, found
 * WITHOUT the records in front of it (*voffset = -1: none); the handle is left there.  A position counts as a record start
 * when the record and the records chained behind it pass every structural check of the format (field ranges against
 * the header, printable name, CIGAR codes, a tag region that parses to block_size exactly).  With it N workers split a
 * file by byte ranges in O(1) instead of one O(file) pass; the worker in front verifies each guess for certain (its
 * own chain of records has to end on it).  Same reference counterpart as rmr_bam_scan. */
int rmr_bam_guess_start(rmr_bam *b, int64_t file_offset, int64_t *voffset);

/* ---- N3: the output side of `remora infer` for a batch of reads (host code) ----------------------------- */
/* replaces: util.format_mm_ml_tags (src/remora/util.py:485-537) as inference.post_process_reads calls it per read
 * (src/remora/inference.py:429-459; flagged slow in the source, :55).  Read r has calls call_off[r] .. call_off[r+1]:
 * pos[] = positions in its sequence seq[seq_off[r] .. seq_off[r+1]) (any order: sorted stably here), probs[call][n_mods]
 * = probabilities of the modified bases.  mod_codes = n_mods NUL-terminated short names one after the other ("m\0h\0",
 * ChEBI codes allowed).  Per read and modified base: "<can_base><strand><code>?,<gaps>;" appended to mm (gaps = canonical
 * bases skipped between consecutive calls) and floor(p * 256) clipped to 255 appended to ml (all calls of base 0, then of
 * base 1, ...); mm_off / ml_off [n_reads + 1] delimit the reads' slices; a read without calls gets empty slices. */
int rmr_format_mm_ml(int64_t n_reads, const char *seq, const int64_t *seq_off, const int64_t *pos, const double *probs,
                     const int64_t *call_off, int n_mods, const char *mod_codes, char can_base, char strand, char *mm,
                     int64_t mm_cap, int64_t *mm_off, uint8_t *ml, int64_t ml_cap, int64_t *ml_off);
/* replaces: pysam.AlignedSegment.from_dict(io_read.full_align) + the MM/ML tags, src/remora/inference.py:450, :619-623.
 * raw[r] = record r as stored (without block_size, raw_len[r] bytes), tags_off[r] = offset of its tag region.  Written to
 * `out`, one after the other: int32 block_size + the record with any MM/ML/Mm/Ml tag removed and, when has_tags[r],
 * MM:Z:<mm slice> and ML:B:C<ml slice> appended (has_tags[r] = 0: the record leaves without modified-base tags). */
int rmr_records_with_mod_tags(int64_t n_reads, const uint8_t *const *raw, const int64_t *raw_len, const int64_t *tags_off,
                              const char *mm, const int64_t *mm_off, const uint8_t *ml, const int64_t *ml_off,
                              const uint8_t *has_tags, uint8_t *out, int64_t out_cap, int64_t *out_len);
/* The same for reference-anchored calling (`infer --reference-anchored`): a record that gets tags and owns a non-empty slice
 * ref_seq[ref_off[r] .. ref_off[r+1]) - the reference bases of its alignment, forward strand - is written in the form the
 * reference writes there: CIGAR <len>M, that sequence, qualities 0xff (src/remora/inference.py:452-458); every other record
 * as rmr_records_with_mod_tags writes it.  The caller's `out` needs 4 + (len + 1) / 2 + len more bytes per such record. */
int rmr_records_with_mod_tags_ref(int64_t n_reads, const uint8_t *const *raw, const int64_t *raw_len, const int64_t *tags_off,
                                  const char *mm, const int64_t *mm_off, const uint8_t *ml, const int64_t *ml_off,
                                  const uint8_t *has_tags, const char *ref_seq, const int64_t *ref_off, uint8_t *out, int64_t out_cap,
                                  int64_t *out_len);

/* ---- `validate from_modbams`: modified-base calls read back from a BAM and joined with ground-truth sites -------------- */
/* The MM / ML tokeniser (host code, native threads).
 * replaces: htslib's bam_parse_basemod below pysam.AlignedSegment.modified_bases, which validate.check_mod_strand and
 * validate.parse_mod_read consume per read (src/remora/validate.py:414-446, :322-335) - the text half of it: tags found,
 * text turned into numbers; the walk along the read's bases is rmr_modbam_site_counts' (GPU).
 * Records as rmr_bam_batch delivers them: record r = raw[raw_off[r] .. raw_off[r+1]), its tag region tags_off[r] bytes in.
 * MM / Mm (type Z) and ML / Ml (type B, subtype C) are looked for; one MM entry is
 *     ([ACGTUN])([+-])([a-z]+|[0-9]+)([.?]?)(,[0-9]+)*;
 * a run of letters is that many single-letter codes (at most RMR_MOD_MAX_CODES), a run of digits one ChEBI code.  An entry
 * of c codes and n deltas owns c * n ML bytes, call-major (per call the codes in listed order); ML is consumed in entry order.
 * status[r]: 0 ok; 1 no MM tag; 2 malformed (tag region does not parse, MM / ML of another type, bad grammar, a number
 * beyond int32, ML shorter or longer than the entries need, ML absent while an entry has deltas).  Records with a status
 * other than 0 own no entries, deltas or ML bytes.
 * rmr_mod_tags_sizes counts per record (n_entries, n_deltas, n_ml: int64[n]); the caller's exclusive prefix sums are the
 * [n+1] offset tables of rmr_mod_tags_fill, which writes the entry table, the flat int32 deltas and the flat ML bytes
 * (RMR_ERR_INVALID when the tables are not the counts of these records).  delta_off / ml_off inside an entry index the
 * flat arrays of the batch. */
#define RMR_MOD_MAX_CODES 16
typedef struct rmr_mod_entry {
    int64_t delta_off;               /* deltas[delta_off .. delta_off + n_deltas) */
    int64_t ml_off;                  /* ml[ml_off .. ml_off + n_codes * n_deltas) */
    int32_t n_deltas, n_codes;
    int32_t chebi;                   /* the ChEBI code of a numeric entry (n_codes = 1, codes[0] = 0), else 0 */
    char base, strand, flag, pad;    /* [ACGTUN], [+-], '.', '?' or 0 (absent) */
    char codes[RMR_MOD_MAX_CODES];   /* single-letter codes in listed order */
} rmr_mod_entry;
int rmr_mod_tags_sizes(int64_t n, const uint8_t *raw, const int64_t *raw_off, const int64_t *tags_off, int32_t *status,
                       int64_t *n_entries, int64_t *n_deltas, int64_t *n_ml, int threads);
int rmr_mod_tags_fill(int64_t n, const uint8_t *raw, const int64_t *raw_off, const int64_t *tags_off, const int32_t *status,
                      const int64_t *ent_off, const int64_t *delta_off, const int64_t *ml_off, rmr_mod_entry *entries, int32_t *deltas,
                      uint8_t *ml, int threads);
/* One aux field per record (host), for the partition tag of `analyze pileup_modbams`.
 * rmr_bam_aux_values: for the records as above, the first aux field named tag[0] tag[1] ([A-Za-z][A-Za-z0-9]):
 * kind[r] = RMR_AUX_ABSENT; RMR_AUX_INT with value[r] the number, for the types c C s S i I; RMR_AUX_CHAR with value[r] the
 * byte, for type A; RMR_AUX_OTHER_TYPE with value[r] the type letter, for Z H B f; RMR_AUX_UNWALKABLE (value 0) when the
 * fields of the aux region do not tile it - the regions rmr_mod_tags_sizes gives status 2 for their framing.  Nothing at or
 * behind raw_off[r + 1] is read. */
#define RMR_AUX_ABSENT 0
#define RMR_AUX_INT 1
#define RMR_AUX_CHAR 2
#define RMR_AUX_OTHER_TYPE 3
#define RMR_AUX_UNWALKABLE 4
int rmr_bam_aux_values(int64_t n, const uint8_t *raw, const int64_t *raw_off, const int64_t *tags_off, const char *tag, int64_t *value,
                       uint8_t *kind, int threads);

/* The site join (GPU; DEVICE pointers only, asynchronous on the engine's stream).
 * replaces: validate.check_mod_strand + validate.parse_mod_read for a batch of records (src/remora/validate.py:296-446):
 * the loop over pysam's get_aligned_pairs(with_seq=True) with a dictionary lookup per pair, and the base walk of
 * modified_bases.  Per record, one workgroup:
 *   - skipped whole, status set: 1 / 2 the tokeniser's status, 3 ref_id < 0, 4 no MD tag (has bit 7; the reference returns
 *     nothing for such a read, :309-313), 5 no entry that counts (check_mod_strand), 2 also for a call beyond the last
 *     occurrence of its base (any entry) and for a CIGAR whose query length is not the read's;
 *   - the original sequence is the stored one, reverse-complemented for flag 0x10; call k of an entry sits on occurrence
 *     d_0 + .. + d_k + k of the entry's base in it (N: every base; U counts T); its stored position is L-1-p there;
 *   - entries that count: strand '+', and of their codes those among mod_codes (the alphabet's modified bases, n_mods <= 7;
 *     ChEBI entries never count); p = (ML + 0.5) / 256 per code, the later entry wins where two give one code at one
 *     position, other columns 0, column 0 = 1 - sum (all multiples of 1/512: exact);
 *   - stored position -> reference position through the CIGAR (inside M / = / X only); the position is kept when the truth
 *     table of (ref_id, strand of the record) holds it.
 * Truth table: positions i64 ascending per (ref_id, strand) slice with their label u8, slice 2 * ref_id + (reverse ? 1 : 0)
 * = [truth_off[s], truth_off[s+1]); a ref_id >= n_refs has no truth.
 * rmr_modbam_site_counts writes counts i64[n] and status i32[n] and fills the workspaces ords i32[total deltas], cig_q /
 * cig_r i64[total CIGAR words]; the caller's exclusive prefix sum of counts is out_off i64[n+1] of rmr_modbam_site_fill
 * (same batch, same workspaces, same status), which writes probs f32[][n_mods + 1], label u8[], qpos i64[] (stored
 * coordinate), rpos i64[]: records in batch order, ascending stored position inside a record (the order of aligned_pairs). */
typedef struct rmr_modbam_batch {
    int64_t n_records;
    const uint8_t *seq;      const int64_t *seq_off;     /* ASCII bases as stored */
    const uint32_t *cigar;   const int64_t *cigar_off;   /* BAM CIGAR words */
    const int32_t *flag, *ref_id, *pos;
    const uint8_t *has;                                  /* rmr_bam_batch.has */
    const int32_t *tok_status;                           /* rmr_mod_tags_sizes */
    const int64_t *ent_off;  const rmr_mod_entry *entries;
    const int32_t *deltas;   const uint8_t *ml;
    int64_t n_deltas, n_ml;                              /* sizes of the two flat arrays (bounds of the entries' ranges) */
    int32_t n_mods; char mod_codes[8];
    int64_t n_refs;          const int64_t *truth_off;   /* [2 * n_refs + 1] */
    const int64_t *truth_pos; const uint8_t *truth_label;
} rmr_modbam_batch;
int rmr_modbam_site_counts(rmr_engine *e, const rmr_modbam_batch *b, int32_t *ords, int64_t *cig_q, int64_t *cig_r, int64_t *counts,
                           int32_t *status);
int rmr_modbam_site_fill(rmr_engine *e, const rmr_modbam_batch *b, const int32_t *ords, const int64_t *cig_q, const int64_t *cig_r,
                         const int32_t *status, const int64_t *out_off, float *probs, uint8_t *label, int64_t *qpos, int64_t *rpos);

/* ---- `analyze pileup_modbams`: the modified-base calls of BAM records counted per reference site ----------------------- */
/* The reference's command line has no such step; its users build this table (bedMethyl) from the output BAM with a CPU
 * pileup over a sorted, indexed file.  Here the calls are keyed by site, sorted and counted on the device.
 * A site word:  ref_id << 36 | pos << 5 | strand << 4 | code  (24 + 31 + 1 + 4 bits; strand 0 '+', 1 '-'; code = the call's
 * class 0 .. n_mods, or n_mods + 1 = `fail`).  A site key is word >> 4. */
#define RMR_PILEUP_BINS 513                          /* 512 x the winning probability of a call: 0 .. 512 */
#define RMR_PILEUP_MAX_CONTIGS ((int64_t)1 << 24)
#define RMR_PILEUP_MAX_POS ((int64_t)1 << 31)       /* positions lie below it */
/* The reference genome on the device (GPU), for the motif test and the strand fold of the emit below.
 * Form: one nibble per base, two bases per byte, low nibble first; every contig starts on a byte boundary; sum of
 * ceil(len / 2) bytes (1.55 GB for a human genome) plus 16 bytes per contig.  A code is the IUPAC set of the letter as a mask:
 * A 1, C 2, G 4, T / U 8, an ambiguity letter the union of its bases, N 15; lower case as upper case; 0 is no letter.  The
 * complement of a code is its four bits reversed.
 * rmr_ref_genome_create: allocates the table for n_contigs contigs of lens[c] bases (HOST array; 0: a contig that is not
 * loaded, on which nothing matches) and zeroes it; *device_bytes (nullable) gets the bytes it holds.
 * rmr_ref_genome_load: fills contig `contig` from `text` (HOST pointer), the text_bytes bytes of its sequence lines as they
 * stand in a FASTA file, from the first base to the last, line terminators inside included: lines of line_bases bases, each
 * followed by line_width - line_bases terminator bytes ("\n": 1, "\r\n": 2), the last line possibly shorter - the layout
 * `samtools faidx` requires.  The bases the text holds by that layout must be lens[contig].  The text goes to the device in
 * pieces of at most piece_bytes bytes (>= 16; 0: 64 MiB), each an even number of bases from an even base index, one kernel
 * launch per piece: the thread of a packed byte reads its two bases, and the same threads verify every byte of the text - a
 * base byte must be an IUPAC letter, a byte behind a line's last base the terminator.  *bad_offset (nullable) gets -1, or
 * the offset in `text` of the first violation, and the call then fails with RMR_ERR_INVALID naming the 1-based sequence
 * line; the contig's table is not to be used after that.  Synchronous.
 * rmr_ref_genome_read: codes [lo, hi) of a contig, one per byte, to a HOST array.  Synchronous; for tests.
 * rmr_ref_genome_destroy: waits for the engine's stream, then frees the table. */
typedef struct rmr_ref_genome rmr_ref_genome;
int rmr_ref_genome_create(rmr_engine *e, int64_t n_contigs, const int64_t *lens, rmr_ref_genome **out, int64_t *device_bytes);
int rmr_ref_genome_load(rmr_ref_genome *g, int64_t contig, const uint8_t *text, int64_t text_bytes, int64_t line_bases, int64_t line_width,
                        int64_t piece_bytes, int64_t *bad_offset);
int rmr_ref_genome_read(rmr_ref_genome *g, int64_t contig, int64_t lo, int64_t hi, uint8_t *codes);
void rmr_ref_genome_destroy(rmr_ref_genome *g);
/* The emit (GPU; DEVICE pointers only, asynchronous on the engine's stream): the walk of rmr_modbam_site_counts / _fill
 * with another end.  The batch is the same struct; n_refs is the header's contig count and truth_off / truth_pos /
 * truth_label are not read.  Differences to the site join:
 *   - a record is skipped whole with status 3 when ref_id < 0 or flag & 0x4, 6 when flag & 0x900 (secondary, supplementary),
 *     2 when ref_id >= n_refs; an MD tag is not asked for (no status 4); statuses 1, 2 and 5 as there;
 *   - every called base inside M / = / X is kept - when region_ref >= 0, only on that contig at region_lo <= pos < region_hi;
 *   - the call is classified in integers: k_j = 2 ML + 1 for a listed code (the later entry wins), 0 for the other modified
 *     bases, column 0 = 512 - sum; class = the first largest column, kmax = its value.
 * rmr_pileup_emit_counts: counts / status / workspaces as rmr_modbam_site_counts; hist (nullable, u64[RMR_PILEUP_BINS],
 * zeroed by the caller once) gets +1 at kmax for every kept call of every record that ends with status 0.
 * rmr_pileup_emit_fill: one site word per kept call into words[out_off[r] .. out_off[r+1]) (a record's calls in the order
 * of the walk along the original sequence), its code `fail` where kmax < k_t (0 .. RMR_PILEUP_BINS).
 * Both take the same rmr_pileup_emit_opts (HOST struct, read before the call returns): the region, and three modes.
 * ref != NULL: a call is kept only where the reference shows a motif around it.
 * A motif: len bases (1 .. RMR_PILEUP_MAX_MOTIF_LEN), the called base at index focus; mask = len nibbles of IUPAC codes, base
 * i in bits 4 i .. 4 i + 3; rc_mask = its reverse complement, nibble i = the 4 bits of nibble len - 1 - i of mask reversed.
 * A reference code r matches a nibble m iff r != 0 and (r & ~m) == 0 - everything the reference allows, the motif allows; a
 * reference N matches only a motif N.  A call at position rp of a '+' record matches when ref[rp - focus + i] matches nibble
 * i of mask for every i, of a '-' record when ref[rp - (len - 1 - focus) + i] matches nibble i of rc_mask; a window that
 * leaves the contig does not match.  The call is kept iff a motif matches; the first that does, in array order, is its motif.
 * combine != 0 (every motif must then be its own reverse complement, mask == rc_mask): a kept '-' call is written on '+' at
 * rp - (len - 1 - 2 focus) of its motif - the focus of the same window read on '+' - and the table has one row per motif site.
 * The region is asked of the position that is written.  The histogram and the counts see kept calls only.  The genome must
 * hold the batch's n_refs contigs and belong to the same engine; refused before any launch otherwise, and for a motif outside
 * the bounds above or an rc_mask that is not mask's reverse complement.
 * duplex != 0 (`infer duplex_from_pod5_and_bam` writes a `C+m?` part from the template read and a `G-m?` part from the
 * complement read into one record): an entry counts when its strand is '+' or '-', it has no ChEBI code and a code of it is
 * among mod_codes (status 5 is asked of the entries of both strands).  The call of a '-' entry lies on the reference strand
 * opposite to its record's: the effective strand, rev XOR (entry strand == '-'), goes into the site word, picks mask or rc_mask
 * and the window start of the motif test, and is what combine folds.  A position that entries of both strands list: the strand
 * of the last entry in tag order that lists it with a code of mod_codes decides, and what entries of the other strand gave the
 * position is dropped; within one strand the later entry wins.
 * hemi != 0 (the fill; the count pass checks it and counts the same calls): a '-' call is written at the '+' position of its
 * window, as combine does, but KEEPS its strand bit - the '+' call at rp and the '-' call at rp + (len - 1 - 2 focus) of one
 * record then differ in bit 4 and the code alone, which is what the pair passes below look for.  Refused before any launch
 * with hemi: duplex == 0, a NULL ref, combine == 0, n_motifs != 1 (and, by combine, a motif that is not its own reverse
 * complement).  n_records 0 launches nothing. */
#define RMR_PILEUP_MAX_MOTIFS 4
#define RMR_PILEUP_MAX_MOTIF_LEN 16
typedef struct rmr_pileup_motif {
    int32_t len, focus;
    uint64_t mask, rc_mask;
} rmr_pileup_motif;
typedef struct rmr_pileup_ref {
    const rmr_ref_genome *genome;
    int32_t n_motifs, combine;
    rmr_pileup_motif motifs[RMR_PILEUP_MAX_MOTIFS];
} rmr_pileup_ref;
typedef struct rmr_pileup_emit_opts {
    int32_t region_ref;                 /* < 0: everywhere */
    int64_t region_lo, region_hi;
    const rmr_pileup_ref *ref;          /* NULL: no motif test, no fold */
    int32_t duplex;                     /* '-'-strand entries count too */
    int32_t hemi;                       /* needs duplex, ref, combine, exactly one motif */
} rmr_pileup_emit_opts;
int rmr_pileup_emit_counts(rmr_engine *e, const rmr_modbam_batch *b, const rmr_pileup_emit_opts *opt, int32_t *ords, int64_t *cig_q,
                           int64_t *cig_r, int64_t *counts, int32_t *status, uint64_t *hist);
int rmr_pileup_emit_fill(rmr_engine *e, const rmr_modbam_batch *b, const rmr_pileup_emit_opts *opt, int32_t k_t, const int32_t *ords,
                         const int64_t *cig_q, const int64_t *cig_r, const int32_t *status, const int64_t *out_off, uint64_t *words);
/* The per-site table (GPU).  rmr_pileup_create: a table for n_contigs contigs, the longest of max_contig_len bases, with
 * n_alpha classes (the canonical base and 1 .. 7 modified ones; a row has n_alpha + 1 u32 counts, the last is `fail`) and a
 * call buffer of buffer_calls words (below 2^31).  Refused before anything is allocated or launched: n_contigs outside 1 ..
 * RMR_PILEUP_MAX_CONTIGS, max_contig_len above RMR_PILEUP_MAX_POS.  Device memory: about 52 + 4 (n_alpha + 1) bytes per word
 * of the buffer plus rocPRIM's scratch, allocated here, and 8 + 4 (n_alpha + 1) bytes per distinct site (twice that while
 * a merge copies the table).
 * rmr_pileup_add: n site words (DEVICE pointer; read before the call returns or in stream order before anything the caller
 * issues on the engine's stream afterwards) are appended to the buffer; whenever it is full it is flushed - one radix sort
 * over the used bits, one count per (site, code) run by binary search, rows merged into the resident table of ascending
 * unique site keys.  The table does not depend on how the words were cut into calls or flushes.
 * rmr_pileup_finish: flushes what the buffer holds and reports the distinct sites, the words added, the flushes so far and
 * the peak of the device memory held; RMR_ERR_INVALID naming the site if a count would have passed 2^32 - 1.  Words may be
 * added again afterwards.
 * rmr_pileup_read: after rmr_pileup_finish, the table to HOST arrays keys u64[n_sites] (ascending) and counts
 * u32[n_sites][n_alpha + 1].  Synchronous.
 * rmr_pileup_destroy: waits for the engine's stream, then frees the buffer and the table. */
typedef struct rmr_pileup rmr_pileup;
int rmr_pileup_create(rmr_engine *e, int64_t n_contigs, int64_t max_contig_len, int n_alpha, int64_t buffer_calls, rmr_pileup **out);
int rmr_pileup_add(rmr_pileup *p, const uint64_t *words, int64_t n);
int rmr_pileup_finish(rmr_pileup *p, int64_t *n_sites, int64_t *n_calls, int64_t *n_flushes, int64_t *peak_device_bytes);
int rmr_pileup_read(rmr_pileup *p, uint64_t *keys, uint32_t *counts);
void rmr_pileup_destroy(rmr_pileup *p);
/* A partition field above the contig index (GPU; DEVICE pointers, asynchronous on the engine's stream), for per-haplotype
 * tables.  rmr_pileup_stamp_partition: between rmr_pileup_emit_fill and rmr_pileup_add,
 *     words[i] |= (uint64_t)part[r] << shift     for out_off[r] <= i < out_off[r + 1],   r = 0 .. n_records - 1,
 * with shift = 36 + the bits the contig index takes; a pileup created for n_contigs << (bits of the field) contigs then sorts
 * and counts the partitions apart, and the ref_id of a key it returns is part << (shift - 36) | ref_id.  part: i32[n_records],
 * 0 <= part[r] < 2^(60 - shift) (the caller's to keep); a record with part 0 or without words writes nothing.  out_off as
 * rmr_pileup_emit_fill took it; the n_words of `words` bound every store.  n_records 0 launches nothing.  Refused before
 * the launch: n_records or n_words negative, a shift outside 36 .. 59, NULL pointers. */
int rmr_pileup_stamp_partition(rmr_engine *e, int64_t n_records, const int64_t *out_off, const int32_t *part, int shift, uint64_t *words,
                               int64_t n_words);
/* The strand pairs of a hemi emit (GPU; DEVICE pointers, asynchronous on the engine's stream).
 * rmr_pileup_pair_counts / rmr_pileup_pair_fill: the two strands' calls of one record at one site -> one pair word.  words /
 * out_off as the hemi fill wrote and took them: a record's words stand in walk order, their positions are monotone, so the
 * partner of a '+' word (bit 4 clear) is the first word, in index order, among the RMR_PILEUP_MAX_MOTIF_LEN - 1 words before
 * and behind it IN ITS RECORD'S SLICE [out_off[r], out_off[r + 1]) with an equal word >> 5 and bit 4 set.  pairs[r] (i64
 * [n_records]) gets the pairs of record r; with pair_off their exclusive prefix sum (n_records + 1 entries, the caller's), the
 * fill writes pair_words[pair_off[r] .. pair_off[r + 1]) in the order of the '+' words:
 *     pair word = the '+' word with code a * n_codes + b,   a / b = the code of the '+' / '-' word (at most n_codes - 1),
 * n_codes = n_mods + 2, so that a table created with rmr_pileup_create_cols(n_codes^2) counts the patterns per site.  Words of
 * different records are never paired; a word without a partner is in no pair word.  n_words and the record's slice bound
 * every load and store.  n_records 0 launches nothing.  Refused before the launch: negative sizes, NULL pointers, n_codes
 * outside 3 .. 4.
 * rmr_pileup_create_cols: rmr_pileup_create for rows of ncol u32 counts, 3 .. 16 (a word's code must lie below ncol; the
 * device memory is that of n_alpha = ncol - 1). */
int rmr_pileup_pair_counts(rmr_engine *e, int64_t n_records, const int64_t *out_off, const uint64_t *words, int64_t n_words, int64_t *pairs);
int rmr_pileup_pair_fill(rmr_engine *e, int64_t n_records, const int64_t *out_off, const uint64_t *words, int64_t n_words, int n_codes,
                         const int64_t *pair_off, uint64_t *pair_words);
int rmr_pileup_create_cols(rmr_engine *e, int64_t n_contigs, int64_t max_contig_len, int ncol, int64_t buffer_calls, rmr_pileup **out);
/* The coverage join (GPU): per site of the finished table, how many records cover it WITHOUT a call - the N_delete, N_diff and
 * N_nocall columns of the eighteen-column bedMethyl.  replaces: nothing in the reference; these are this project's own
 * definitions (the column order of the files is modkit's).
 * A record takes part iff its status is 0.  It is asked about every site of the table on its contig, on its strand (bit 0 of
 * the key = flag & 0x10), in its partition (part[r] above the contig index, as rmr_pileup_stamp_partition puts it; part NULL:
 * none) whose position rp lies in its reference span [pos, pos + the reference length of its CIGAR).  The first rule that fits:
 *   1. one of the record's own words, words[out_off[r] .. out_off[r + 1]) - passing or `fail` - has the site's key: nothing;
 *   2. rp lies inside a D operation: delete += 1;
 *   3. rp lies inside M / = / X: the base of the original read there (the stored base, complemented for flag & 0x10; U as T)
 *      equals the canonical base: nocall += 1; anything else, N included: diff += 1;
 *   4. otherwise (an N skip): nothing.
 * ref with ref->combine != 0 (the table of a combined emit: one row per motif site, strand bit 0): a '+' record is asked at rp =
 * S of a site S, a '-' record at rp = S + (len - 1 - 2 focus) of the first motif, in array order, whose window matches the
 * reference on '+' with its focus at S; a site no motif matches at, or an rp outside the span, adds nothing.  ref NULL or
 * combine == 0: ref is not read.
 * rmr_pileup_set_canonical: the canonical base of the table, 'A' 'C' 'G' 'T' or 'U' (= 'T'); the join is refused without it.
 * rmr_pileup_cover: DEVICE pointers, asynchronous on the engine's stream.  b, status, cig_q, cig_r, out_off and words are those
 * of the rmr_pileup_emit_counts / _fill of the same batch, the words stamped already when part is given (shift as
 * there; ignored without part); words may be NULL when n_words is 0.  One workgroup of 256 threads per record: two binary
 * searches in the table's keys bracket its sites, each lane finds the CIGAR operation of its rp - the LAST index with
 * cig_r <= rp - pos, since operations that consume no reference share their cig_r with the next one -, takes the stored
 * position from cig_q, searches the record's slice of words (monotone in position) for the key and does one integer atomicAdd.
 * Every load is bounded by the record's slices, n_words and n_sites; the result does not depend on the order or the batches.
 * Each record adds at most 1 per site and column: the caller refuses 2^32 records.  The counts live in a u32[n_sites][3] array
 * beside the table (12 bytes per site, in the peak rmr_pileup_finish reports from then on), allocated and zeroed by the first
 * call after rmr_pileup_finish and dropped when rmr_pileup_add is called again.  Refused before any launch: before
 * rmr_pileup_finish, without a canonical base, NULL pointers, bad sizes, a ref the emit would refuse.  n_records 0 or a table
 * without a site: nothing is launched or stored.
 * rmr_pileup_read_cover: cover u32[n_sites][3] (HOST; delete, diff, nocall per site in the order of rmr_pileup_read's keys);
 * all zero when no record was joined since the table last changed.  Synchronous. */
int rmr_pileup_set_canonical(rmr_pileup *p, int base);
int rmr_pileup_cover(rmr_pileup *p, const rmr_modbam_batch *b, const rmr_pileup_ref *ref, const int32_t *status, const int64_t *cig_q,
                     const int64_t *cig_r, const int64_t *out_off, const uint64_t *words, int64_t n_words, const int32_t *part, int shift);
int rmr_pileup_read_cover(rmr_pileup *p, uint32_t *cover);

/* The simplex-to-duplex alignment of duplex calling (GPU; HOST pointers, synchronous).
 * replaces: duplex_utils.parasail_align + trim_parasail_alignment, src/remora/duplex_utils.py:22-115, i.e.
 * parasail.sg_qx_trace_scan_32(simplex, duplex, 10, 2, dnafull) and the stripping of the gap operations at both ends, for a
 * batch of alignments.  Semi-global affine-gap alignment, exact (unbanded): the query (simplex) has free ends, the ref (duplex)
 * is consumed whole; H[i][0] = 0, H[0][j] = -(OPEN + EXTEND (j - 1)), the result is max_i H[i][m].  The scores are the block
 * below (a gap of k bases costs OPEN + EXTEND (k - 1)).  Among co-optimal paths ("Duplex"): the end row is the
 * smallest i with H[i][m] maximal; walking back, H prefers the diagonal, then the deletion state (consumes the duplex), then
 * the insertion state (consumes the simplex); a gap state returns to H as soon as the scores allow. */
#define RMR_DUPLEX_MATCH 5
#define RMR_DUPLEX_MISMATCH (-4)
#define RMR_DUPLEX_N_BASE (-2)   /* N against A / C / G / T */
#define RMR_DUPLEX_N_N (-1)
#define RMR_DUPLEX_GAP_OPEN 10
#define RMR_DUPLEX_GAP_EXTEND 2
#define RMR_DUPLEX_ROWS_PER_LANE 8
#define RMR_DUPLEX_STRIP_ROWS 512   /* 64 lanes of RMR_DUPLEX_ROWS_PER_LANE simplex rows: the strip height of the kernel */
#define RMR_DUPLEX_DEFAULT_TRACE_BYTES ((int64_t)1 << 34) /* 16 GiB */
/* per-alignment status (out field 0) */
#define RMR_DUPLEX_OK 0
#define RMR_DUPLEX_NO_MATCH 1      /* no match operation on the path */
#define RMR_DUPLEX_BAD_BASE 2      /* a letter other than A C G T N (upper case) */
#define RMR_DUPLEX_OVER_BUDGET 3   /* its own trace (checkpointed: its lines and one strip of trace) is larger than trace_budget */
#define RMR_DUPLEX_EMPTY 4         /* an empty sequence */
#define RMR_DUPLEX_OUT_FIELDS 8
/* Alignment a: query bases[q_off[a] .. + q_len[a]), ref bases[r_off[a] .. + r_len[a]) (ASCII).  The trace of an alignment takes
 * ceil(q_len / STRIP_ROWS) * (r_len + 63) * 256 bytes (4 bits per cell).  The alignments are sorted by that size and run in as
 * many groups as trace_budget bytes need (<= 0: RMR_DUPLEX_DEFAULT_TRACE_BYTES); one group's traces are allocated for the call
 * and freed before it returns.  The grouping changes no result.  *n_groups (may be NULL) receives the number of groups.
 * out i32[n][RMR_DUPLEX_OUT_FIELDS]: status, score, end row, query_start, ref_start, ref_end, number of runs, 0; everything
 * after the status is 0 unless the status is RMR_DUPLEX_OK.  The path between (query_start, ref_start) and the end, gap runs at
 * both ends stripped, is written as BAM CIGAR words (length << 4 | op; M = 0 with = and X folded, I = 1, D = 2) to
 * runs[run_off[a] ..]: the caller provides run_off i64[n + 1] with room for at least 2 r_len + 2 words per alignment (the most
 * a path can have). */
int rmr_duplex_align(rmr_engine *e, int64_t n, const uint8_t *bases, const int64_t *q_off, const int64_t *q_len, const int64_t *r_off,
                     const int64_t *r_len, int64_t trace_budget, int32_t *out, const int64_t *run_off, uint32_t *runs,
                     int64_t *n_groups);

/* rmr_duplex_align with a choice of the memory the walk back is made from.  The alignments, their scores, the rule among
 * co-optimal paths and every output are those of rmr_duplex_align in every mode, bit for bit.
 *   RMR_DUPLEX_MODE_FULL        the 4-bit trace of every cell is stored: rmr_duplex_align itself (which is this call).
 *   RMR_DUPLEX_MODE_CHECKPOINT  the forward pass keeps the DP line (r_len (H, F) pairs) above every strip of STRIP_ROWS query rows
 *                               and no trace; the walk back recomputes the trace of one strip at a time, from the strip of the
 *                               end row down, and only the columns at or left of where the walk stands.  An alignment takes
 *                               ceil(q_len / STRIP_ROWS) * r_len * 8 + (r_len + 63) * 256 bytes (about 1/20 of its trace at 25 kb)
 *                               and each cell is computed at most twice.  RMR_DUPLEX_OVER_BUDGET is given only to an alignment
 *                               whose own checkpointed footprint exceeds trace_budget; the rest is sorted by footprint and
 *                               grouped under the budget as the traces are, allocated for the call and freed before it returns.
 *   RMR_DUPLEX_MODE_AUTO        FULL where no live alignment is over the budget with its trace and all traces fit it together
 *                               (one group); otherwise the whole call runs CHECKPOINT.
 * *n_checkpointed (may be NULL) receives the number of alignments that ran checkpointed (0 in FULL). */
#define RMR_DUPLEX_MODE_FULL 0
#define RMR_DUPLEX_MODE_CHECKPOINT 1
#define RMR_DUPLEX_MODE_AUTO 2
int rmr_duplex_align_mode(rmr_engine *e, int64_t n, const uint8_t *bases, const int64_t *q_off, const int64_t *q_len, const int64_t *r_off,
                          const int64_t *r_len, int64_t trace_budget, int mode, int32_t *out, const int64_t *run_off, uint32_t *runs,
                          int64_t *n_groups, int64_t *n_checkpointed);

/* ---- the read-id index of a POD5 dataset (GPU; HOST pointers, synchronous) ---------------------------------------------- */
/* replaces: the read-id lookup of pod5.DatasetReader, which the reference opens every POD5 argument with - a file or a
 * directory of files: src/remora/io.py:427 (iter_signal), src/remora/inference.py:481, src/remora/prepare_train_data.py:153,
 * src/remora/parsers.py:2109 and src/remora/io.py:2554 (duplex).  The ids of all files of a run are one table on the device.
 * keys u8[n][16]: the read ids as the POD5 reads table stores them (fixed-size binary, the bytes of the UUID in text order);
 * values i64[n]: what an id resolves to (io.Pod5Dataset: the global row of the read).  The pairs are sorted by key on the
 * device (two stable 64-bit radix sorts) and every entry whose key equals its predecessor's is dropped: of equal ids the one
 * given FIRST stays.  *n_distinct (may be NULL) receives the size of the table, which stays resident at 24 bytes per distinct
 * id until rmr_read_index_destroy; the build takes about 80 n bytes more, freed before the call returns.  n = 0 is a valid,
 * empty index.  n > 2^31 - 1, or device memory that cannot be had, is RMR_ERR_INVALID / RMR_ERR_NOMEM with a message that names
 * the bytes needed.  The index belongs to `e` (its device, its stream, its mutex) and must be destroyed before it. */
typedef struct rmr_read_index rmr_read_index;
int rmr_read_index_create(rmr_engine *e, const uint8_t *keys, const int64_t *values, int64_t n, rmr_read_index **out,
                          int64_t *n_distinct);
/* replaces: DatasetReader.get_read / `read_id in ...` for a batch of BAM records (src/remora/io.py:427-441,
 * src/remora/inference.py:481-519).  Name i is the text names[name_off[i] .. name_off[i+1]) (name_off i64[m+1], ascending; no
 * terminators); values_out[i] receives the value of its id, or -1.  A name is an id only as the canonical 36-character
 * 8-4-4-4-12 hexadecimal text, in either letter case; anything else (another length, another character, a hyphen elsewhere,
 * the empty name) gives -1 and is never an error.  One launch, one thread per name; m = 0 launches nothing. */
int rmr_read_index_lookup(rmr_read_index *index, const char *names, const int64_t *name_off, int64_t m, int64_t *values_out);
/* replaces: DatasetReader.close (src/remora/io.py:441). */
void rmr_read_index_destroy(rmr_read_index *index);

/* The signal coordinate of every reference position of one alignment (host code).
 * replaces: compute_ref_to_signal = map_ref_to_signal(make_sequence_coordinate_mapping(cigar)), src/remora/data_chunks.py:60-122
 * (called from io.Read.add_alignment, src/remora/io.py:2070-2080), with np.interp's float64 arithmetic: the same integers.
 * cigar u32[n_ops] as stored in a BAM record (length << 4 | op), taken back to front when `reverse` (a reverse-strand
 * record: the read-oriented CIGAR); query_to_signal i64[n_knots] (the expanded move table, seq_len + 1 entries).
 * ref_to_signal receives *n_out = reference length + 1 entries (RMR_ERR_INVALID and *n_out set when cap is smaller).
 * Errors (RMR_ERR_INVALID, the reference's texts): "Invalid cigar op(s)", "No match operations found in alignment cigar". */
int rmr_ref_to_signal(const uint32_t *cigar, int64_t n_ops, int reverse, const int64_t *query_to_signal, int64_t n_knots,
                      int64_t *ref_to_signal, int64_t cap, int64_t *n_out);
/* The reference-anchored half of a BAM batch's ingest, per record on native threads: io.parse_move_tag
 * (src/remora/io.py:394-407: mv -> query_to_signal, with its two checks) followed by compute_ref_to_signal
 * (src/remora/data_chunks.py:118-122) as Read.add_alignment composes them (io.py:2066-2084).  Record i: move table
 * mv[mv_off[i] .. mv_off[i+1]) (first entry = stride), trimmed signal length sig_len[i], seq_len[i] bases, CIGAR words
 * cigar[cigar_off[i] .. cigar_off[i+1]) in BAM order (reverse[i]: walked backwards, the read's orientation), ref_len[i]
 * reference bases (< 0: no reference sequence - status 9 once its move table has passed the checks).  Its ref_to_signal goes
 * to r2s[r2s_off[i] .. +ref_len[i]+1).
 * status[i]: 0 done; RMR_ERR_INVALID (empty table / stride <= 0), RMR_ERR_DISCORDANT_SEQ, RMR_ERR_DISCORDANT_SIG as
 * rmr_parse_moves_batch; 1 "Discordant ref seq lengths" (io.py:2078-2079); 2 "Invalid cigar op(s)"; 3 "No match operations
 * found in alignment cigar"; 4 a CIGAR with an empty match run; 8 no move table; 9 no reference sequence. */
int rmr_ref_anchor_batch(int64_t n, const int8_t *mv, const int64_t *mv_off, const int64_t *sig_len, const int64_t *seq_len,
                         const uint32_t *cigar, const int64_t *cigar_off, const uint8_t *reverse, const int64_t *ref_len,
                         int64_t *r2s, const int64_t *r2s_off, int32_t *status, int threads);
/* The same for signal recorded 3'->5' (`reverse_signal` models).  replaces: the reverse_signal branch of io.parse_move_tag
 * (src/remora/io.py:401-402: query_to_signal = sig_len - query_to_signal[::-1], after the two checks) inside the composition
 * above - with reverse_signal != 0 the CIGAR walk interpolates in those reversed coordinates, exactly as Read.add_alignment +
 * compute_ref_to_signal do for a read built with reverse_signal=True.  Same arguments otherwise, same status codes;
 * reverse_signal == 0 IS rmr_ref_anchor_batch, which forwards here.  (`reverse` is the strand of the alignment, per record;
 * `reverse_signal` the direction of the signal, per call.) */
int rmr_ref_anchor_batch_dir(int64_t n, const int8_t *mv, const int64_t *mv_off, const int64_t *sig_len, const int64_t *seq_len,
                             const uint32_t *cigar, const int64_t *cigar_off, const uint8_t *reverse, const int64_t *ref_len,
                             int64_t *r2s, const int64_t *r2s_off, int32_t *status, int reverse_signal, int threads);

/* The native BAM reader's own inflater for BGZF members, alone (host code; replaces zlib's inflate under
 * rmr_bam_read_batch, which itself stands in for htslib below pysam, src/remora/io.py:184-358): a raw RFC 1951 stream
 * src[0..n) into exactly out[0..out_len); RMR_ERR_INVALID when the stream is malformed, ends elsewhere or does not fill
 * the output exactly.  Inside the reader every member's CRC32 is checked and zlib takes what this decoder refuses. */
int rmr_inflate_raw(const uint8_t *src, int64_t n, uint8_t *out, int64_t out_len);

/* ---- N3: BGZF members for the output BAM (host code) ------------------------------------------------ */
/* replaces: the deflate step of pysam / htslib below AlignmentFile.write (src/remora/inference.py:619-623), for the
 * writer's fast mode (`--bam-level 1`).  src[0..n) is cut into payloads of 0xFF00 bytes (the last one shorter); each
 * becomes one BGZF member (gzip + BC extra field, SAM spec 4.1) whose deflate stream is a single dynamic-Huffman block
 * over the literals - no LZ77 matches - or a stored block when that would not shrink it; CRC32 and ISIZE as gzip wants
 * them.  Members are written to `out` back to back (out_cap >= 65311 bytes per payload), *out_len = their total size;
 * `n_threads` payloads are coded side by side.  No end-of-file marker is appended. */
int rmr_bgzf_huffman(const uint8_t *src, int64_t n, int n_threads, uint8_t *out, int64_t out_cap, int64_t *out_len);

/* ---- N1: POD5 signal rows, the zstd layer (host code, parallel over rows) ----------------------------- */
/* replaces: the zstd step of pod5's signal reader under io.iter_signal (src/remora/io.py:441-474).  `src[i]`
 * points at row i's compressed bytes (one zstd frame, src_len[i] bytes).  rmr_zstd_frame_sizes reads the
 * decompressed size of every frame from its header; rmr_zstd_rows inflates row i into out[out_off[i] ..
 * out_off[i+1]) (that span must equal the frame's content size) with `n_threads` threads.  libzstd.so.1 is
 * loaded from the system at run time. */
int rmr_zstd_frame_sizes(const uint8_t *const *src, const int64_t *src_len, int64_t n_rows, int64_t *sizes);
int rmr_zstd_rows(const uint8_t *const *src, const int64_t *src_len, int64_t n_rows, uint8_t *out,
                  const int64_t *out_off, int n_threads);

/* ---- N1: POD5 signal decompression (the VBZ layer below zstd) ------------------------------ */
/* replaces: the per-row signal decode that pod5's C++ reader performs for the records consumed by
 * io.iter_signal (src/remora/io.py:441-474) / Read.from_pod5_and_alignment (:2086-2121):
 * streamvbyte16 (ceil(n/8) key bytes, one bit per sample LSB first: 0 = one data byte, 1 = two; then the
 * data bytes) -> zigzag -> running sum in int16.  `svb` holds the zstd-DEcompressed bytes of the rows back to
 * back (row r = svb[row_off[r] : row_off[r+1]]), row_samples[r] its sample count; `out` receives the rows'
 * samples back to back (sum(row_samples) int16).  The delta coding restarts in every row.
 * Reads with RMR_MEM_DEVICE: the kernel fetches each step's data bytes as whole aligned dwords, so it reads up to 3 bytes
 * behind the last row and up to 3 bytes in front of a step's first data byte (for a first row of fewer than 3 key bytes and an `svb` off a dword
 * boundary these lie before `svb`); both reads stay inside the aligned dwords that hold valid
 * bytes, and what they return beyond the row is never used.  `svb` may have any alignment; remora_amd/io.py leaves 16 bytes
 * of slack behind the last row.  With RMR_MEM_HOST the library stages `svb` itself and the caller's buffer is read as given.
 * `out` may have any int16 alignment (16-byte aligned spans are stored as vectors); nothing outside a row's own span of
 * `out` is written.  After an error the contents of `out` are unspecified within the rows' spans: rows other than the
 * refused one may be decoded, and a row refused for bytes left over, or at a later step, is stored up to that point.
 * Errors: RMR_ERR_INVALID "corrupt VBZ signal block (row r)", r the first such row, when a row's byte count disagrees with
 * its keys (a row without samples has no bytes), row_samples[r] < 0 or row_off decreases. */
int rmr_vbz_decode(rmr_engine *e, const uint8_t *svb, const int64_t *row_off, const int32_t *row_samples,
                   int64_t n_rows, int16_t *out, int mem);

/* ---- M3: motif scan ---------------------------------------------------------------------- */
/* replaces: Motif.findall (src/remora/util.py:281-297) + find_focus_bases_in_int_sequence (:413-426) as
 * called by RemoraRead.set_motif_focus_bases (src/remora/data_chunks.py:310-317), for a batch of reads:
 * flags[b] = 1 iff base b (index into the concatenated int_seq) is the focus base of a hit of any motif
 * that lies entirely inside its read.  mask[m][j] has bit k set when base k (0..3 = ACGT) is allowed at
 * motif position j; N bases (-1) never match.  The positions come out in ascending order once the
 * flags are compacted (the reference's python-set order is a property of the single-read host API). */
typedef struct {
    int32_t n_motifs;            /* <= 8 */
    int32_t len[8];              /* <= 16 */
    int32_t focus_pos[8];        /* may be negative after leading-N stripping (util.py:208-214) */
    uint8_t mask[8][16];
} rmr_motif_set;
int rmr_motif_flags(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads,
                    const rmr_motif_set *motifs, uint8_t *flags, int mem);
/* The same scan for a batch of device-resident reads without the flag array (DEVICE pointers only): pass 1 counts the
 * hits of every read (counts i64[n_reads]); the caller turns them into offsets foc_off i64[n_reads+1] (exclusive
 * prefix sum) and sizes `focus`; pass 2 writes the read-local focus positions of read r, ascending, at
 * focus[foc_off[r] .. foc_off[r+1]).  One wavefront per read, ballot + prefix-popcount compaction. */
int rmr_motif_focus_counts(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads,
                           const rmr_motif_set *motifs, int64_t *counts);
int rmr_motif_focus_fill(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads,
                         const rmr_motif_set *motifs, const int64_t *foc_off, int64_t *focus);

/* Host-side gather of a batch of reads into the concatenated rmr_reads layout (no GPU involved; native threads): read i
 * contributes sig_n[i] int16 dacs, seq_n[i]+1 int64 mapping entries and seq_n[i] bases (integers of seq_itemsize[i]
 * bytes, narrowed to int8).  dst_* are caller buffers (typically the pinned staging buffer that is uploaded next);
 * sig_off / seq_off i64[n_reads+1] receive the offsets; the mapping of read i starts at dst_maps[seq_off[i] + i].
 * replaces: nothing in the reference (it handles one read at a time, src/remora/inference.py:62-137). */
int rmr_pack_reads(int64_t n_reads, const void *const *dacs, const int64_t *sig_n, const void *const *maps,
                   const void *const *seqs, const int64_t *seq_n, const int32_t *seq_itemsize, int16_t *dst_dacs,
                   int64_t *dst_maps, int8_t *dst_seq, int64_t *sig_off, int64_t *seq_off, int threads);
/* The same gather with the mapping narrowed to int32 (dst_maps32, same offsets) - a seventh less to carry across PCIe; the
 * caller widens it on the device.  *maps_fit = 0 when some mapping value does not fit int32 (the buffer's mapping is then
 * not usable: gather again with rmr_pack_reads). */
int rmr_pack_reads_narrow(int64_t n_reads, const void *const *dacs, const int64_t *sig_n, const void *const *maps,
                          const void *const *seqs, const int64_t *seq_n, const int32_t *seq_itemsize, int16_t *dst_dacs,
                          int32_t *dst_maps32, int8_t *dst_seq, int64_t *sig_off, int64_t *seq_off, int threads, int *maps_fit);

/* The bases of selected records of a BAM batch in read orientation, back to back, with their integer codes (host code, native
 * threads).  Record i: src[start[i] .. start[i] + len[i]); `upper` != 0 folds ASCII lower case first; rev[i] != 0: reversed and
 * mapped through comp[256]; codes[j] = code[256] of the oriented byte; fwd (NULL allowed): the folded bases un-reversed.  Output
 * offset of record i = len[0] + ... + len[i-1] in all three.
 * replaces: per read, revcomp(query_sequence) / revcomp(ref_seq) in io.Read.add_alignment (src/remora/io.py:2023, :2058-2060)
 * and util.seq_to_int (src/remora/util.py:131-142). */
int rmr_orient_bases(const uint8_t *src, const int64_t *start, const int64_t *len, const uint8_t *rev, int64_t n, int upper,
                     const uint8_t *comp, const int8_t *code, uint8_t *fwd, uint8_t *oriented, int8_t *codes, int threads);


/* ---- X1 + X2 + X3 (+X6): chunk extraction for a batch of reads --------------------------- */
/* replaces: RemoraRead.sig (src/remora/data_chunks.py:191-197), iter_chunks (:425-466),
 * extract_chunk (:331-423) and the row packing of CoreRemoraDataset.write_chunk
 * (:1376-1418).  Reads are concatenated; read r owns dacs[sig_off[r]:sig_off[r+1]],
 * int_seq[seq_off[r]:seq_off[r+1]], seq_to_sig_map[seq_off[r]+r : seq_off[r+1]+r+1]
 * (one more entry than bases) and focus_bases[focus_off[r]:focus_off[r+1]] (read-local
 * base indices, in the order the caller wants the chunks).
 *
 * Step 1 normalises the signal and computes the geometry of every chunk:
 *   sig_out      f32[sig_off[n_reads]]            ((dacs - shift)/scale in f64, cast to f32)
 *   geo          i64[n_chunks, 6] = {seq_len, chunk_sig_focus_idx, chunk_focus_base,
 *                                    read_focus_base, seq_start, sig_start(signed, unclipped)}
 *   *max_seq_len max over chunks of seq_len (host int, always written; implies a sync)
 * Step 2 fills the dataset-layout arrays for widths seq_w >= max_seq_len+kb+ka,
 *   map_w >= max_seq_len+1 (padding columns: sequence -1, mapping 0; the reference leaves
 *   them uninitialised). */
typedef struct {
    int64_t n_reads;
    const int16_t *dacs;        /* concatenated */
    const int64_t *sig_off;     /* [n_reads+1] */
    const int64_t *seq_to_sig;  /* concatenated, n_bases+1 per read */
    const int8_t *int_seq;      /* concatenated, values -1..3 */
    const int64_t *seq_off;     /* [n_reads+1] */
    const double *shift;        /* [n_reads] */
    const double *scale;        /* [n_reads] */
    const int64_t *focus_bases; /* concatenated, read-local */
    const int64_t *focus_off;   /* [n_reads+1] */
    int32_t cc_before, cc_after, kb, ka, base_start_justify, offset;
    /* base_start_justify == 2: focus_bases holds SIGNAL indices (the focus_sig_idx argument of RemoraRead.extract_chunk,
     * src/remora/data_chunks.py:331-343) and `offset` is the read_focus_base the chunks report - no clipping, no mapping
     * look-up */
    /* optional (all three or NULL): HOST copies of sig_off / seq_off / focus_off for callers whose arrays are device
     * memory - the library needs the offsets on the host (launch sizes, staging) and otherwise fetches them with three
     * small device-to-host copies per call (about 60 us of a single-read call) */
    const int64_t *host_sig_off, *host_seq_off, *host_focus_off;
} rmr_reads;

int rmr_chunk_geometry(rmr_engine *e, const rmr_reads *reads, float *sig_out, int64_t *geo,
                       int64_t *max_seq_len, int mem);
int rmr_chunk_fill(rmr_engine *e, const rmr_reads *reads, const float *sig, const int64_t *geo,
                   float *signal /* f32[n_chunks, L] */, int8_t *seqs, int seq_w, int16_t *maps,
                   int map_w, int16_t *lens, int64_t *read_focus_bases, int mem);

/* ---- F1 / F2: network forward on materialised inputs ------------------------------------ */
/* replaces: `model(sigs, enc_kmers)` = ConvLSTM_w_ref.network.forward
 * (models/ConvLSTM_w_ref.py:39-58) / Conv_w_ref.network.forward (models/Conv_w_ref.py:44-62)
 * as called from RemoraRead.run_model (src/remora/data_chunks.py:528-533) and
 * run_model_batched (src/remora/inference.py:311-315).  sigs f32[n,1,L]; seqs f32[n,4K,L]
 * (any values, not only one-hot); logits f32[n,num_out]. */
int rmr_forward(rmr_model *m, const float *sigs, const float *seqs, int64_t n, float *logits,
                int mem);

/* ---- fused hot path: chunk arrays -> logits, never materialising the one-hot ------------- */
/* replaces: CoreRemoraDataset.extract_batch -> compute_encoded_kmer_batch
 * (src/remora/data_chunks.py:1652-1676) followed by model(sigs, enc_kmers) — i.e. what
 * RemoraRead.prepare_batches + run_model (:468-540) and prep_nn_input + run_model_batched
 * (src/remora/inference.py:152-168, :277-316) compute between them.
 * label_counts (nullable): i64[num_out], INCREMENTED by the argmax histogram of this call
 * (first maximum wins, as np.argmax in src/remora/validate.py:42-45). */
int rmr_infer_chunks(rmr_model *m, const float *signal, const int8_t *seqs, int seq_w,
                     const int16_t *maps, int map_w, const int16_t *lens, int kb, int ka,
                     int64_t n, float *logits, int64_t *label_counts, int mem);

/* ---- one read, one call ------------------------------------------------------------------- */
/* replaces: what `call_read_mods` does for ONE read between its motif search and its return
 * (src/remora/inference.py:661-712): RemoraRead.prepare_batches -> an in-memory CoreRemoraDataset of the read's chunks
 * (src/remora/data_chunks.py:468-514: sig :191-197, iter_chunks :425-466, extract_chunk :331-423, write_chunk
 * :1376-1418, compute_encoded_kmer_batch) and RemoraRead.run_model (:516-540) - staging, signal normalisation, chunk
 * geometry and rows, and the network in one call with ONE stream synchronisation (the chunk geometry is integer arithmetic on
 * the mapping and is computed on the host while the arrays cross PCIe), no Python in between.
 * All pointers are HOST memory.  focus_bases: read-local base indices in the order the caller wants the chunks (the
 * reference's python-set order is the caller's business); logits f32[n_focus, num_out] and read_focus_bases
 * i64[n_focus] (the focus base after `offset`, clipped into the read, :443-446) are written in that order. */
typedef struct {
    const int16_t *dacs;        /* [n_sig] */
    int64_t n_sig;
    const int64_t *seq_to_sig;  /* [n_bases + 1] */
    const void *int_seq;        /* [n_bases] integers of seq_itemsize bytes (1, 2, 4 or 8), values -1..3 */
    int32_t seq_itemsize, _pad;
    int64_t n_bases;
    double shift, scale;
    const int64_t *focus_bases; /* [n_focus] */
    int64_t n_focus;
    int32_t cc_before, cc_after, kb, ka, base_start_justify, offset;
} rmr_read;
int rmr_call_read(rmr_model *m, const rmr_read *read, float *logits, int64_t *read_focus_bases);

/* argmax histogram of existing logits (same rule), counts[num_out] incremented. */
int rmr_count_labels(rmr_engine *e, const float *logits, int64_t n, int num_out,
                     int64_t *counts, int mem);

/* Validation tally of one batch of logits ON THE DEVICE (every pointer except label_of_column is device memory): what
 * ValidationLogger.run_validation computes on the host per batch and at the end (src/remora/validate.py:208-259) -
 * add_unmodeled_labels (:69-99: the model's num_out columns widened to the dataset's num_labels; label_of_column[c] = the
 * model column of label c, -1 = not modelled -> -1000), util.softmax_axis1 in float32 (util.py:182-186), np.argmax, the
 * confusion counts of compute_metrics (:42-45), CrossEntropyLoss.
 *   confusion i64[num_labels * num_labels] (true x called) and loss_sum f64[1] (sum of the chunks' cross entropies) are
 *   INCREMENTED; win_prob f32[n] (the called class's probability: what the filtered metrics take their quantile of) and
 *   call u8[n] are written.  Asynchronous on the engine's stream. */
int rmr_validation_tally(rmr_engine *e, const float *logits, const int64_t *labels, int64_t n, int num_out, int num_labels,
                         const int32_t *label_of_column, int64_t *confusion, float *win_prob, uint8_t *call, double *loss_sum);

/* ---- (e) multi-GPU: the ONE collective of the path, RCCL over xGMI called from the library ------- */
/* replaces, in distributed form: the per-label tally of a run summed over the workers —
 * validate.compute_metrics' confusion/label tally (src/remora/validate.py:42-45) and get_label_counts
 * (src/remora/data_chunks.py:1074-1082); the reference itself is single-process.  One process per GPU; chunks /
 * reads shard embarrassingly, so this int64[num_out] all-reduce(sum) is the only exchange of a job.
 * Bootstrap as RCCL's own: rank 0 calls rmr_comm_unique_id and hands the 128 bytes to every rank by ANY channel
 * (file, socket, MPI, torch.distributed ...); every rank then calls rmr_comm_init (collective: all ranks must
 * call it) with the same id.  librccl is dlopen'ed on first use: a single-GPU caller never needs it.
 * rmr_allreduce_counts: in place; world 1 (or no communicator) = identity.  RMR_MEM_DEVICE: enqueued on the
 * engine stream (ordered after the kernels that produced the counts; rmr_engine_synchronize to read them on the
 * host); RMR_MEM_HOST: staged through the engine, synchronous. */
#define RMR_COMM_ID_BYTES 128
int rmr_comm_unique_id(uint8_t id[RMR_COMM_ID_BYTES]);
int rmr_comm_init(rmr_engine *e, const uint8_t id[RMR_COMM_ID_BYTES], int rank, int world);
int rmr_comm_destroy(rmr_engine *e);
int rmr_allreduce_counts(rmr_engine *e, int64_t *counts, int n, int mem);

/* ---- N2: signal-mapping refinement (banded dynamic programming) --------------------------- */
/* replaces, for a batch of reads, the body of refine_signal_mapping
 * (src/remora/refine_signal_map.py:780-840) as called by SigMapRefiner.refine_sig_map (:472-497):
 * extract_levels (src/remora/refine_signal_map_core.pyx:87-101), compute_sig_band (.py:631-683),
 * convert_to_seq_band (.py:740-772), adjust_seq_band (core.pyx:31-74), validate_band (.py:686-737),
 * the signal normalisation (dacs - shift) / scale (f64, cast to f32, .py:479), and seq_banded_dp
 * (core.pyx:403-473) with either forward step (Viterbi core.pyx:256-317, dwell penalty :150-253)
 * and the traceback (:119-148).  Scores are float32 with the reference's operation order, so the
 * returned paths equal the reference's. */
enum rmr_refine_algo { RMR_REFINE_VITERBI = 0, RMR_REFINE_DWELL_PENALTY = 1 };
enum rmr_refine_status {   /* per read; > 0 are the RemoraError cases of validate_band */
    RMR_REFINE_OK = 0,
    RMR_REFINE_BAND_START = 1,   /* "Band does not start with 0 coordinate." */
    RMR_REFINE_ZERO_LEN = 2,     /* "Band contains 0-length region" */
    RMR_REFINE_START_ORDER = 3,  /* "Band start positions are not monotonically increasing" */
    RMR_REFINE_END_ORDER = 4,    /* "Band end positions are not monotonically increasing" */
    RMR_REFINE_BAND_END = 5,     /* "Invalid seq_band end coordinate" */
    RMR_REFINE_BAND_LENGTH = 6,  /* "Invalid sig_band length" */
    RMR_REFINE_EMPTY = 7         /* read without bases */
};
typedef struct {
    const float *kmer_levels;   /* host, f32[4^kmer_len], index = sum base_j * 4^(kmer_len-1-j); no NaN */
    int32_t kmer_len, center_idx;
    const float *sd_arr;        /* host, short dwell penalties (SigMapRefiner.sd_arr); dwell_penalty only */
    int32_t sd_len;
    int32_t algo;               /* rmr_refine_algo */
    int32_t half_bandwidth;     /* SigMapRefiner.half_bandwidth */
    int32_t min_step;           /* adjust_band_min_step (2 in the reference) */
} rmr_refine_desc;
typedef struct rmr_refiner rmr_refiner;

int rmr_refiner_create(rmr_engine *e, const rmr_refine_desc *desc, rmr_refiner **out);
void rmr_refiner_destroy(rmr_refiner *r);
const char *rmr_refine_status_message(int status);
/* Reads are concatenated exactly as in rmr_reads (dacs / sig_off / seq_to_sig / int_seq / seq_off /
 * shift / scale).  out_map has the layout of seq_to_sig and receives the refined mapping of every
 * read whose status is 0 (other reads are left untouched); status i32[n_reads]. */
int rmr_refine_signal_maps(rmr_refiner *r, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off,
                           const int64_t *seq_to_sig, const int8_t *int_seq, const int64_t *seq_off,
                           const double *shift, const double *scale, int64_t *out_map, int32_t *status,
                           int mem);
/* The two quantile vectors the rough re-scale fits its line through (SigMapRefiner.rough_rescale,
 * src/remora/refine_signal_map.py:330-420: np.quantile of the normalised centre sample of every base and of the
 * expected k-mer levels, clip_bases dropped at both ends of reads longer than 2 * clip_bases).  Reads laid out as
 * above, DEVICE pointers; quants is a HOST array f64[n_quants] in [0, 1].  sig_q / lvl_q: device f64[n_reads][n_quants],
 * bit-identical to numpy's "linear" quantiles of the float64 / float32 arrays.  status i32[n_reads] (device): 0 ok,
 * 1 = read longer than the in-LDS sort holds (16384 kept bases; max_read_bases, the longest read of the batch or 0
 * if unknown, sizes the sort), 2 = read without bases; rows of such reads are not written. */
int rmr_rescale_quantiles(rmr_refiner *r, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off,
                          const int64_t *seq_to_sig, const int8_t *int_seq, const int64_t *seq_off,
                          const double *shift, const double *scale, int64_t max_read_bases, int clip_bases,
                          int n_quants, const double *quants, double *sig_q, double *lvl_q, int32_t *status);
/* The points the precise re-scale of an iterative refiner (scale_iters > 0) fits its line through: SigMapRefiner.rescale up
 * to its call of rescale_theil_sen (src/remora/refine_signal_map.py:406-469) for every read of a resident batch.  Reads laid
 * out as above, DEVICE pointers, no limit on the read length.  Per read, with dwells = diff(seq_to_sig): dwell_min / dwell_max
 * = np.percentile(dwells, (10, 90)) ("linear": the difference of the two order statistics in int64, numpy's two-sided lerp in
 * float64); base b is kept when dwell_min < dwell < dwell_max, level_ok[b] != 0, its dwell is not 0 and
 * edge_filter_bases <= b < n - edge_filter_bases.  levels f32 / level_ok u8 per base of the concatenated reads: the expected
 * level (extract_levels) and numpy's |level - mean(levels)| > min_abs_level, which no round changes.  live u8[n_reads] or
 * NULL: reads with live == 0 are not touched.  count i32[n_reads]: kept bases; x f64 / y f32, written from the read's seq_off
 * on, in base order: ((double)(sum of the base's samples) / dwell - shift) / scale and the base's level.  Asynchronous on the
 * engine's stream. */
int rmr_rescale_points(rmr_refiner *r, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off,
                       const int64_t *seq_to_sig, const int64_t *seq_off, const double *shift, const double *scale,
                       const float *levels, const uint8_t *level_ok, const uint8_t *live, int edge_filter_bases,
                       int32_t *count, double *x, float *y);
/* theil_sen (src/remora/refine_signal_map.py:83-103) for every live read, one block per read: slope = np.median of
 * (double)(y[i] - y[j]) / (x[i] - x[j]) over the pairs with x[i] - x[j] > 0 (a radix select on the quotients, which are
 * recomputed in every pass and never stored), inter = np.median of (double)y[i] - slope * x[i].  x / y / count / seq_off as
 * rmr_rescale_points leaves them.  A read with count > 1000 (MAX_POINTS_FOR_THEIL_SEN) is fitted through the 1000 points
 * samp[samp_off[read] ..] names (i32 indices into its points, drawn by the host as rescale_theil_sen :106-114 draws them;
 * samp_off i64[n_reads], negative: none; n_samp: the length of samp, which every block of 1000 must lie inside; both NULL and
 * n_samp 0 when no read needs one).  slope / inter f64[n_reads], status i32[n_reads] (rmr_theil_sen_status); reads with live == 0 are not touched.  All DEVICE pointers; asynchronous on the
 * engine's stream. */
enum rmr_theil_sen_status {
    RMR_THEIL_SEN_OK = 0,
    RMR_THEIL_SEN_NO_PAIR = 1,     /* no pair with dx > 0: slope and inter are NaN, as the reference's median of nothing */
    RMR_THEIL_SEN_ZERO_SLOPE = 2,  /* RemoraError("Theil-Sen slope is zero: cannot re-scale"); either sign of zero */
    RMR_THEIL_SEN_BAD_INPUT = 3    /* count outside 0..bases, more than 1000 points without a sample inside samp, index outside the points */
};
int rmr_theil_sen_fit(rmr_refiner *r, int64_t n_reads, const double *x, const float *y, const int32_t *count,
                      const int64_t *seq_off, const int32_t *samp, const int64_t *samp_off, int64_t n_samp,
                      const uint8_t *live, double *slope, double *inter, int32_t *status);

/* ---- P1: per-base signal metrics and the k-mer level table estimated from them ------------ */
/* replaces, for a batch of reads in one launch: metrics.METRIC_FUNCS (src/remora/metrics.py:45-117: compute_dwell,
 * compute_dwell_mean, compute_dwell_mean_sd, compute_trimmean, compute_trimmean_trimsd with clip_sig :7-9) as
 * io.Read.compute_per_base_metric applies them to one read's normalised signal (src/remora/io.py:2394-2480).
 * Reads laid out as in rmr_reads (dacs / sig_off / seq_to_sig / seq_off / shift / scale), DEVICE pointers; max_read_bases: the
 * longest read of the batch (sizes the launch).  Per base b of the concatenated reads (any output may be NULL):
 *   dwell f32    seq_to_sig[b + 1] - seq_to_sig[b]
 *   mean, sd     f64, over the base's samples (dacs - shift) / scale evaluated in float64 as Read.norm_signal does (io.py:1842-1849);
 *                sd = sqrt(max(0, E[x^2] - mean^2)); NaN for a base without samples (the reference's inf becomes NaN too)
 *   trimmean, trimsd   the same over the samples left after dropping start_trim at the base's start and end_trim at its end;
 *                NaN when max(0, dwell - start_trim - end_trim) is 0
 * Every base's samples are summed directly in float64 (error <= dwell * 2^-53 * sum|x|) where the reference takes differences
 * of a whole-read cumulative sum; a base's result does not depend on the other reads of the batch or on the read's place in it.
 * A mapping entry outside the read's own signal gives NaN for the bases it bounds.  Asynchronous on the engine's stream. */
int rmr_base_metrics(rmr_engine *e, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off, const int64_t *seq_to_sig,
                     const int64_t *seq_off, const double *shift, const double *scale, int64_t max_read_bases, int start_trim,
                     int end_trim, float *dwell, double *mean, double *sd, double *trimmean, double *trimsd);
/* replaces, for a list of (read, region) pairs of one resident batch in one launch: io.Read.compute_per_base_metric(metric,
 * region=...) as io.get_ref_reg_sample_metrics stacks it (src/remora/io.py:840-886, :2394-2479) - the metrics of only the bases of
 * a read that lie in a reference region, NaN where the read does not cover the region (:2471-2478), the row reversed for reference
 * orientation on the reverse strand (:879-885).  Reads as in rmr_base_metrics.  pairs i64[n_pairs][8]: read (index into the
 * batch), first, last (bases [first, last) of the read, read-local), lead (region positions in front of the read's first base),
 * row, region length, flip (0 / 1), 0; max_pair_bases >= every last - first (sizes the launch).  Outputs f64[rows][width], any may
 * be NULL (dwell is the float32 value of rmr_base_metrics, widened): base first + i of the pair goes to column lead + i of its row,
 * or, flipped, region length - 1 - (lead + i); every other column of the row is NaN.  The values are the bits rmr_base_metrics
 * gives for the same bases: the 64-base groups of the read that meet [first, last) are summed, counted from the read's first base.
 * A pair is used only if 0 <= first < last <= bases of its read, lead + (last - first) <= region length <= width and 0 <= row <
 * rows; otherwise nothing is written for it and status[pair] = 1 (0: done).  status i32[n_pairs].  Two pairs must not share a
 * row.  All array pointers are DEVICE memory.  Asynchronous on the engine's stream. */
int rmr_region_base_metrics(rmr_engine *e, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off, const int64_t *seq_to_sig,
                            const int64_t *seq_off, const double *shift, const double *scale, int64_t n_pairs, const int64_t *pairs,
                            int64_t max_pair_bases, int start_trim, int end_trim, int64_t rows, int64_t width, double *dwell, double *mean,
                            double *sd, double *trimmean, double *trimsd, int32_t *status);
/* replaces, for the same pairs: Read.extract_ref_reg (src/remora/io.py:2342-2392; the signal of Read.get_sig_type :2294-2308).
 * Per pair, with map = seq_to_sig of its read: the samples [map[first], map[last]) as (dacs - shift[read]) / scale[read] in float64
 * (raw = 0: sig_out is f64; the caller's shift / scale arrays choose "norm", "pa" or "zc_pa") or the int16 samples themselves (raw =
 * 1: sig_out is i16, "dac"), at sig_out[sig_out_off[pair] ..]; the last - first + 1 entries map[first .. last] - map[first] at
 * map_out[map_out_off[pair] ..]; sig_start[pair] = map[first] (read-local).  flip: the samples back to front and the mapping as
 * map[-1] - map[::-1] (:2376-2379).  sig_out_off / map_out_off i64[n_pairs + 1]: the pairs back to back; the caller reads map[first]
 * and map[last] to lay them out, and a pair whose slots are not exactly its sizes, or end beyond sig_capacity / map_capacity
 * (items), or whose read, first or last fail the checks of rmr_region_base_metrics, writes nothing: status[pair] = 1; a mapping that
 * leaves the read's signal there: status 2.  A pair's lead, row and region length are not looked at by this call.  All array pointers
 * are DEVICE memory.  Asynchronous on the engine's stream. */
int rmr_region_signals(rmr_engine *e, int64_t n_reads, const int16_t *dacs, const int64_t *sig_off, const int64_t *seq_to_sig,
                       const int64_t *seq_off, const double *shift, const double *scale, int64_t n_pairs, const int64_t *pairs,
                       const int64_t *sig_out_off, const int64_t *map_out_off, int raw, void *sig_out, int64_t sig_capacity, int64_t *map_out,
                       int64_t map_capacity, int64_t *sig_start, int32_t *status);
/* replaces: io.get_region_kmers (src/remora/io.py:930-982; sequence from get_ref_seq_from_reads :671-703) over every region
 * of io.get_site_kmer_levels (:991-1044) and the median per k-mer of `remora analyze estimate_kmer_levels`
 * (src/remora/parsers.py:2296-2331).  The bases of n_reads reference-anchored reads, concatenated (seq_off i64[n_reads + 1]), are
 * the observations: base i of read r lies on site site0[r] + i - a caller-chosen 64-bit key that encodes contig, strand and the
 * reference position counted in READ orientation, so that the next base of a read is the next site on either strand, and that
 * differs by more than kmer_before + kmer_after between the last site of one contig / strand and the first of another -,
 * carries trimmean[i] (rmr_base_metrics) and int_seq[i] (-1..3, read orientation).  Per site the non-finite values are dropped,
 * at least max(1, min_cov) values are required, and the median (numpy's: the mean of the two middle values of an even count) is
 * the site's level; its k-mer is made of the bases of sites key - kmer_before .. key + kmer_after, each known from any read
 * that covers it, and a window with a site no read covers or a base outside ACGT is skipped.  levels f64[4^k]: the median of
 * the site levels of every k-mer (index = sum base_j * 4^(k-1-j)), NaN for a k-mer without site; kmer_sites i64[4^k] (nullable):
 * how many sites; site_kmer i32 / site_level f64 (nullable, both or none, capacity n_bases): the *n_sites (host) reported sites
 * ordered by (k-mer, level).  k = kmer_before + 1 + kmer_after <= RMR_MAX_LEVEL_KMER.  Sorting and selection run on the device
 * (four radix sorts of 16 bytes per observation; 32 bytes of scratch per observation, plus the sorts' own, are allocated for
 * the call, so n_bases is bounded by device memory: RMR_ERR_HIP when it does not fit).
 * remora_amd.metrics.site_key0 is the key the package uses: sample (8 bits) | contig (20) | strand (1) | position (34).
 * All array pointers are DEVICE memory.  Synchronous. */
#define RMR_MAX_LEVEL_KMER 8
int rmr_site_kmer_levels(rmr_engine *e, int64_t n_reads, const int64_t *seq_off, const int64_t *site0, int64_t n_bases,
                         const double *trimmean, const int8_t *int_seq, int kmer_before, int kmer_after, int64_t min_cov,
                         double *levels, int64_t *kmer_sites, int32_t *site_kmer, double *site_level, int64_t *n_sites);
/* The two stages of rmr_site_kmer_levels as calls of their own, for an input that is aggregated one range of site keys after the
 * other in bounded device memory (remora_amd.metrics.plan_level_ranges cuts the ranges).  The results are those of one
 * rmr_site_kmer_levels call over all observations, bit for bit, however the keys are cut and the k-mers grouped.
 * rmr_site_medians: stage 1 for the range [key_lo, key_hi).  The observations are given as to rmr_site_kmer_levels and must hold
 * every observation of the input with a key in [key_lo - kmer_before, key_hi + kmer_after) (reads clipped to that interval; more
 * does no harm): only sites inside [key_lo, key_hi) are reported, the margins supply their neighbours' bases.  Every reported site
 * is appended as (k-mer index, median) to list_kmer i32 / list_level f64, which hold list_len entries and have room for
 * list_capacity (a range reports at most min(n_bases, key_hi - key_lo) sites; a call that would overrun fails and leaves
 * list_len entries valid), in no particular order; *n_appended (host): how many; site_counts i64[4^k] (zeroed by the caller before
 * the first range) gains the number of appended sites of every k-mer.  32 bytes of scratch per observation, as the one-shot call.
 * rmr_kmer_levels_from_sites: stage 2 over the n_sites accumulated entries and their site_counts.  levels, kmer_sites (nullable),
 * site_kmer / site_level (nullable, both or none, capacity n_sites) as rmr_site_kmer_levels writes them.  max_bytes > 0 bounds the
 * sort buffers (32 bytes per site): consecutive k-mers whose sites fit are sorted together, one group after the other, each group
 * gathered from the lists (*n_groups, host, nullable: how many); a single k-mer whose sites alone exceed it is refused by name.
 * 0: everything in one group.  Slots are handed out with one integer atomic per wave, counts are integer atomics; no float atomics.
 * All array pointers are DEVICE memory.  Synchronous. */
int rmr_site_medians(rmr_engine *e, int64_t n_reads, const int64_t *seq_off, const int64_t *site0, int64_t n_bases, const double *trimmean,
                     const int8_t *int_seq, int kmer_before, int kmer_after, int64_t min_cov, int64_t key_lo, int64_t key_hi,
                     int32_t *list_kmer, double *list_level, int64_t list_len, int64_t list_capacity, int64_t *site_counts,
                     int64_t *n_appended);
int rmr_kmer_levels_from_sites(rmr_engine *e, int64_t n_sites, const int32_t *list_kmer, const double *list_level, int kmer_len,
                               const int64_t *site_counts, int64_t max_bytes, double *levels, int64_t *kmer_sites, int32_t *site_kmer,
                               double *site_level, int64_t *n_groups);

/* ---- training (L5: `remora model train`) ------------------------------------------------------------------------------
 * One fp32 training step of ConvLSTM_w_ref (models/ConvLSTM_w_ref.py:11-58) on the device: the forward pass with BatchNorm
 * in train mode (batch mean and biased variance over (N, L), eps 1e-5; running statistics moved with momentum 0.1 and the
 * unbiased variance), mean cross-entropy over the rows a byte mask keeps, the backward pass and AdamW.  size a multiple of 16
 * from 16 to 256, k-mer length 1..21, chunk length >= 29, num_out 2..16, batch 2..max_batch; Conv_w_ref, the 16-bit dtypes
 * and every other size are refused by name (zero-weight channel padding is no identity under train-mode BatchNorm).
 * The trainer's state is ONE flat fp32 buffer in the order of rmr_model_create's blob (parameters and running statistics),
 * so what rmr_trainer_read returns can be handed to rmr_model_create unchanged; gradients and the two Adam moments are
 * buffers of the same layout (zeros in the running statistics' places).  The same inputs and state give the same bits on
 * every run: every sum over rows is per-block partials plus a second pass in fixed order, no float atomics. */
typedef struct rmr_trainer rmr_trainer;
enum rmr_train_buffer {
    RMR_TRAIN_PARAMS = 0,  /* parameters + running statistics */
    RMR_TRAIN_GRADS = 1,
    RMR_TRAIN_ADAM_M = 2,  /* exp_avg */
    RMR_TRAIN_ADAM_V = 3,  /* exp_avg_sq */
    RMR_TRAIN_COUNTERS = 4 /* 3 floats: optimiser steps taken, num_batches_tracked, workspace bytes per chunk (read only) */
};
#define RMR_TRAIN_NAME_LEN 32
/* `blob`: the initial state, host, rmr_model_weight_count(desc) floats; desc->dtype must be 0.  The workspace is allocated
 * here, once, for max_batch chunks.
 * replaces: model construction and `.to(device)`, src/remora/train_model.py:333-352; torch.optim.AdamW's state, :354-360. */
int rmr_trainer_create(rmr_engine *e, const rmr_model_desc *desc, const float *blob, size_t n_floats, int64_t max_batch,
                       rmr_trainer **out);
void rmr_trainer_destroy(rmr_trainer *t);
/* sigs f32[n][1][L], seqs f32[n][4 kmer_len][L] (dense one-hot, as rmr_forward takes them), labels i64[n], mask u8[n] or
 * NULL (rows with 0 leave the loss and still take part in BatchNorm: --high-conf-incorrect-thr-frac); all four in `mem`.
 * Fills the gradient buffer, moves the running statistics, *loss (HOST) = mean cross-entropy; logits f32[n][num_out] (in
 * `mem`) or NULL.  Synchronous.
 * A label outside 0..num_out-1 in a row of the loss (torch raises there) is refused by name, RMR_ERR_INVALID "label ... of chunk
 * ... is outside 0..num_out-1", with the gradients, the running statistics, the batch counter and *loss left as they were;
 * rows the mask drops may hold any label.  HOST labels are checked before anything is staged or launched.  DEVICE labels are
 * checked by the step's first kernel, which leaves the first such row beside the row count; the kernels that write a gradient
 * or a running statistic read that record and hold their stores, and the host reads it with the loss on the one
 * synchronisation the call always had - the step's other launches still run, and a DEVICE `logits` is written.
 * replaces: model.train(); outputs = model(sigs, seqs); loss = criterion(outputs, labels); loss.backward(),
 *           src/remora/train_model.py:470-499. */
int rmr_trainer_forward_backward(rmr_trainer *t, const float *sigs, const float *seqs, const int64_t *labels,
                                 const uint8_t *mask, int64_t n, float *loss, float *logits, int mem);
/* out (HOST) f32[parameter tensors]: max |grad| of each, named_parameters order.
 * replaces: apply_clipping's grad_maxs, src/remora/train_model.py:118-123. */
int rmr_trainer_grad_absmax(rmr_trainer *t, float *out);
/* One torch.optim.AdamW step over the whole buffer in one launch: decoupled decay p -= lr wd p, bias-corrected moments,
 * p -= lr mhat / (sqrt(vhat) + eps).  clip (HOST, f32[parameter tensors]) or NULL: gradients of tensor i are clamped to
 * [-clip[i], clip[i]] first (a negative entry: not clamped).  The scalars are doubles so that 1 - beta is formed before the
 * rounding to fp32, as torch forms it (1 - (float)0.999 is off by 1.3e-5 of itself).
 * replaces: apply_clipping's clamp_ and opt.step(), src/remora/train_model.py:124-131, :500-503. */
int rmr_trainer_adamw_step(rmr_trainer *t, double lr, double beta1, double beta2, double eps, double weight_decay, const float *clip);
/* copy one buffer (rmr_train_buffer) to / from HOST memory; n_floats must be the buffer's size
 * replaces: model.state_dict() / load_state_dict(), opt.state_dict(), src/remora/train_model.py:134-161. */
int rmr_trainer_read(rmr_trainer *t, int which, float *out, size_t n_floats);
int rmr_trainer_write(rmr_trainer *t, int which, const float *in, size_t n_floats);
/* The tensors of the flat buffer in order: names (cap x RMR_TRAIN_NAME_LEN bytes, NUL-terminated torch names), offsets and
 * sizes in floats, is_param (0: a running statistic).  The entries with is_param = 1 are named_parameters, in its order.
 * Every array may be NULL; *n_out = number of tensors.
 * replaces: model.named_parameters() / named_buffers(). */
int rmr_trainer_tensor_layout(const rmr_trainer *t, int cap, char *names, int64_t *offsets, int64_t *sizes, int32_t *is_param,
                              int *n_out);

/* ---- measurement: HIP-event timing of every kernel launch on the engine stream ----------- */
int rmr_profile_enable(rmr_engine *e, int on);
int rmr_profile_reset(rmr_engine *e);
int rmr_profile_num_kernels(void);
const char *rmr_profile_kernel_name(int kernel_id);
/* synchronises, then returns accumulated event time and launch count for one kernel id */
int rmr_profile_get(rmr_engine *e, int kernel_id, double *total_ms, int64_t *launches);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* REMORA_HIP_H */
