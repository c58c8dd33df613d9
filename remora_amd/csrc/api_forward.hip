// api_forward.hip — models and the forward entry points of the C ABI: model creation (fold and pack on the host, rmr_pack.h,
// then upload), the three forward pipelines over the kernels of k_*.hip, rmr_forward, rmr_infer_chunks and rmr_call_read.
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <thread>
#include <tuple>

#include "rmr_internal.h"
#include "rmr_geometry.h"
#include "rmr_probe.h"
#include "rmr_stage.h"

using namespace rmr;

// =========================================================================================
// model: fold and pack on the host (rmr_pack.h), upload
// =========================================================================================

extern "C" {

size_t rmr_model_weight_count(const rmr_model_desc *d) { return (d && desc_ok(*d)) ? weight_count(*d) : 0; }

void rmr_model_destroy(rmr_model *m) {
    if (!m) return;
    if (m->eng) {
        (void)hipSetDevice(m->eng->device);
        (void)hipStreamSynchronize(m->eng->stream);
    }
    for (void *p : m->dev_allocs) (void)hipFree(p);
    delete m;
}

int rmr_model_padded_size(const rmr_model_desc *d) { return (d && desc_ok(*d)) ? padded_size(d->size, d->dtype) : 0; }

int rmr_model_pad_weights(const rmr_model_desc *desc, const float *weights, size_t n_floats, rmr_model_desc *padded_desc,
                          float *out, size_t out_cap, size_t *out_n) {
    if (!desc || !weights || !padded_desc || !out_n) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (!desc_ok(*desc)) RMR_FAIL(RMR_ERR_INVALID, "unsupported model description");
    if (rmr_model_weight_count(desc) != n_floats)
        RMR_FAIL(RMR_ERR_INVALID, "weight blob has %zu floats, expected %zu", n_floats, rmr_model_weight_count(desc));
    *padded_desc = *desc;
    padded_desc->size = padded_size(desc->size, desc->dtype);
    *out_n = rmr_model_weight_count(padded_desc);
    if (!out) return 0;  // size query
    if (out_cap < *out_n) RMR_FAIL(RMR_ERR_INVALID, "output holds %zu floats, %zu needed", out_cap, *out_n);
    if (padded_desc->size == desc->size) {
        memcpy(out, weights, n_floats * sizeof(float));
        return 0;
    }
    const std::vector<float> o = pad_model_blob(*desc, weights, padded_desc->size);
    if (o.size() != *out_n) RMR_FAIL(RMR_ERR_INVALID, "internal: padded blob has %zu floats, expected %zu", o.size(), *out_n);
    memcpy(out, o.data(), o.size() * sizeof(float));
    return 0;
}

static int model_create_at_kernel_size(rmr_engine *e, const rmr_model_desc *desc, const float *weights, size_t n_floats, rmr_model **out);
static int model_probe_winograd(rmr_model *m, float tol);

// the load-time screen of the Winograd kernels (below, behind the pipelines); a model whose probe fails to run is not handed out
static int model_probe_or_destroy(rmr_model **out) {
    const int rc = model_probe_winograd(*out, -1.0f);
    if (rc != 0) {
        rmr_model_destroy(*out);
        *out = nullptr;
    }
    return rc;
}

int rmr_model_create(rmr_engine *e, const rmr_model_desc *desc, const float *weights,
                     size_t n_floats, rmr_model **out) {
    if (!e || !desc || !weights || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (!desc_ok(*desc))
        RMR_FAIL(RMR_ERR_INVALID,
                 "unsupported model: arch=%d size=%d kmer_len=%d num_out=%d dtype=%d "
                 "(size 1..%d; num_out <= 16; the 16-bit dtypes need conv_lstm; up to 64 channels f16 takes 33..64 channels and a k-mer "
                 "length of 9 or 6; above 64 channels the dtypes are fp32, bf16 and f16)",
                 desc->arch, desc->size, desc->kmer_len, desc->num_out, desc->dtype, kMaxPaddedSize);
    const size_t want = rmr_model_weight_count(desc);
    if (want != n_floats) RMR_FAIL(RMR_ERR_INVALID, "weight blob has %zu floats, expected %zu", n_floats, want);
    const int sp = padded_size(desc->size, desc->dtype);
    if (sp == desc->size) {
        RMR_TRY(model_create_at_kernel_size(e, desc, weights, n_floats, out));
        return model_probe_or_destroy(out);
    }
    rmr_model_desc pd = *desc;
    pd.size = sp;
    const std::vector<float> blob = pad_model_blob(*desc, weights, sp);
    RMR_TRY(model_create_at_kernel_size(e, &pd, blob.data(), blob.size(), out));
    (*out)->true_size = desc->size;
    return model_probe_or_destroy(out);
}

// `desc->size` is a size the kernels run at (padded_size is the identity on it)
static int model_create_at_kernel_size(rmr_engine *e, const rmr_model_desc *desc, const float *weights, size_t n_floats, rmr_model **out) {
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::unique_ptr<rmr_model, void (*)(rmr_model *)> m(new rmr_model(), rmr_model_destroy);
    m->eng = e;
    m->true_size = desc->size;
    RMR_TRY(pack_model(*desc, weights, n_floats, m.get(), [&](const std::string &, const std::vector<float> &h, float **dev) -> int {
        void *p = nullptr;
        RMR_HIP(hipMalloc(&p, h.size() * sizeof(float) + 16));
        m->dev_allocs.push_back(p);
        RMR_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        *dev = reinterpret_cast<float *>(p);
        return 0;
    }));
    m->sig3.kid = K_CONV_SIG3;  // profiling ids
    m->seq2.kid = K_CONV_SEQ2;
    m->seq3.kid = K_CONV_SEQ3;
    m->merge1.kid = K_CONV_MERGE1;
    m->merge2.kid = K_CONV_MERGE2;
    m->merge3.kid = K_CONV_MERGE3;
    m->merge4.kid = K_CONV_MERGE4;
    *out = m.release();
    return 0;
}

}  // extern "C"

// =========================================================================================
// forward pipelines
// =========================================================================================
namespace {

// The loop of every pipeline: sub-batches of `dflt` chunks (rmr_engine_set_subbatch overrides it), never more than n; the
// activation arena holds `act_bytes` per chunk of one sub-batch.  body(c0, nb, sb): chunks [c0, c0 + nb) of sub-batches of sb.
template <class Body>
int for_subbatches(rmr_engine *e, int64_t dflt, int64_t n, size_t act_bytes, Body body) {
    int64_t sb = e->subbatch > 0 ? e->subbatch : dflt;
    if (sb > n) sb = n;
    RMR_TRY(e->ensure(e->act, act_bytes * sb));
    for (int64_t c0 = 0; c0 < n; c0 += sb) RMR_TRY(body(c0, (n - c0) < sb ? (n - c0) : sb, sb));
    return 0;
}

// bf16 / f16 above 64 channels (k_stream16.hip): fp32 front kernels (sig_conv1/2, seq_conv1: 16 channels), then the three
// size-wide convolutions and the LSTM on the 16-bit matrix cores with streamed weights; cat and x are 16-bit in HBM
int pipeline_stream16(rmr_model *m, const ChunkArrays &in, int64_t n, float *logits) {
    rmr_engine *e = m->eng;
    const int sz = m->desc.size, L = m->L, EC = 4 * m->desc.kmer_len;
    const size_t front_fl = (size_t)(m->P1 + m->P2) * 16;
    const size_t cat_el = (size_t)m->P3 * 2 * sz, x_el = (size_t)m->T * sz;
    // a chunk length one of the three convolutions refuses is refused here, before the front kernels are queued
    RMR_TRY(check_conv_stream16(m->sig3, m->P2));
    RMR_TRY(check_conv_stream16(m->seq2, m->P1));
    RMR_TRY(check_conv_stream16(m->merge1, m->P3));
    return for_subbatches(e, 131072, n, front_fl * sizeof(float) + (cat_el + x_el) * sizeof(uint16_t) + 64, [&](int64_t c0, int64_t nb, int64_t sb) -> int {
        float *seq1 = reinterpret_cast<float *>(e->act.ptr);
        float *sig2 = seq1 + (size_t)nb * m->P1 * 16;
        uint16_t *cat = reinterpret_cast<uint16_t *>(seq1 + front_fl * sb);
        uint16_t *x16 = cat + cat_el * sb + 32;
        const ChunkArrays b = in.at(c0, L, EC);
        RMR_TRY(launch_front(m, e->stream, b, nb, sig2, b.enc ? nullptr : seq1));
        if (b.enc) RMR_TRY(launch_seq1_dense(m, b.enc, nb, seq1));
        RMR_TRY(launch_conv_stream16(m, m->sig3, sig2, false, m->P2, cat, 2 * sz, 0, m->P3, nb));
        RMR_TRY(launch_conv_stream16(m, m->seq2, seq1, false, m->P1, cat, 2 * sz, sz, m->P3, nb));
        RMR_TRY(launch_conv_stream16(m, m->merge1, cat, true, m->P3, x16, sz, 0, m->T, nb));
        return launch_lstm_stream16(m, x16, nb, logits + (size_t)c0 * m->desc.num_out);
    });
}

// plain-bf16 / f16 ConvLSTM (k_fused.hip): two launches per sub-batch, x (bf16, 3 KB/chunk @C100) is the only intermediate in
// HBM; sub-batches are sized so that x stays in the 256 MiB Infinity Cache between producer and consumer
int pipeline_fused(rmr_model *m, const ChunkArrays &in, int64_t n, float *logits) {
    rmr_engine *e = m->eng;
    const size_t x_elems = (size_t)m->T * m->desc.size;
    return for_subbatches(e, 65536, n, x_elems * sizeof(uint16_t), [&](int64_t c0, int64_t nb, int64_t) -> int {
        uint16_t *x16 = reinterpret_cast<uint16_t *>(e->act.ptr);
        RMR_TRY(launch_fused_front(m, in.at(c0, m->L, 0), nb, x16));
#ifdef RMR_TIMING_ABLATIONS  // experiment build only (make abl; tools/stress_determinism.py): x of every sub-batch, appended
        if (const char *dump = getenv("RMR_FUSED_DUMP_X")) {
            std::vector<uint16_t> h(x_elems * nb);
            RMR_HIP(hipStreamSynchronize(e->stream));
            RMR_HIP(hipMemcpy(h.data(), x16, h.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
            if (FILE *f = fopen(dump, "ab")) {
                fwrite(h.data(), sizeof(uint16_t), h.size(), f);
                fclose(f);
            }
        }
        if (abl_int("RMR_DEBUG_SKIP_LSTM", 0)) return 0;  // the front kernel alone (x through RMR_FUSED_DUMP_X)
#endif
        return launch_lstm_head_x16(m, x16, nb, logits + (size_t)c0 * m->desc.num_out);
    });
}

size_t act_floats_per_chunk(const rmr_model *m) {
    const size_t sz = m->desc.size;
    const size_t n = (size_t)m->P1 * 16 + (size_t)m->P2 * 16 + (size_t)m->P3 * 2 * sz;
    if (m->desc.arch == RMR_ARCH_CONV_LSTM) return n + (size_t)m->T * sz;
    return n + (size_t)m->PQ2 * 32 + (size_t)(m->T + m->T2 + m->T3 + m->T4) * sz;
}

// fp32 (and the split 16-bit dtypes, nparts > 0), both architectures
int pipeline_fp32(rmr_model *m, const ChunkArrays &in, int64_t n, float *logits, const FwdSwitches &sw) {
    rmr_engine *e = m->eng;
    const int sz = m->desc.size, L = m->L, EC = 4 * m->desc.kmer_len;
    // fp32 ConvLSTM size 64 straight from the chunk arrays: sig_conv1/2 and seq_conv1 are produced inside the staging of
    // sig_conv3 / seq_conv2 (k_conv_front.hip); sig2 / seq1 never exist in HBM.  (RMR_CONV_FRONT=0: the separate front
    // kernels - the comparand of tests/test_gpu_conv_front.py)
    const bool fold = !in.enc && sw.conv_front && conv_front_supported(m, in.kb, in.ka, in.seq_w, in.map_w);
    // every other fp32 path (Conv_w_ref; ConvLSTM shapes the two-branch fold does not cover): the signal branch alone is
    // folded - sig_conv1 / sig_conv2 (matrix cores) produced inside the staging of sig_conv3, sig2 never in HBM
    const bool sigfold = !fold && m->nparts == 0 && sw.sig3_mfma && sig3_front_mfma_supported(m);
    // (Running the front kernels of sub-batch i + 1 on a second stream under the matrix kernels of sub-batch i was measured in
    //  rounds 1-2 in two forms and gained nothing - they share the CUs with conv_sig3, or half a register file under the LSTM -
    //  and is gone; profiles/NOTES_r03.md.)
    const size_t front_fl = fold ? 0 : (size_t)(m->P1 + m->P2) * 16;
    const bool split_conv = m->nparts > 0;
    // 262144 chunks per sub-batch: the tail of every persistent-block kernel is paid half as often as with 131072
    // (+1.2 % measured; 524288: +0.2 % more for twice the 5.5 GB arena)
    return for_subbatches(e, 262144, n, (act_floats_per_chunk(m) + front_fl) * sizeof(float), [&](int64_t c0, int64_t nb, int64_t sb) -> int {
        float *seq1 = reinterpret_cast<float *>(e->act.ptr), *rest = seq1 + front_fl * sb;
        float *sig2 = seq1 + (size_t)nb * m->P1 * 16;
        float *out = logits + (size_t)c0 * m->desc.num_out;
        const ChunkArrays b = in.at(c0, L, EC);
        if (!fold) {  // sig_conv1/2 -> sig2 unless folded, seq_conv1 -> seq1 from the chunk arrays or the dense tensor (k_front.hip)
            if (!b.enc || !sigfold) RMR_TRY(launch_front(m, e->stream, b, nb, sigfold ? nullptr : sig2, b.enc ? nullptr : seq1));
            if (b.enc) RMR_TRY(launch_seq1_dense(m, b.enc, nb, seq1));
        }
        float *base = rest;
        float *cat = base; base += (size_t)nb * m->P3 * 2 * sz;
        if (fold) RMR_TRY(launch_conv_front(m, b, nb, cat, sw));
        else if (split_conv) RMR_TRY(launch_conv_split(e, m->sig3, m->nparts, sig2, 16, m->P2, cat, 2 * sz, 0, m->P3, nb));
        else if (sigfold) RMR_TRY(launch_sig3_front_mfma(m, b.signal, nb, cat, sw.winograd));
        else RMR_TRY(launch_conv(e, m->sig3, sig2, 16, m->P2, cat, 2 * sz, 0, m->P3, nb, sw.winograd));
#ifdef RMR_TIMING_ABLATIONS  // experiment build only (tools/stress_determinism.py): cat [nb][P3][2 sz] of the last sub-batch
        if (const char *dump = fold ? getenv("RMR_DUMP_CAT") : nullptr) {
            std::vector<float> h((size_t)nb * m->P3 * 2 * sz);
            RMR_HIP(hipStreamSynchronize(e->stream));
            RMR_HIP(hipMemcpy(h.data(), cat, h.size() * sizeof(float), hipMemcpyDeviceToHost));
            if (FILE *f = fopen(dump, "wb")) {
                fwrite(h.data(), sizeof(float), h.size(), f);
                fclose(f);
            }
        }
#endif
        if (m->desc.arch == RMR_ARCH_CONV_LSTM) {
            float *x = base; base += (size_t)nb * m->T * sz;
            if (fold) {
                RMR_TRY(launch_conv(e, m->merge1, cat, 2 * sz, m->P3, x, sz, 0, m->T, nb, sw.winograd));
            } else if (split_conv) {
                RMR_TRY(launch_conv_split(e, m->seq2, m->nparts, seq1, 16, m->P1, cat, 2 * sz, sz, m->P3, nb));
                RMR_TRY(launch_conv_split(e, m->merge1, m->nparts, cat, 2 * sz, m->P3, x, sz, 0, m->T, nb));
            } else {
                RMR_TRY(launch_conv(e, m->seq2, seq1, 16, m->P1, cat, 2 * sz, sz, m->P3, nb, sw.winograd));
                RMR_TRY(launch_conv(e, m->merge1, cat, 2 * sz, m->P3, x, sz, 0, m->T, nb, sw.winograd));
            }
            if (m->nparts > 0 && lstm_x16s_supported(m)) return launch_lstm_head_x16s(m, x, nb, out);
            if (m->nparts > 0) return launch_lstm_head_split(m, x, nb, out);
            return launch_lstm_head(m, x, nb, out);
        }
        float *seq2 = base; base += (size_t)nb * m->PQ2 * 32;
        float *m1 = base; base += (size_t)nb * m->T * sz;
        float *m2 = base; base += (size_t)nb * m->T2 * sz;
        float *m3 = base; base += (size_t)nb * m->T3 * sz;
        float *m4 = base;
        RMR_TRY(launch_conv(e, m->seq2, seq1, 16, m->P1, seq2, 32, 0, m->PQ2, nb, sw.winograd));
        RMR_TRY(launch_conv(e, m->seq3, seq2, 32, m->PQ2, cat, 2 * sz, sz, m->P3, nb, sw.winograd));
        RMR_TRY(launch_conv(e, m->merge1, cat, 2 * sz, m->P3, m1, sz, 0, m->T, nb, sw.winograd));
        RMR_TRY(launch_conv(e, m->merge2, m1, sz, m->T, m2, sz, 0, m->T2, nb, sw.winograd));
        RMR_TRY(launch_conv(e, m->merge3, m2, sz, m->T2, m3, sz, 0, m->T3, nb, sw.winograd));
        RMR_TRY(launch_conv(e, m->merge4, m3, sz, m->T3, m4, sz, 0, m->T4, nb, sw.winograd));
        return launch_fc_head(m, m4, nb, out);
    });
}

// in.enc != nullptr: dense seqs path; otherwise gather path from (seqs, maps, lens)
int run_pipeline(rmr_model *m, const ChunkArrays &in, int64_t n, float *logits) {
    if (n <= 0) return 0;
    if (in.enc) RMR_TRY(check_seq1_dense(m));  // before the signal branch is launched
    // the switches of every kernel choice below, read once per call
    const FwdSwitches sw{tune_int("RMR_FUSED", 1) != 0, tune_int("RMR_CONV_FRONT", 1) != 0,
                         tune_int("RMR_WINOGRAD", 1) != 0 && m->use_winograd, tune_int("RMR_SIG3_MFMA", 1) != 0};
    if (m->nparts == 1 && m->desc.size > 64) return pipeline_stream16(m, in, n, logits);
    if (m->f16 && (in.enc || !fused_front_supported(m, in.seq_w, in.map_w)))
        RMR_FAIL(RMR_ERR_INVALID, "dtype f16 runs on the fused kernels only: chunk arrays (not a dense one-hot tensor), sequence rows of at "
                                  "most 256 columns, a chunk length that is a multiple of 4");
    if (!in.enc && fused_front_supported(m, in.seq_w, in.map_w) && (m->f16 || sw.fused)) return pipeline_fused(m, in, n, logits);
    return pipeline_fp32(m, in, n, logits, sw);
}

// ---- the Winograd guard (include/remora_hip.h, rmr_model_numerics) ---------------------------------------------------------
constexpr float kWinogradTol = 2e-5f;  // what tests/test_gpu_wino.py allows the two forms on the reference-generated models

// Whether a forward call of this model launches a kernel in a Winograd form: the question pipeline_fp32 and launch_conv answer
// per launch, asked for the layers of the architecture at once.  `seq_w`, `map_w`, `n`: the probe's chunk arrays (the fronts'
// plans depend on them only through what fits the LDS; a dense one-hot call takes a subset of these kernels).
bool model_takes_winograd(const rmr_model *m, int kb, int ka, int seq_w, int map_w, int64_t n) {
    if (m->desc.dtype != 0 || m->nparts != 0 || m->f16) return false;
    auto conv = [](const ConvLayer &c, int pin, int pout) { return conv_wino_supported(c, pin, pout) || conv_wino_s3_supported(c, pin, pout); };
    const bool sw_front = tune_int("RMR_CONV_FRONT", 1) != 0, sw_mfma = tune_int("RMR_SIG3_MFMA", 1) != 0;
    const bool fold = sw_front && conv_front_supported(m, kb, ka, seq_w, map_w);
    bool any = fold ? seq2_front_takes_winograd(m, seq_w, map_w, n) : false;
    if (sw_mfma && sig3_front_mfma_supported(m)) any |= sig3_front_takes_winograd(m, n);
    else if (!fold) any |= conv(m->sig3, m->P2, m->P3);
    any |= conv(m->merge1, m->P3, m->T);
    if (m->desc.arch == RMR_ARCH_CONV_LSTM) return any || (!fold && conv(m->seq2, m->P1, m->P3));
    return any || conv(m->seq2, m->P1, m->PQ2) || conv(m->seq3, m->PQ2, m->P3) || conv(m->merge2, m->T, m->T2) ||
           conv(m->merge3, m->T2, m->T3) || conv(m->merge4, m->T3, m->T4);
}

}  // namespace

// The probe batch (rmr_probe.h) through pipeline_fp32 in both forms, everything on the device, and the decision of
// include/remora_hip.h.  tol < 0: the default.  On the engine's stream, synchronised before returning; the engine's sub-batch
// setting and its profiler are put aside for the two runs (no record of the probe reaches rmr_profile_get).
static int model_probe_winograd(rmr_model *m, float tol) {
    rmr_engine *e = m->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    rmr_model_numerics &nm = m->numerics;
    nm = rmr_model_numerics{};
    nm.tol = tol < 0.0f ? kWinogradTol : tol;
    m->use_winograd = true;
    const int K = m->desc.kmer_len, kb = (K - 1) / 2, ka = K - 1 - kb, L = m->L, no = m->desc.num_out;
    const int max_len = probe_max_len(L);
    if (!model_takes_winograd(m, kb, ka, max_len + kb + ka, max_len + 1, PROBE_CHUNKS)) return 0;
    // the entry the probe goes through: the chunk arrays where launch_front takes the model's k-mer length, else the same batch
    // as a one-hot tensor through the dense entry; a model that neither entry runs (every forward call of it is refused by name)
    // has no form to choose and is handed out unchecked
    const bool dense = !front_seq_supported(m, max_len + kb + ka, max_len + 1);
    if (dense && !seq1_dense_supported(m)) return 0;
    // the batch is generated once per geometry and kept as ONE host blob in the layout of the staging slots below: one upload
    struct Packed { ProbeBatch pb; std::vector<char> blob; };
    static std::mutex cache_mu;
    static std::map<std::tuple<int, int, int>, Packed> cache;
    const Packed *pk;
    {
        std::lock_guard<std::mutex> ck(cache_mu);
        Packed &c = cache[std::make_tuple(L, kb, ka)];
        if (c.blob.empty()) {
            c.pb = make_probe_batch(L, kb, ka);
            const size_t o_seq = Stage::pad(c.pb.signal.size() * sizeof(float)), o_map = o_seq + Stage::pad(c.pb.seqs.size());
            const size_t o_len = o_map + Stage::pad(c.pb.maps.size() * sizeof(int16_t));
            c.blob.assign(o_len + Stage::pad(c.pb.lens.size() * sizeof(int16_t)), 0);
            memcpy(c.blob.data(), c.pb.signal.data(), c.pb.signal.size() * sizeof(float));
            memcpy(c.blob.data() + o_seq, c.pb.seqs.data(), c.pb.seqs.size());
            memcpy(c.blob.data() + o_map, c.pb.maps.data(), c.pb.maps.size() * sizeof(int16_t));
            memcpy(c.blob.data() + o_len, c.pb.lens.data(), c.pb.lens.size() * sizeof(int16_t));
        }
        pk = &c;  // (std::map: the node stays where it is)
    }
    const ProbeBatch &pb = pk->pb;
    const int64_t n = pb.n;
    Stage st;
    float *dsig, *dw, *dd;
    int8_t *ds;
    int16_t *dm, *dl;
    unsigned *dred;
    st.add(&dsig, pb.signal.size()).add(&ds, pb.seqs.size()).add(&dm, pb.maps.size()).add(&dl, pb.lens.size());
    if (st.total != pk->blob.size()) RMR_FAIL(RMR_ERR_INVALID, "internal: probe blob of %zu bytes, slots of %zu", pk->blob.size(), st.total);
    st.add(&dw, (size_t)n * no).add(&dd, (size_t)n * no).add(&dred, 2);
    float *denc = nullptr;
    const std::vector<float> enc = dense ? probe_one_hot(pb) : std::vector<float>();  // (alive until the stream is synchronised below)
    st.add(&denc, enc.size());
    RMR_TRY(st.commit(e));
    H2D(dsig, pk->blob.data(), pk->blob.size());
    H2D(denc, enc.data(), enc.size() * sizeof(float));
    const ChunkArrays in = dense ? ChunkArrays{dsig, denc, nullptr, 0, nullptr, 0, nullptr, 0, 0}
                                 : ChunkArrays{dsig, nullptr, ds, pb.seq_w, dm, pb.map_w, dl, kb, ka};
    const bool profiling = e->profiling;
    const int64_t subbatch = e->subbatch;
    e->profiling = false;
    e->subbatch = 0;
    unsigned red[2] = {0, 0};
    auto run = [&]() -> int {
        FwdSwitches sw{false, tune_int("RMR_CONV_FRONT", 1) != 0, true, tune_int("RMR_SIG3_MFMA", 1) != 0};
        RMR_TRY(pipeline_fp32(m, in, n, dw, sw));
        sw.winograd = false;
        RMR_TRY(pipeline_fp32(m, in, n, dd, sw));
        RMR_TRY(launch_probe_compare(e, dw, dd, n * no, dred));
        D2H(red, dred, sizeof(red));
        RMR_HIP(hipStreamSynchronize(e->stream));
        return 0;
    };
    const int rc = run();
    e->profiling = profiling;
    e->subbatch = subbatch;
    if (rc != 0) {
        (void)hipStreamSynchronize(e->stream);
        return rc;
    }
    nm.checked = 1;
    nm.probe_chunks = (int32_t)n;
    memcpy(&nm.max_abs_diff, &red[0], sizeof(float));
    nm.nonfinite = (int32_t)red[1];
    m->use_winograd = nm.nonfinite == 0 && nm.max_abs_diff <= nm.tol;
    nm.winograd = m->use_winograd ? 1 : 0;
    return 0;
}

extern "C" {

int rmr_model_numerics_get(const rmr_model *m, rmr_model_numerics *out) {
    if (!m || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> lk(m->eng->mu);
    *out = m->numerics;
    return 0;
}

int rmr_model_check_winograd(rmr_model *m, float tol, rmr_model_numerics *out) {
    if (!m) RMR_FAIL(RMR_ERR_INVALID, "model is NULL");
    if (tol != tol) RMR_FAIL(RMR_ERR_INVALID, "tol is NaN");
    RMR_TRY(model_probe_winograd(m, tol));
    if (out) *out = m->numerics;
    return 0;
}

int rmr_forward(rmr_model *m, const float *sigs, const float *seqs, int64_t n, float *logits, int mem) {
    if (!m || !sigs || !seqs || !logits) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n <= 0) return 0;
    rmr_engine *e = m->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE) return run_pipeline(m, ChunkArrays{sigs, seqs, nullptr, 0, nullptr, 0, nullptr, 0, 0}, n, logits);
    const size_t L = m->L, EC = 4 * (size_t)m->desc.kmer_len, no = m->desc.num_out;
    Stage st;
    float *ds, *dq, *dl;
    st.add(&ds, n * L).add(&dq, n * EC * L).add(&dl, n * no);
    RMR_TRY(st.commit(e));
    H2D(ds, sigs, n * L * 4);
    H2D(dq, seqs, n * EC * L * 4);
    RMR_TRY(run_pipeline(m, ChunkArrays{ds, dq, nullptr, 0, nullptr, 0, nullptr, 0, 0}, n, dl));
    D2H(logits, dl, n * no * 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// ---- one read, one call: staging + X1-X3 + the network, ONE stream synchronisation -------------------------------------
int rmr_call_read(rmr_model *m, const rmr_read *r, float *logits, int64_t *read_focus_bases) {
    if (!m || !r || !logits || !read_focus_bases) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (r->n_focus <= 0) return 0;
    if (!r->dacs || !r->seq_to_sig || !r->int_seq || !r->focus_bases) RMR_FAIL(RMR_ERR_INVALID, "NULL array in rmr_read");
    if (r->n_sig <= 0 || r->n_bases <= 0) RMR_FAIL(RMR_ERR_INVALID, "empty read");
    if (r->seq_itemsize != 1 && r->seq_itemsize != 2 && r->seq_itemsize != 4 && r->seq_itemsize != 8)
        RMR_FAIL(RMR_ERR_INVALID, "int_seq itemsize %d not in {1,2,4,8}", r->seq_itemsize);
    if (r->kb < 0 || r->ka < 0 || r->kb + r->ka + 1 != m->desc.kmer_len)
        RMR_FAIL(RMR_ERR_INVALID, "kmer context (%d,%d) does not match model kmer_len %d", r->kb, r->ka, m->desc.kmer_len);
    if (r->cc_before + r->cc_after != m->L)
        RMR_FAIL(RMR_ERR_INVALID, "chunk context (%d,%d) does not match model chunk_len %d", r->cc_before, r->cc_after, m->L);
    rmr_engine *e = m->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    const int64_t ns = r->n_sig, nb = r->n_bases, nc = r->n_focus;
    const int no = m->desc.num_out, L = m->L;
    // one pinned host blob: everything the extraction kernels read, the geometry rows behind it, then the logits
    size_t off = 0;
    auto seg = [&off](size_t bytes) { const size_t o = off; off += Stage::pad(bytes); return o; };
    const size_t o_dacs = seg(ns * 2 + 16), o_map = seg((nb + 1) * 8), o_seq = seg(nb + 16), o_foc = seg(nc * 8), o_off = seg(6 * 8),
                 o_sc = seg(2 * 8), o_cr = seg((nc + 1) * 4), o_geo = seg(nc * 48), in_bytes = off;
    const size_t out_bytes = Stage::pad((size_t)nc * no * 4) + 256;
    RMR_TRY(e->ensure_pin_call(in_bytes + out_bytes));
    char *hp = reinterpret_cast<char *>(e->pin_call);
    // The staging buffer is pinned host memory the GPU can address: for ONE read the kernels fetch the read's arrays and the
    // chunk geometry from it across PCIe themselves and write the logits back into it (150 KB in, 2.5 KB out) instead of three
    // queued copies, each of which cost a launch on the host and a blit kernel + a dependency gap on the stream - a sixth of
    // the call (profiles/NOTES_r05.md section 1d).
    char *dp = nullptr;
    RMR_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&dp), hp, 0));
    memcpy(hp + o_dacs, r->dacs, (size_t)ns * 2);
    memcpy(hp + o_map, r->seq_to_sig, (size_t)(nb + 1) * 8);
    {
        int8_t *q = reinterpret_cast<int8_t *>(hp + o_seq);
        switch (r->seq_itemsize) {
        case 1: memcpy(q, r->int_seq, (size_t)nb); break;
        case 2: { const int16_t *s = reinterpret_cast<const int16_t *>(r->int_seq); for (int64_t i = 0; i < nb; ++i) q[i] = (int8_t)s[i]; } break;
        case 4: { const int32_t *s = reinterpret_cast<const int32_t *>(r->int_seq); for (int64_t i = 0; i < nb; ++i) q[i] = (int8_t)s[i]; } break;
        default: { const int64_t *s = reinterpret_cast<const int64_t *>(r->int_seq); for (int64_t i = 0; i < nb; ++i) q[i] = (int8_t)s[i]; } break;
        }
    }
    memcpy(hp + o_foc, r->focus_bases, (size_t)nc * 8);
    int64_t *ho = reinterpret_cast<int64_t *>(hp + o_off);
    ho[0] = 0; ho[1] = ns; ho[2] = 0; ho[3] = nb; ho[4] = 0; ho[5] = nc;
    double *hs = reinterpret_cast<double *>(hp + o_sc);
    hs[0] = r->shift; hs[1] = r->scale;
    memset(hp + o_cr, 0, (size_t)(nc + 1) * 4);  // every chunk belongs to read 0
    rmr_reads d{};
    d.n_reads = 1;
    d.dacs = reinterpret_cast<const int16_t *>(dp + o_dacs);
    d.seq_to_sig = reinterpret_cast<const int64_t *>(dp + o_map);
    d.int_seq = reinterpret_cast<const int8_t *>(dp + o_seq);
    d.focus_bases = reinterpret_cast<const int64_t *>(dp + o_foc);
    d.sig_off = reinterpret_cast<const int64_t *>(dp + o_off);
    d.seq_off = d.sig_off + 2, d.focus_off = d.sig_off + 4;
    d.shift = reinterpret_cast<const double *>(dp + o_sc);
    d.scale = d.shift + 1;
    d.cc_before = r->cc_before; d.cc_after = r->cc_after; d.kb = r->kb; d.ka = r->ka;
    d.base_start_justify = r->base_start_justify; d.offset = r->offset;
    const int32_t *chunk_read = reinterpret_cast<const int32_t *>(dp + o_cr);
    const int64_t *dgeo = reinterpret_cast<const int64_t *>(dp + o_geo);
    float *dlog = reinterpret_cast<float *>(dp + in_bytes), *hlog = reinterpret_cast<float *>(hp + in_bytes);
    // The arena is planned before the widths of the chunk rows are known, for chunks of up to `cap` bases (a chunk of L samples
    // holds more only where bases have no samples of their own: then it is planned again for the exact number below, before
    // anything that depends on it is queued).
    auto seq_w_of = [r](int64_t bases) { return (int)std::max<int64_t>(bases + r->kb + r->ka, r->kb + r->ka + 1); };
    auto map_w_of = [](int64_t bases) { return (int)std::max<int64_t>(bases + 1, 2); };
    float *dsig = nullptr;
    ChunkSlots c;
    auto plan = [&](int64_t bases) {
        Stage st;
        st.add(&dsig, ns + 4);
        c.declare(st, nc, L, seq_w_of(bases), map_w_of(bases));
        return st.commit(e);
    };
    const int64_t cap = std::min<int64_t>(nb + 1, 2 * (int64_t)L + 8);
    RMR_TRY(plan(cap));
    RMR_TRY(launch_geometry(e, d, 0, chunk_read, dsig, ns, nullptr, nullptr, nullptr));  // n_chunks 0: the signal normalisation alone
    // While that runs, the geometry of the chunks on the host: integer arithmetic on the mapping - the function the
    // geometry kernel runs (rmr_geometry.h), its searches started at the focus base when the mapping is monotone.  The widths
    // of the chunk rows are then known without asking the GPU: the whole call is queued behind one another and waited for once.
    const int64_t *map = reinterpret_cast<const int64_t *>(hp + o_map);
    bool monotone = true;
    for (int64_t i = 0; i < nb; ++i) monotone &= map[i + 1] >= map[i];
    int64_t *hgeo = reinterpret_cast<int64_t *>(hp + o_geo);
    int64_t msl = 0;
    for (int64_t i = 0; i < nc; ++i) {
        const int64_t sl = chunk_geometry_row(map, nb, ns, r->focus_bases[i], r->base_start_justify, r->offset, r->cc_before, r->cc_after,
                                              hgeo + i * 6, monotone);
        msl = sl > msl ? sl : msl;
        read_focus_bases[i] = hgeo[i * 6 + 3];
    }
    if (msl > nb + 1 || msl > 32000) RMR_FAIL(RMR_ERR_INVALID, "chunk of %lld bases", (long long)msl);
    if (msl > cap) {  // zero-dwell bases made a chunk wider than the arena was planned for: start over with the exact width
        RMR_HIP(hipStreamSynchronize(e->stream));
        RMR_TRY(plan(msl));
        RMR_TRY(launch_geometry(e, d, 0, chunk_read, dsig, ns, nullptr, nullptr, nullptr));
    }
    const int seq_w = seq_w_of(msl), map_w = map_w_of(msl);
    RMR_TRY(launch_fill(e, d, nc, chunk_read, dsig, dgeo, c.signal, c.seqs, seq_w, c.maps, map_w, c.lens, c.rfb));
    RMR_TRY(run_pipeline(m, ChunkArrays{c.signal, nullptr, c.seqs, seq_w, c.maps, map_w, c.lens, r->kb, r->ka}, nc, dlog));
    RMR_HIP(hipStreamSynchronize(e->stream));
    memcpy(logits, hlog, (size_t)nc * no * 4);
    return 0;
}

int rmr_infer_chunks(rmr_model *m, const float *signal, const int8_t *seqs, int seq_w,
                     const int16_t *maps, int map_w, const int16_t *lens, int kb, int ka, int64_t n,
                     float *logits, int64_t *label_counts, int mem) {
    if (!m || !signal || !seqs || !maps || !lens || !logits) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (kb < 0 || ka < 0 || kb + ka + 1 != m->desc.kmer_len)
        RMR_FAIL(RMR_ERR_INVALID, "kmer context (%d,%d) does not match model kmer_len %d", kb, ka, m->desc.kmer_len);
    if (seq_w < kb + ka + 1 || map_w < 2) RMR_FAIL(RMR_ERR_INVALID, "bad array widths");
    if (n <= 0) return 0;
    rmr_engine *e = m->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    const int no = m->desc.num_out;
    if (mem == RMR_MEM_DEVICE) {
        RMR_TRY(run_pipeline(m, ChunkArrays{signal, nullptr, seqs, seq_w, maps, map_w, lens, kb, ka}, n, logits));
        if (label_counts) RMR_TRY(launch_count(e, logits, n, no, label_counts));
        return 0;
    }
    const size_t L = m->L;
    Stage st;
    float *dsig, *dlog;
    int8_t *ds;
    int16_t *dm, *dl;
    int64_t *dc;
    st.add(&dsig, n * L).add(&ds, (size_t)n * seq_w).add(&dm, (size_t)n * map_w).add(&dl, n).add(&dlog, (size_t)n * no).add(&dc, 16);
    RMR_TRY(st.commit(e));
    const ChunkArrays dev{dsig, nullptr, ds, seq_w, dm, map_w, dl, kb, ka};
    const int64_t hsb = tune_int("RMR_HOST_SUBBATCH", 131072);
    if (hsb > 0 && n > hsb) {
        // pipelined upload: the CPU copies sub-batch i+1 into a pinned slot and the aux stream uploads it
        // while the kernels of sub-batch i run on the main stream
        const size_t o_seq = Stage::pad((size_t)hsb * L * 4), o_map = o_seq + Stage::pad((size_t)hsb * seq_w);
        const size_t o_len = o_map + Stage::pad((size_t)hsb * map_w * 2), slot_b = o_len + Stage::pad((size_t)hsb * 2);
        RMR_TRY(e->ensure_pinned(2 * slot_b));
        const int nthr = 4;
        int64_t idx = 0;
        for (int64_t c0 = 0; c0 < n; c0 += hsb, ++idx) {
            const int64_t nb = (n - c0) < hsb ? (n - c0) : hsb;
            const int slot = (int)(idx & 1);
            char *pb = reinterpret_cast<char *>(e->pinned) + (size_t)slot * slot_b;
            if (idx >= 2) RMR_HIP(hipEventSynchronize(e->ev_h2d[slot]));  // the upload that used this slot is done
            {
                const char *src = reinterpret_cast<const char *>(signal + (size_t)c0 * L);
                const size_t bytes = (size_t)nb * L * 4, part = (bytes / nthr + 4095) & ~(size_t)4095;
                std::vector<std::thread> pool;
                for (int t = 1; t < nthr; ++t) {
                    const size_t b0 = (size_t)t * part;
                    if (b0 < bytes) pool.emplace_back([=] { memcpy(pb + b0, src + b0, std::min(part, bytes - b0)); });
                }
                memcpy(pb, src, std::min(part, bytes));
                memcpy(pb + o_seq, seqs + (size_t)c0 * seq_w, (size_t)nb * seq_w);
                memcpy(pb + o_map, maps + (size_t)c0 * map_w, (size_t)nb * map_w * 2);
                memcpy(pb + o_len, lens + c0, (size_t)nb * 2);
                for (auto &th : pool) th.join();
            }
            RMR_HIP(hipMemcpyAsync(dsig + (size_t)c0 * L, pb, (size_t)nb * L * 4, hipMemcpyHostToDevice, e->aux));
            RMR_HIP(hipMemcpyAsync(ds + (size_t)c0 * seq_w, pb + o_seq, (size_t)nb * seq_w, hipMemcpyHostToDevice, e->aux));
            RMR_HIP(hipMemcpyAsync(dm + (size_t)c0 * map_w, pb + o_map, (size_t)nb * map_w * 2, hipMemcpyHostToDevice, e->aux));
            RMR_HIP(hipMemcpyAsync(dl + c0, pb + o_len, (size_t)nb * 2, hipMemcpyHostToDevice, e->aux));
            RMR_HIP(hipEventRecord(e->ev_h2d[slot], e->aux));
            RMR_HIP(hipStreamWaitEvent(e->stream, e->ev_h2d[slot], 0));
            RMR_TRY(run_pipeline(m, dev.at(c0, (int)L, 0), nb, dlog + (size_t)c0 * no));
        }
    } else {
        H2D(dsig, signal, n * L * 4);
        H2D(ds, seqs, (size_t)n * seq_w);
        H2D(dm, maps, (size_t)n * map_w * 2);
        H2D(dl, lens, (size_t)n * 2);
        RMR_TRY(run_pipeline(m, dev, n, dlog));
    }
    if (label_counts) {
        H2D(dc, label_counts, (size_t)no * 8);
        RMR_TRY(launch_count(e, dlog, n, no, dc));
        D2H(label_counts, dc, (size_t)no * 8);
    }
    D2H(logits, dlog, (size_t)n * no * 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

}  // extern "C"
