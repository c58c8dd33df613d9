// engine.hip — host side of libremora_hip.so: engine/model lifetime, BatchNorm folding and
// MFMA-fragment packing of the weights, the C ABI entry points and the per-kernel HIP-event
// profiler.  See include/remora_hip.h for the contract of every entry point and the
// reference interface (file:line) each one replaces.
#include <dlfcn.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <thread>
#include <algorithm>

#include "rmr_internal.h"
#include "rmr_geometry.h"

namespace rmr {

static thread_local std::string g_err;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

static const char *k_names[K_NUM] = {
    "encode_kmers", "trim_chunk_context", "parse_moves", "normalise_signal", "chunk_geometry",
    "chunk_fill", "front_sig", "front_seq", "seq_conv1_dense", "conv_sig3", "conv_seq2", "conv_seq3",
    "conv_merge1", "conv_merge2", "conv_merge3", "conv_merge4", "lstm_head", "fc_head",
    "count_labels", "motif_scan", "vbz_decode", "refine_band", "refine_dp", "refine_dp_rowwise",
    "fused_front", "rescale_quantiles", "sig3_front", "seq2_front"};
const char *kernel_name(int id) { return (id >= 0 && id < K_NUM) ? k_names[id] : "?"; }

}  // namespace rmr

namespace rmr { void rccl_comm_free(void *comm); }  // defined with the collective at the end of this file

using namespace rmr;

// =========================================================================================
// engine
// =========================================================================================
int rmr_engine::ensure_pinned(size_t bytes) {
    if (bytes <= pinned_cap) return 0;
    if (pinned) {
        RMR_HIP(hipStreamSynchronize(aux));
        RMR_HIP(hipHostFree(pinned));
        pinned = nullptr;
        pinned_cap = 0;
    }
    hipError_t err = hipHostMalloc(&pinned, bytes, hipHostMallocDefault);
    if (err != hipSuccess) {
        pinned = nullptr;
        set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
        return RMR_ERR_HIP;
    }
    pinned_cap = bytes;
    return 0;
}

int rmr_engine::ensure_pin_call(size_t bytes) {
    if (bytes <= pin_call_cap) return 0;
    if (pin_call) {
        RMR_HIP(hipStreamSynchronize(stream));
        RMR_HIP(hipHostFree(pin_call));
        pin_call = nullptr;
        pin_call_cap = 0;
    }
    bytes = bytes + bytes / 2 + (1 << 16);
    hipError_t err = hipHostMalloc(&pin_call, bytes, hipHostMallocDefault);
    if (err != hipSuccess) {
        pin_call = nullptr;
        set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
        return RMR_ERR_HIP;
    }
    pin_call_cap = bytes;
    return 0;
}

int rmr_engine::ensure(Arena &a, size_t bytes) {
    if (bytes <= a.cap) return 0;
    if (a.ptr) {
        RMR_HIP(hipStreamSynchronize(stream));
        RMR_HIP(hipFree(a.ptr));
        a.ptr = nullptr;
        a.cap = 0;
    }
    size_t want = bytes + bytes / 8;
    hipError_t err = hipMalloc(&a.ptr, want);
    if (err != hipSuccess) {
        a.ptr = nullptr;
        set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(err));
        return RMR_ERR_NOMEM;
    }
    a.cap = want;
    return 0;
}

// ---- RMR_POISON (rmr_internal.h) -----------------------------------------------------------------------------------
namespace rmr {
__global__ __launch_bounds__(512) void poison_kernel(int lds_words) {
    extern __shared__ unsigned poison_lds[];
    for (int i = threadIdx.x; i < lds_words; i += 512) poison_lds[i] = 0xFFFFFFFFu;
    // v16 .. v255 of the block's 8 waves (2 per SIMD x 256 registers = the whole file of a SIMD) and s40 .. s95: one move per
    // register, unrolled by the assembler.  The clobber list has to name every register (a range is not accepted).
#define RMR_R10(p, t) p #t "0", p #t "1", p #t "2", p #t "3", p #t "4", p #t "5", p #t "6", p #t "7", p #t "8", p #t "9"
    asm volatile(".set rmr_i, 16\n\t.rept 240\n\tv_mov_b32 v[rmr_i], -1\n\t.set rmr_i, rmr_i + 1\n\t.endr\n\t"
                 ".set rmr_i, 40\n\t.rept 56\n\ts_mov_b32 s[rmr_i], -1\n\t.set rmr_i, rmr_i + 1\n\t.endr\n\t"
                 :
                 :
                 : "v16", "v17", "v18", "v19", RMR_R10("v", 2), RMR_R10("v", 3), RMR_R10("v", 4), RMR_R10("v", 5), RMR_R10("v", 6),
                   RMR_R10("v", 7), RMR_R10("v", 8), RMR_R10("v", 9), RMR_R10("v", 10), RMR_R10("v", 11), RMR_R10("v", 12),
                   RMR_R10("v", 13), RMR_R10("v", 14), RMR_R10("v", 15), RMR_R10("v", 16), RMR_R10("v", 17), RMR_R10("v", 18),
                   RMR_R10("v", 19), RMR_R10("v", 20), RMR_R10("v", 21), RMR_R10("v", 22), RMR_R10("v", 23), RMR_R10("v", 24),
                   "v250", "v251", "v252", "v253", "v254", "v255",
                   RMR_R10("s", 4), RMR_R10("s", 5), RMR_R10("s", 6), RMR_R10("s", 7), RMR_R10("s", 8), "s90", "s91", "s92", "s93", "s94", "s95");
#undef RMR_R10
    __syncthreads();
    if (poison_lds[threadIdx.x] != 0xFFFFFFFFu) __builtin_trap();  // (keeps the stores alive)
}

void poison_before_launch(rmr_engine *e, hipStream_t s) {
    static const int on = tune_int("RMR_POISON", 0);
    if (!on) return;
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(poison_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr = true;
    }
    hipLaunchKernelGGL(poison_kernel, dim3((unsigned)e->num_cus * 2), dim3(512), (size_t)160 * 1024, s, 160 * 256);
}
}  // namespace rmr

int rmr_engine::allow_big_lds(const void *kernel, size_t bytes) {
    for (const void *k : lds_attr_set)
        if (k == kernel) return 0;
    RMR_HIP(hipSetDevice(device));
    RMR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    lds_attr_set.push_back(kernel);
    return 0;
}

int rmr_engine::kernel_regs(const void *kernel) {
    for (const auto &kr : regs_seen)
        if (kr.first == kernel) return kr.second;
    hipFuncAttributes attr;
    const int regs = hipFuncGetAttributes(&attr, kernel) == hipSuccess && attr.numRegs > 0 ? attr.numRegs : 256;
    regs_seen.emplace_back(kernel, regs);
    return regs;
}

int rmr_engine::prof_begin(int id, hipEvent_t *t1, hipStream_t s) {
    hipEvent_t ev[2];
    for (int k = 0; k < 2; ++k) {
        if (!pool.empty()) {
            ev[k] = pool.back();
            pool.pop_back();
        } else if (hipEventCreate(&ev[k]) != hipSuccess) {
            return -1;
        }
    }
    if (hipEventRecord(ev[0], s) != hipSuccess) return -1;
    recs.push_back(Rec{id, ev[0], ev[1]});
    *t1 = ev[1];
    return 0;
}

int rmr_engine::prof_collect() {
    if (recs.empty()) return 0;
    RMR_HIP(hipStreamSynchronize(stream));
    if (aux) RMR_HIP(hipStreamSynchronize(aux));
    for (auto &r : recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.t0, r.t1) == hipSuccess) {
            acc_ms[r.id] += ms;
            acc_n[r.id] += 1;
        }
        pool.push_back(r.t0);
        pool.push_back(r.t1);
    }
    recs.clear();
    return 0;
}

extern "C" {

const char *rmr_last_error(void) { return g_err.c_str(); }
const char *rmr_version(void) { return "remora_hip 0.5 (gfx950)"; }  // 0.5: rmr_call_read, rmr_engine_wait_for

int rmr_engine_create(int device, void *stream, int flags, rmr_engine **out) {
    if (!out) RMR_FAIL(RMR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev == 0) {
        set_error("no HIP device available (%s)", hipGetErrorString(err));
        return RMR_ERR_HIP;
    }
    if (device < 0 || device >= ndev) RMR_FAIL(RMR_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    RMR_HIP(hipSetDevice(device));
    std::unique_ptr<rmr_engine> e(new rmr_engine());
    e->device = device;
    hipDeviceProp_t prop;
    RMR_HIP(hipGetDeviceProperties(&prop, device));
    e->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (flags & RMR_ENGINE_USE_STREAM) {
        e->stream = reinterpret_cast<hipStream_t>(stream);
    } else {
        // an engine with a stream of its own is a helper beside the model's engine (chunk extraction, ingest decodes): short
        // kernels whose results somebody waits for - the highest priority the device offers, so that they are dispatched
        // ahead of queued work of the long model kernels wherever the hardware has a choice
        int prio_lo = 0, prio_hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
        if (hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, prio_hi) != hipSuccess)
            RMR_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        e->owns_stream = true;
    }
    RMR_HIP(hipStreamCreateWithFlags(&e->aux, hipStreamNonBlocking));
    RMR_HIP(hipEventCreateWithFlags(&e->ev_handoff, hipEventDisableTiming));
    for (int k = 0; k < 2; ++k) {
        RMR_HIP(hipEventCreateWithFlags(&e->ev_h2d[k], hipEventDisableTiming));
    }
    *out = e.release();
    return 0;
}

void rmr_engine_destroy(rmr_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (e->aux) { (void)hipStreamSynchronize(e->aux); (void)hipStreamDestroy(e->aux); }
    if (e->ev_handoff) (void)hipEventDestroy(e->ev_handoff);
    for (int k = 0; k < 2; ++k) {
        if (e->ev_h2d[k]) (void)hipEventDestroy(e->ev_h2d[k]);
    }
    if (e->comm) {
        rmr::rccl_comm_free(e->comm);
        e->comm = nullptr;
    }
    if (e->pinned) (void)hipHostFree(e->pinned);
    if (e->pin_call) (void)hipHostFree(e->pin_call);
    for (auto &r : e->recs) { (void)hipEventDestroy(r.t0); (void)hipEventDestroy(r.t1); }
    for (auto ev : e->pool) (void)hipEventDestroy(ev);
    if (e->act.ptr) (void)hipFree(e->act.ptr);
    if (e->staging.ptr) (void)hipFree(e->staging.ptr);
    if (e->owns_stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

int rmr_engine_synchronize(rmr_engine *e) {
    if (!e) RMR_FAIL(RMR_ERR_INVALID, "engine is NULL");
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_engine_wait_for(rmr_engine *waiter, rmr_engine *producer) {
    if (!waiter || !producer) RMR_FAIL(RMR_ERR_INVALID, "engine is NULL");
    if (waiter == producer || waiter->stream == producer->stream) return 0;
    if (waiter->device != producer->device) RMR_FAIL(RMR_ERR_INVALID, "engines on different devices");
    {
        std::lock_guard<std::mutex> lk(producer->mu);
        RMR_HIP(hipSetDevice(producer->device));
        RMR_HIP(hipEventRecord(producer->ev_handoff, producer->stream));
    }
    std::lock_guard<std::mutex> lk(waiter->mu);
    RMR_HIP(hipStreamWaitEvent(waiter->stream, producer->ev_handoff, 0));
    return 0;
}

int rmr_engine_set_subbatch(rmr_engine *e, int64_t chunks) {
    if (!e || chunks < 0) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    e->subbatch = chunks;
    return 0;
}

int rmr_profile_enable(rmr_engine *e, int on) {
    if (!e) RMR_FAIL(RMR_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_TRY(e->prof_collect());
    e->profiling = on != 0;
    return 0;
}
int rmr_profile_reset(rmr_engine *e) {
    if (!e) RMR_FAIL(RMR_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_TRY(e->prof_collect());
    for (int i = 0; i < K_NUM; ++i) { e->acc_ms[i] = 0; e->acc_n[i] = 0; }
    return 0;
}
int rmr_profile_num_kernels(void) { return K_NUM; }
const char *rmr_profile_kernel_name(int id) { return kernel_name(id); }
int rmr_profile_get(rmr_engine *e, int id, double *total_ms, int64_t *launches) {
    if (!e || id < 0 || id >= K_NUM) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_TRY(e->prof_collect());
    if (total_ms) *total_ms = e->acc_ms[id];
    if (launches) *launches = e->acc_n[id];
    return 0;
}

}  // extern "C"

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
    if (sp == desc->size) return model_create_at_kernel_size(e, desc, weights, n_floats, out);
    rmr_model_desc pd = *desc;
    pd.size = sp;
    const std::vector<float> blob = pad_model_blob(*desc, weights, sp);
    RMR_TRY(model_create_at_kernel_size(e, &pd, blob.data(), blob.size(), out));
    (*out)->true_size = desc->size;
    return 0;
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
// fused pipeline
// =========================================================================================
namespace {

size_t act_floats_per_chunk(const rmr_model *m) {
    const size_t sz = m->desc.size;
    size_t n = (size_t)m->P1 * 16 + (size_t)m->P2 * 16 + (size_t)m->P3 * 2 * sz;
    if (m->desc.arch == RMR_ARCH_CONV_LSTM) {
        n += (size_t)m->T * sz;
    } else {
        n += (size_t)m->PQ2 * 32 + (size_t)(m->T + m->T2 + m->T3 + m->T4) * sz;
    }
    return n;
}

// enc != nullptr: dense seqs path; otherwise gather path from (seqs, maps, lens)
int run_pipeline(rmr_model *m, const float *signal, const float *enc, const int8_t *seqs, int seq_w,
                 const int16_t *maps, int map_w, const int16_t *lens, int kb, int ka, int64_t n,
                 float *logits) {
    rmr_engine *e = m->eng;
    if (n <= 0) return 0;
    // the switches of every kernel choice below, read once per call
    const FwdSwitches sw{tune_int("RMR_FUSED", 1) != 0, tune_int("RMR_CONV_FRONT", 1) != 0, tune_int("RMR_WINOGRAD", 1) != 0,
                         tune_int("RMR_SIG3_MFMA", 1) != 0};
    if (m->nparts == 1 && m->desc.size > 64) {
        // bf16 / f16 above 64 channels (k_stream16.hip): fp32 front kernels (sig_conv1/2, seq_conv1: 16 channels), then the three
        // size-wide convolutions and the LSTM on the 16-bit matrix cores with streamed weights; cat and x are 16-bit in HBM
        const int sz = m->desc.size, L = m->L, EC = 4 * m->desc.kmer_len;
        int64_t sb = e->subbatch > 0 ? e->subbatch : 131072;
        if (sb > n) sb = n;
        const size_t front_fl = (size_t)(m->P1 + m->P2) * 16;
        const size_t cat_el = (size_t)m->P3 * 2 * sz, x_el = (size_t)m->T * sz;
        RMR_TRY(e->ensure(e->act, (front_fl * sizeof(float) + (cat_el + x_el) * sizeof(uint16_t) + 64) * sb));
        float *seq1 = reinterpret_cast<float *>(e->act.ptr);
        for (int64_t c0 = 0; c0 < n; c0 += sb) {
            const int64_t nb = (n - c0) < sb ? (n - c0) : sb;
            float *sig2 = seq1 + (size_t)nb * m->P1 * 16;
            uint16_t *cat = reinterpret_cast<uint16_t *>(seq1 + front_fl * sb);
            uint16_t *x16 = cat + cat_el * sb + 32;
            const float *sig_b = signal + (size_t)c0 * L;
            if (enc) {
                RMR_TRY(launch_front(m, e->stream, sig_b, nullptr, 0, nullptr, 0, nullptr, 0, 0, nb, sig2, nullptr));
                RMR_TRY(launch_seq1_dense(m, enc + (size_t)c0 * EC * L, nb, seq1));
            } else {
                RMR_TRY(launch_front(m, e->stream, sig_b, seqs + (size_t)c0 * seq_w, seq_w, maps + (size_t)c0 * map_w, map_w, lens + c0, kb, ka, nb,
                                     sig2, seq1));
            }
            RMR_TRY(launch_conv_stream16(m, m->sig3, sig2, false, m->P2, cat, 2 * sz, 0, m->P3, nb));
            RMR_TRY(launch_conv_stream16(m, m->seq2, seq1, false, m->P1, cat, 2 * sz, sz, m->P3, nb));
            RMR_TRY(launch_conv_stream16(m, m->merge1, cat, true, m->P3, x16, sz, 0, m->T, nb));
            RMR_TRY(launch_lstm_stream16(m, x16, nb, logits + (size_t)c0 * m->desc.num_out));
        }
        return 0;
    }
    if (m->f16 && (enc || !fused_front_supported(m, seq_w, map_w)))
        RMR_FAIL(RMR_ERR_INVALID, "dtype f16 runs on the fused kernels only: chunk arrays (not a dense one-hot tensor), sequence rows of at "
                                  "most 256 columns, a chunk length that is a multiple of 4");
    if (!enc && fused_front_supported(m, seq_w, map_w) && (m->f16 || sw.fused)) {
        // plain-bf16 ConvLSTM: two launches per sub-batch, x (bf16, 3 KB/chunk @C100) is the only intermediate in
        // HBM; sub-batches are sized so that x stays in the 256 MiB Infinity Cache between producer and consumer
        int64_t sb = e->subbatch > 0 ? e->subbatch : 65536;
        if (sb > n) sb = n;
        const size_t x_elems = (size_t)m->T * m->desc.size;
        RMR_TRY(e->ensure(e->act, x_elems * sb * sizeof(uint16_t)));
        uint16_t *x16 = reinterpret_cast<uint16_t *>(e->act.ptr);
        for (int64_t c0 = 0; c0 < n; c0 += sb) {
            const int64_t nb = (n - c0) < sb ? (n - c0) : sb;
            RMR_TRY(launch_fused_front(m, signal + (size_t)c0 * m->L, seqs + (size_t)c0 * seq_w, seq_w,
                                       maps + (size_t)c0 * map_w, map_w, lens + c0, nb, x16));
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
            if (abl_int("RMR_DEBUG_SKIP_LSTM", 0)) continue;  // the front kernel alone (x through RMR_FUSED_DUMP_X)
#endif
            RMR_TRY(launch_lstm_head_x16(m, x16, nb, logits + (size_t)c0 * m->desc.num_out));
        }
        return 0;
    }
    const size_t per = act_floats_per_chunk(m);
    // 262144 chunks per sub-batch: the tail of every persistent-block kernel is paid half as often as with 131072
    // (+1.2 % measured; 524288: +0.2 % more for twice the 5.5 GB arena)
    int64_t sb = e->subbatch > 0 ? e->subbatch : 262144;
    if (sb > n) sb = n;
    const int sz = m->desc.size, L = m->L, EC = 4 * m->desc.kmer_len;
    // fp32 ConvLSTM size 64 straight from the chunk arrays: sig_conv1/2 and seq_conv1 are produced inside the staging of
    // sig_conv3 / seq_conv2 (k_conv_front.hip); sig2 / seq1 never exist in HBM.  (RMR_CONV_FRONT=0: the separate front
    // kernels - the comparand of tests/test_gpu_conv_front.py)
    const bool fold = !enc && sw.conv_front && conv_front_supported(m, kb, ka, seq_w, map_w);
    // every other fp32 path (Conv_w_ref; ConvLSTM shapes the two-branch fold does not cover): the signal branch alone is
    // folded - sig_conv1 / sig_conv2 (matrix cores) produced inside the staging of sig_conv3, sig2 never in HBM
    const bool sigfold = !fold && m->nparts == 0 && sw.sig3_mfma && sig3_front_mfma_supported(m);
    // (Running the front kernels of sub-batch i + 1 on a second stream under the matrix kernels of sub-batch i was measured in
    //  rounds 1-2 in two forms and gained nothing - they share the CUs with conv_sig3, or half a register file under the LSTM -
    //  and is gone; profiles/NOTES_r03.md.)
    const size_t front_fl = fold ? 0 : (size_t)(m->P1 + m->P2) * 16;
    RMR_TRY(e->ensure(e->act, (per + front_fl) * sb * sizeof(float)));
    float *arena = reinterpret_cast<float *>(e->act.ptr);
    float *seq1 = arena, *rest = arena + front_fl * sb;
    const bool split_conv = m->nparts > 0;
    for (int64_t c0 = 0; c0 < n; c0 += sb) {
        const int64_t nb = (n - c0) < sb ? (n - c0) : sb;
        float *sig2 = seq1 + (size_t)nb * m->P1 * 16;
        const float *sig_b = signal + (size_t)c0 * L;
        if (!fold) {  // sig_conv1/2 -> sig2, seq_conv1 -> seq1 (k_front.hip)
            if (enc) {
                if (!sigfold) RMR_TRY(launch_front(m, e->stream, sig_b, nullptr, 0, nullptr, 0, nullptr, 0, 0, nb, sig2, nullptr));
                RMR_TRY(launch_seq1_dense(m, enc + (size_t)c0 * EC * L, nb, seq1));
            } else {
                RMR_TRY(launch_front(m, e->stream, sig_b, seqs + (size_t)c0 * seq_w, seq_w, maps + (size_t)c0 * map_w, map_w, lens + c0, kb, ka,
                                     nb, sigfold ? nullptr : sig2, seq1));
            }
        }
        float *base = rest;
        float *cat = base; base += (size_t)nb * m->P3 * 2 * sz;
        if (fold) RMR_TRY(launch_conv_front(m, sig_b, seqs + (size_t)c0 * seq_w, seq_w, maps + (size_t)c0 * map_w, map_w, lens + c0, nb, cat, sw));
        else if (split_conv) RMR_TRY(launch_conv_split(e, m->sig3, m->nparts, sig2, 16, m->P2, cat, 2 * sz, 0, m->P3, nb));
        else if (sigfold) RMR_TRY(launch_sig3_front_mfma(m, sig_b, nb, cat, sw.winograd));
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
            if (m->nparts > 0 && lstm_x16s_supported(m)) RMR_TRY(launch_lstm_head_x16s(m, x, nb, logits + (size_t)c0 * m->desc.num_out));
            else if (m->nparts > 0) RMR_TRY(launch_lstm_head_split(m, x, nb, logits + (size_t)c0 * m->desc.num_out));
            else RMR_TRY(launch_lstm_head(m, x, nb, logits + (size_t)c0 * m->desc.num_out));
        } else {
            float *seq2 = base; base += (size_t)nb * m->PQ2 * 32;
            float *m1 = base; base += (size_t)nb * m->T * sz;
            float *m2 = base; base += (size_t)nb * m->T2 * sz;
            float *m3 = base; base += (size_t)nb * m->T3 * sz;
            float *m4 = base; base += (size_t)nb * m->T4 * sz;
            RMR_TRY(launch_conv(e, m->seq2, seq1, 16, m->P1, seq2, 32, 0, m->PQ2, nb, sw.winograd));
            RMR_TRY(launch_conv(e, m->seq3, seq2, 32, m->PQ2, cat, 2 * sz, sz, m->P3, nb, sw.winograd));
            RMR_TRY(launch_conv(e, m->merge1, cat, 2 * sz, m->P3, m1, sz, 0, m->T, nb, sw.winograd));
            RMR_TRY(launch_conv(e, m->merge2, m1, sz, m->T, m2, sz, 0, m->T2, nb, sw.winograd));
            RMR_TRY(launch_conv(e, m->merge3, m2, sz, m->T2, m3, sz, 0, m->T3, nb, sw.winograd));
            RMR_TRY(launch_conv(e, m->merge4, m3, sz, m->T3, m4, sz, 0, m->T4, nb, sw.winograd));
            RMR_TRY(launch_fc_head(m, m4, nb, logits + (size_t)c0 * m->desc.num_out));
        }
    }
    return 0;
}

// host <-> device staging helper: a bump allocator over the engine's staging arena
struct Stage {
    rmr_engine *e;
    char *base = nullptr;
    size_t off = 0, cap = 0;
    int init(size_t bytes) {
        RMR_TRY(e->ensure(e->staging, bytes));
        base = reinterpret_cast<char *>(e->staging.ptr);
        cap = bytes;
        return 0;
    }
    template <typename T>
    T *take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T *p = reinterpret_cast<T *>(base + off);
        off += count * sizeof(T);
        return p;
    }
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
};

#define H2D(dst, src, bytes) do { if ((bytes) > 0) RMR_HIP(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, e->stream)); } while (0)
#define D2H(dst, src, bytes) do { if ((bytes) > 0) RMR_HIP(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, e->stream)); } while (0)

}  // namespace

extern "C" {

int rmr_encode_kmers(rmr_engine *e, int kb, int ka, const int8_t *seqs, int seq_w,
                     const int16_t *maps, int map_w, const int16_t *lens, int64_t n, int sig_len,
                     float *out, int mem) {
    if (!e || !seqs || !maps || !lens || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (kb < 0 || ka < 0 || n < 0 || sig_len <= 0 || seq_w <= 0 || map_w <= 0)
        RMR_FAIL(RMR_ERR_INVALID, "bad sizes");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    const size_t out_b = (size_t)n * 4 * (kb + ka + 1) * sig_len * sizeof(float);
    if (mem == RMR_MEM_DEVICE) return launch_encode(e, kb, ka, seqs, seq_w, maps, map_w, lens, n, sig_len, out);
    Stage st{e};
    RMR_TRY(st.init(Stage::pad(n * seq_w) + Stage::pad(n * map_w * 2) + Stage::pad(n * 2) + Stage::pad(out_b) + 1024));
    int8_t *ds = st.take<int8_t>(n * seq_w);
    int16_t *dm = st.take<int16_t>(n * map_w);
    int16_t *dl = st.take<int16_t>(n);
    float *dout = st.take<float>(out_b / 4);
    H2D(ds, seqs, (size_t)n * seq_w);
    H2D(dm, maps, (size_t)n * map_w * 2);
    H2D(dl, lens, (size_t)n * 2);
    RMR_TRY(launch_encode(e, kb, ka, ds, seq_w, dm, map_w, dl, n, sig_len, dout));
    D2H(out, dout, out_b);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_trim_chunk_context(rmr_engine *e, int sb, int sa, int cb, int ca, int tsc, int8_t *seqs,
                           int seq_w, int16_t *maps, int map_w, int16_t *lens, int64_t n, int mem) {
    if (!e || !seqs || !maps || !lens) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE) return launch_trim(e, sb, sa, cb, ca, tsc, seqs, seq_w, maps, map_w, lens, n);
    Stage st{e};
    RMR_TRY(st.init(Stage::pad(n * seq_w) + Stage::pad(n * map_w * 2) + Stage::pad(n * 2) + 1024));
    int8_t *ds = st.take<int8_t>(n * seq_w);
    int16_t *dm = st.take<int16_t>(n * map_w);
    int16_t *dl = st.take<int16_t>(n);
    H2D(ds, seqs, (size_t)n * seq_w);
    H2D(dm, maps, (size_t)n * map_w * 2);
    H2D(dl, lens, (size_t)n * 2);
    RMR_TRY(launch_trim(e, sb, sa, cb, ca, tsc, ds, seq_w, dm, map_w, dl, n));
    D2H(seqs, ds, (size_t)n * seq_w);
    D2H(maps, dm, (size_t)n * map_w * 2);
    D2H(lens, dl, (size_t)n * 2);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_parse_moves(rmr_engine *e, const int8_t *mv_tag, int64_t mv_tag_len, int64_t sig_len,
                    int64_t seq_len, int check, int reverse_signal, int64_t *q2s, int64_t *n_out,
                    int mem) {
    if (!e || !mv_tag || !q2s || !n_out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (mv_tag_len < 1) RMR_FAIL(RMR_ERR_INVALID, "empty move tag");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    Stage st{e};
    RMR_TRY(st.init(Stage::pad(mv_tag_len) + Stage::pad((mv_tag_len + 1) * 8) + 2048));
    int64_t *dcount = st.take<int64_t>(1);
    int8_t stride_h = 0;
    const int8_t *dmv = mv_tag;
    int64_t *dq = q2s;
    if (mem == RMR_MEM_HOST) {
        int8_t *t = st.take<int8_t>(mv_tag_len);
        H2D(t, mv_tag, (size_t)mv_tag_len);
        dmv = t;
        dq = st.take<int64_t>(mv_tag_len + 1);
        stride_h = mv_tag[0];
    } else {
        RMR_HIP(hipMemcpyAsync(&stride_h, mv_tag, 1, hipMemcpyDeviceToHost, e->stream));
    }
    RMR_TRY(launch_moves(e, dmv, mv_tag_len, sig_len, reverse_signal, dq, dcount));
    int64_t cnt = 0;
    D2H(&cnt, dcount, 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    if (mem == RMR_MEM_HOST) {
        RMR_HIP(hipMemcpy(q2s, dq, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    }
    *n_out = cnt;
    if (stride_h <= 0) RMR_FAIL(RMR_ERR_INVALID, "move table stride %d", (int)stride_h);
    if (check && seq_len >= 0 && cnt - 1 != seq_len) {
        set_error("Move table discordant with basecalls");
        return RMR_ERR_DISCORDANT_SEQ;
    }
    if (check && (mv_tag_len - 1) != sig_len / stride_h) {
        set_error("Move table discordant with signal");
        return RMR_ERR_DISCORDANT_SIG;
    }
    return 0;
}

int rmr_parse_moves_batch(rmr_engine *e, const int8_t *mv_tags, const int64_t *mv_off, const int64_t *sig_len,
                          const int64_t *seq_len, int64_t n_reads, int check, int reverse_signal, int64_t *q2s,
                          int64_t *counts, int32_t *status, int mem) {
    if (!e || !mv_tags || !mv_off || !sig_len || !seq_len || !q2s || !counts || !status)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE)
        return launch_moves_batch(e, mv_tags, mv_off, sig_len, seq_len, n_reads, check, reverse_signal, q2s, counts, status);
    const int64_t total = mv_off[n_reads];
    if (mv_off[0] != 0 || total < n_reads) RMR_FAIL(RMR_ERR_INVALID, "bad move table offsets");
    Stage st{e};
    RMR_TRY(st.init(Stage::pad(total) + Stage::pad((size_t)total * 8) + 5 * Stage::pad((size_t)(n_reads + 1) * 8) + 4096));
    int8_t *dmv = st.take<int8_t>(total);
    int64_t *doff = st.take<int64_t>(n_reads + 1);
    int64_t *dsl = st.take<int64_t>(n_reads);
    int64_t *dql = st.take<int64_t>(n_reads);
    int64_t *dq = st.take<int64_t>(total);
    int64_t *dcnt = st.take<int64_t>(n_reads);
    int32_t *dst = st.take<int32_t>(n_reads);
    H2D(dmv, mv_tags, (size_t)total);
    H2D(doff, mv_off, (size_t)(n_reads + 1) * 8);
    H2D(dsl, sig_len, (size_t)n_reads * 8);
    H2D(dql, seq_len, (size_t)n_reads * 8);
    RMR_TRY(launch_moves_batch(e, dmv, doff, dsl, dql, n_reads, check, reverse_signal, dq, dcnt, dst));
    D2H(q2s, dq, (size_t)total * 8);
    D2H(counts, dcnt, (size_t)n_reads * 8);
    D2H(status, dst, (size_t)n_reads * 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_signal_histograms(rmr_engine *e, const int16_t *signal, const int64_t *start, const int64_t *len, int64_t n, int32_t *lo, int32_t *hi,
                          const int64_t *hist_off, uint32_t *hist) {
    if (!e || !signal || !start || !len || !lo || !hi || (hist != nullptr) != (hist_off != nullptr)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n < 0 || n > (int64_t)1 << 24) RMR_FAIL(RMR_ERR_INVALID, "bad n");
    if (n == 0) return 0;
    for (int64_t i = 0; i < n; ++i)
        if (start[i] < 0 || len[i] < 0) RMR_FAIL(RMR_ERR_INVALID, "span %lld: negative extent", (long long)i);
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    const size_t nn = (size_t)n;
    Stage st{e};
    if (!hist) {  // pass 1: the range of every span
        RMR_TRY(st.init(2 * Stage::pad(nn * 8) + 2 * Stage::pad(nn * 4) + 4096));
        int64_t *d_start = st.take<int64_t>(nn), *d_len = st.take<int64_t>(nn);
        int32_t *d_lo = st.take<int32_t>(nn), *d_hi = st.take<int32_t>(nn);
        H2D(d_start, start, nn * 8);
        H2D(d_len, len, nn * 8);
        RMR_TRY(launch_signal_range(e, signal, d_start, d_len, n, d_lo, d_hi));
        D2H(lo, d_lo, nn * 4);
        D2H(hi, d_hi, nn * 4);
        RMR_HIP(hipStreamSynchronize(e->stream));
        return 0;
    }
    // pass 2: counts over [lo, hi] of every span, at the offsets the caller summed up
    if (hist_off[0] != 0) RMR_FAIL(RMR_ERR_INVALID, "hist_off[0] != 0");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t width = len[i] > 0 ? (int64_t)hi[i] - lo[i] + 1 : 0;
        if (hist_off[i + 1] - hist_off[i] != (width > 0 ? width : 0)) RMR_FAIL(RMR_ERR_INVALID, "span %lld: hist_off does not match hi - lo + 1", (long long)i);
    }
    const size_t total = (size_t)hist_off[n];
    if (total == 0) return 0;
    RMR_TRY(st.init(2 * Stage::pad(nn * 8) + Stage::pad(nn * 4) + Stage::pad((nn + 1) * 8) + Stage::pad(total * 4) + 4096));
    int64_t *d_start = st.take<int64_t>(nn), *d_len = st.take<int64_t>(nn);
    int32_t *d_lo = st.take<int32_t>(nn);
    int64_t *d_off = st.take<int64_t>(nn + 1);
    uint32_t *d_hist = st.take<uint32_t>(total);
    H2D(d_start, start, nn * 8);
    H2D(d_len, len, nn * 8);
    H2D(d_lo, lo, nn * 4);
    H2D(d_off, hist_off, (nn + 1) * 8);
    RMR_HIP(hipMemsetAsync(d_hist, 0, total * 4, e->stream));
    RMR_TRY(launch_signal_hist(e, signal, d_start, d_len, d_lo, d_off, n, d_hist));
    D2H(hist, d_hist, total * 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_assemble_reads(rmr_engine *e, int64_t n_reads, const int16_t *signal, const int64_t *src_start, const int64_t *q2s,
                       const int64_t *q2s_off, const int64_t *seq_len, int16_t *dacs, int64_t dacs_cap, int64_t *s2s,
                       int64_t *d_sig_off, int64_t *d_seq_off, int64_t *sig_off) {
    if (!e || !signal || !src_start || !q2s || !q2s_off || !seq_len || !dacs || !s2s || !d_sig_off || !d_seq_off || !sig_off)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0) RMR_FAIL(RMR_ERR_INVALID, "bad sizes");
    sig_off[0] = 0;
    if (n_reads == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    const size_t n = (size_t)n_reads;
    Stage st{e};
    RMR_TRY(st.init(4 * Stage::pad(n * 8) + 4096));
    int64_t *d_start = st.take<int64_t>(n), *d_qoff = st.take<int64_t>(n), *d_slen = st.take<int64_t>(n), *d_len = st.take<int64_t>(n);
    H2D(d_start, src_start, n * 8);
    H2D(d_qoff, q2s_off, n * 8);
    H2D(d_slen, seq_len, n * 8);
    RMR_TRY(launch_assemble_lengths(e, q2s, d_qoff, d_slen, n_reads, d_len));
    std::vector<int64_t> len(n), seq_off(n + 1, 0);
    D2H(len.data(), d_len, n * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < n; ++i) {
        if (len[i] < 0 || seq_len[i] < 0) RMR_FAIL(RMR_ERR_INVALID, "read %zu: a mapping that runs backwards", i);
        sig_off[i + 1] = sig_off[i] + len[i];
        seq_off[i + 1] = seq_off[i] + seq_len[i];
    }
    if (sig_off[n] > dacs_cap) RMR_FAIL(RMR_ERR_INVALID, "dacs capacity %lld < %lld samples", (long long)dacs_cap, (long long)sig_off[n]);
    H2D(d_sig_off, sig_off, (n + 1) * 8);
    H2D(d_seq_off, seq_off.data(), (n + 1) * 8);
    RMR_TRY(launch_assemble_reads(e, signal, d_start, q2s, d_qoff, d_sig_off, d_seq_off, n_reads, dacs, s2s));
    RMR_HIP(hipStreamSynchronize(e->stream));  // (the pageable offset vectors above are read by the copies)
    return 0;
}

}  // extern "C"

// ---- chunk extraction ------------------------------------------------------------------------
namespace {

// device-side copy of an rmr_reads whose arrays live on the host
struct DevReads {
    rmr_reads d{};
    int32_t *chunk_read = nullptr;
    int32_t *sig_read = nullptr;
    int64_t n_chunks = 0, total_sig = 0, total_bases = 0;
};

int read_offsets_host(rmr_engine *e, const rmr_reads *r, int mem, std::vector<int64_t> &sig_off,
                      std::vector<int64_t> &seq_off, std::vector<int64_t> &foc_off) {
    const size_t n1 = (size_t)r->n_reads + 1;
    sig_off.resize(n1); seq_off.resize(n1); foc_off.resize(n1);
    if (mem == RMR_MEM_HOST) {
        memcpy(sig_off.data(), r->sig_off, n1 * 8);
        memcpy(seq_off.data(), r->seq_off, n1 * 8);
        memcpy(foc_off.data(), r->focus_off, n1 * 8);
    } else if (r->host_sig_off && r->host_seq_off && r->host_focus_off) {
        // the caller kept host copies of the offsets: three small device-to-host copies (and their syncs) saved per call
        memcpy(sig_off.data(), r->host_sig_off, n1 * 8);
        memcpy(seq_off.data(), r->host_seq_off, n1 * 8);
        memcpy(foc_off.data(), r->host_focus_off, n1 * 8);
    } else {
        RMR_HIP(hipMemcpy(sig_off.data(), r->sig_off, n1 * 8, hipMemcpyDeviceToHost));
        RMR_HIP(hipMemcpy(seq_off.data(), r->seq_off, n1 * 8, hipMemcpyDeviceToHost));
        RMR_HIP(hipMemcpy(foc_off.data(), r->focus_off, n1 * 8, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i + 1 < n1; ++i)
        if (sig_off[i + 1] < sig_off[i] || seq_off[i + 1] < seq_off[i] || foc_off[i + 1] < foc_off[i])
            RMR_FAIL(RMR_ERR_INVALID, "offsets of read %zu are not increasing", i);
    if (sig_off[0] != 0 || seq_off[0] != 0 || foc_off[0] != 0) RMR_FAIL(RMR_ERR_INVALID, "offsets must start at 0");
    return 0;
}

int stage_reads(rmr_engine *e, Stage &st, const rmr_reads *r, int mem, bool need_dacs, const std::vector<int64_t> &sig_off,
                const std::vector<int64_t> &seq_off, const std::vector<int64_t> &foc_off, DevReads *o) {
    const int64_t nr = r->n_reads;
    o->total_sig = sig_off[nr];
    o->total_bases = seq_off[nr];
    o->n_chunks = foc_off[nr];
    o->d = *r;
    o->chunk_read = st.take<int32_t>(o->n_chunks + 1);
    if (mem == RMR_MEM_DEVICE) {
        // device-resident batch: the read index of every chunk comes from the offsets where they are - no host loop, no
        // upload, no wait (a batch of the reads pipeline paid two of these round trips per extraction, each behind whatever
        // the GPU was running)
        return launch_chunk_read(e, r->focus_off, nr, o->n_chunks, o->chunk_read);
    }
    // read index per chunk (host-built, tiny next to the data itself)
    std::vector<int32_t> cr((size_t)o->n_chunks);
    for (int64_t k = 0; k < nr; ++k)
        for (int64_t i = foc_off[k]; i < foc_off[k + 1]; ++i) cr[(size_t)i] = (int32_t)k;
    H2D(o->chunk_read, cr.data(), cr.size() * 4);
    if (mem == RMR_MEM_HOST) {
#define STAGE_ARR(field, T, count)                                        \
    {                                                                     \
        T *d_ = st.take<T>((count) + 1);                                  \
        H2D(d_, r->field, (size_t)(count) * sizeof(T));                   \
        o->d.field = d_;                                                  \
    }
        if (need_dacs) STAGE_ARR(dacs, int16_t, o->total_sig)
        STAGE_ARR(sig_off, int64_t, nr + 1)
        STAGE_ARR(seq_to_sig, int64_t, o->total_bases + nr)
        STAGE_ARR(int_seq, int8_t, o->total_bases)
        STAGE_ARR(seq_off, int64_t, nr + 1)
        STAGE_ARR(shift, double, nr)
        STAGE_ARR(scale, double, nr)
        STAGE_ARR(focus_bases, int64_t, o->n_chunks)
        STAGE_ARR(focus_off, int64_t, nr + 1)
#undef STAGE_ARR
    }
    // the H2D copies above read from host vectors that die with this frame
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

size_t reads_stage_bytes(const rmr_reads *r, int64_t total_sig, int64_t total_bases, int64_t n_chunks) {
    const int64_t nr = r->n_reads;
    return Stage::pad(total_sig * 2) + Stage::pad(total_sig * 4 + 8) + 4 * Stage::pad((nr + 2) * 8) +
           Stage::pad((total_bases + nr + 1) * 8) + Stage::pad(total_bases + 1) + 2 * Stage::pad((nr + 1) * 8) +
           Stage::pad((n_chunks + 1) * 8) + Stage::pad((n_chunks + 1) * 4) + 8192;
}

}  // namespace

extern "C" {

int rmr_chunk_geometry(rmr_engine *e, const rmr_reads *reads, float *sig_out, int64_t *geo,
                       int64_t *max_seq_len, int mem) {
    if (!e || !reads || !sig_out || !geo || !max_seq_len) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (reads->n_reads < 0) RMR_FAIL(RMR_ERR_INVALID, "n_reads < 0");
    *max_seq_len = 0;
    if (reads->n_reads == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::vector<int64_t> so, qo, fo;
    RMR_TRY(read_offsets_host(e, reads, mem, so, qo, fo));
    const int64_t nr = reads->n_reads, ts = so[nr], tb = qo[nr], nc = fo[nr];
    Stage st{e};
    RMR_TRY(st.init(reads_stage_bytes(reads, ts, tb, nc) + Stage::pad(ts * 4) + Stage::pad(nc * 48) + 4096));
    DevReads dr;
    RMR_TRY(stage_reads(e, st, reads, mem, true, so, qo, fo, &dr));
    int *dmax = st.take<int>(4);
    RMR_HIP(hipMemsetAsync(dmax, 0, 16, e->stream));
    float *dsig = sig_out;
    int64_t *dgeo = geo;
    if (mem == RMR_MEM_HOST) {
        dsig = st.take<float>(ts + 1);
        dgeo = st.take<int64_t>(nc * 6 + 1);
    }
    RMR_TRY(launch_geometry(e, dr.d, nc, dr.chunk_read, dsig, ts, dr.sig_read, dgeo, dmax));
    int hmax = 0;
    D2H(&hmax, dmax, 4);
    if (mem == RMR_MEM_HOST) {
        D2H(sig_out, dsig, (size_t)ts * 4);
        D2H(geo, dgeo, (size_t)nc * 48);
    }
    RMR_HIP(hipStreamSynchronize(e->stream));
    *max_seq_len = hmax;
    return 0;
}

int rmr_chunk_fill(rmr_engine *e, const rmr_reads *reads, const float *sig, const int64_t *geo,
                   float *signal, int8_t *seqs, int seq_w, int16_t *maps, int map_w, int16_t *lens,
                   int64_t *read_focus_bases, int mem) {
    if (!e || !reads || !sig || !geo || !signal || !seqs || !maps || !lens || !read_focus_bases)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (reads->n_reads <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::vector<int64_t> so, qo, fo;
    RMR_TRY(read_offsets_host(e, reads, mem, so, qo, fo));
    const int64_t nr = reads->n_reads, ts = so[nr], tb = qo[nr], nc = fo[nr];
    if (nc == 0) return 0;
    const int L = reads->cc_before + reads->cc_after;
    Stage st{e};
    RMR_TRY(st.init(reads_stage_bytes(reads, ts, tb, nc) + Stage::pad(ts * 4) + Stage::pad(nc * 48) +
                    Stage::pad((size_t)nc * L * 4) + Stage::pad((size_t)nc * seq_w) +
                    Stage::pad((size_t)nc * map_w * 2) + Stage::pad(nc * 2) + Stage::pad(nc * 8) + 8192));
    DevReads dr;
    RMR_TRY(stage_reads(e, st, reads, mem, false, so, qo, fo, &dr));
    if (mem == RMR_MEM_DEVICE)
        return launch_fill(e, dr.d, nc, dr.chunk_read, sig, geo, signal, seqs, seq_w, maps, map_w, lens,
                           read_focus_bases);
    float *dsig = st.take<float>(ts + 1);
    int64_t *dgeo = st.take<int64_t>(nc * 6);
    float *dsignal = st.take<float>((size_t)nc * L);
    int8_t *dseqs = st.take<int8_t>((size_t)nc * seq_w);
    int16_t *dmaps = st.take<int16_t>((size_t)nc * map_w);
    int16_t *dlens = st.take<int16_t>(nc);
    int64_t *drfb = st.take<int64_t>(nc);
    H2D(dsig, sig, (size_t)ts * 4);
    H2D(dgeo, geo, (size_t)nc * 48);
    RMR_TRY(launch_fill(e, dr.d, nc, dr.chunk_read, dsig, dgeo, dsignal, dseqs, seq_w, dmaps, map_w, dlens, drfb));
    D2H(signal, dsignal, (size_t)nc * L * 4);
    D2H(seqs, dseqs, (size_t)nc * seq_w);
    D2H(maps, dmaps, (size_t)nc * map_w * 2);
    D2H(lens, dlens, (size_t)nc * 2);
    D2H(read_focus_bases, drfb, (size_t)nc * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_count_labels(rmr_engine *e, const float *logits, int64_t n, int num_out, int64_t *counts,
                     int mem) {
    if (!e || !logits || !counts) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (num_out < 1 || num_out > 16) RMR_FAIL(RMR_ERR_INVALID, "num_out %d not in [1,16]", num_out);
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE) return launch_count(e, logits, n, num_out, counts);
    Stage st{e};
    RMR_TRY(st.init(Stage::pad((size_t)n * num_out * 4) + 4096));
    float *dl = st.take<float>((size_t)n * num_out);
    int64_t *dc = st.take<int64_t>(16);
    H2D(dl, logits, (size_t)n * num_out * 4);
    H2D(dc, counts, (size_t)num_out * 8);
    RMR_TRY(launch_count(e, dl, n, num_out, dc));
    D2H(counts, dc, (size_t)num_out * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_validation_tally(rmr_engine *e, const float *logits, const int64_t *labels, int64_t n, int num_out, int num_labels,
                         const int32_t *label_of_column, int64_t *confusion, float *win_prob, uint8_t *call, double *loss_sum) {
    if (!e || !logits || !labels || !label_of_column || !confusion || !win_prob || !call || !loss_sum)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (num_out < 1 || num_out > 16 || num_labels < num_out || num_labels > 16)
        RMR_FAIL(RMR_ERR_INVALID, "num_out %d / num_labels %d not in [1,16], num_labels >= num_out", num_out, num_labels);
    for (int c = 0; c < num_labels; ++c)
        if (label_of_column[c] < -1 || label_of_column[c] >= num_out) RMR_FAIL(RMR_ERR_INVALID, "label_of_column[%d] = %d", c, label_of_column[c]);
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_validation_tally(e, logits, labels, n, num_out, num_labels, label_of_column, confusion, win_prob, call, loss_sum);
}

static int check_motifs(const rmr_motif_set *motifs) {
    if (motifs->n_motifs < 1 || motifs->n_motifs > 8) RMR_FAIL(RMR_ERR_INVALID, "1..8 motifs supported");
    for (int m = 0; m < motifs->n_motifs; ++m)
        if (motifs->len[m] < 1 || motifs->len[m] > 16 || motifs->focus_pos[m] >= motifs->len[m] || motifs->focus_pos[m] < -64)
            RMR_FAIL(RMR_ERR_INVALID, "motif %d: length %d / focus %d unsupported", m, motifs->len[m], motifs->focus_pos[m]);
    return 0;
}

int rmr_motif_focus_counts(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads, const rmr_motif_set *motifs,
                           int64_t *counts) {
    if (!e || !int_seq || !seq_off || !motifs || !counts) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads");
    RMR_TRY(check_motifs(motifs));
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_motif_focus(e, int_seq, seq_off, (int)n_reads, *motifs, counts, nullptr, nullptr);
}

int rmr_motif_focus_fill(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads, const rmr_motif_set *motifs,
                         const int64_t *foc_off, int64_t *focus) {
    if (!e || !int_seq || !seq_off || !motifs || !foc_off || !focus) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads");
    RMR_TRY(check_motifs(motifs));
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_motif_focus(e, int_seq, seq_off, (int)n_reads, *motifs, nullptr, foc_off, focus);
}

// ---- the one collective: RCCL, loaded on first use (a single-GPU process never touches it) ----------------
namespace {
struct NcclId { char internal[RMR_COMM_ID_BYTES]; };  // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(NcclId *) = nullptr;
    int (*CommInitRank)(void **, int, NcclId, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
constexpr int kNcclInt64 = 4, kNcclSum = 0;  // rccl.h ncclDataType_t / ncclRedOp_t

int rccl_api(Rccl **out) {
    static Rccl api;
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (!api.lib) {
        // the RCCL already in the process (PyTorch-ROCm ships one bound to the HIP runtime this process uses), else ROCm's
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        void *h = nullptr;
        for (const char *nm : names)
            if ((h = dlopen(nm, RTLD_NOW | RTLD_NOLOAD))) break;
        for (size_t i = 0; !h && i < sizeof(names) / sizeof(names[0]); ++i) h = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
        if (!h) RMR_FAIL(RMR_ERR_INVALID, "cannot load librccl (%s)", dlerror());
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
        api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(h, "ncclAllReduce"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
        if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy || !api.GetErrorString)
            RMR_FAIL(RMR_ERR_INVALID, "librccl lacks an expected symbol");
        api.lib = h;
    }
    *out = &api;
    return 0;
}
#define RMR_NCCL(api, expr)                                                                  \
    do {                                                                                     \
        const int _r = (expr);                                                               \
        if (_r != 0) RMR_FAIL(RMR_ERR_HIP, "RCCL error %s (%s)", (api)->GetErrorString(_r), #expr); \
    } while (0)
}  // namespace

}  // extern "C"
namespace rmr {
void rccl_comm_free(void *comm) {
    Rccl *r;
    if (comm && rccl_api(&r) == 0) (void)r->CommDestroy(comm);
}
}  // namespace rmr
extern "C" {

int rmr_comm_unique_id(uint8_t id[RMR_COMM_ID_BYTES]) {
    if (!id) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    Rccl *r;
    RMR_TRY(rccl_api(&r));
    NcclId u;
    RMR_NCCL(r, r->GetUniqueId(&u));
    memcpy(id, u.internal, RMR_COMM_ID_BYTES);
    return 0;
}

int rmr_comm_init(rmr_engine *e, const uint8_t id[RMR_COMM_ID_BYTES], int rank, int world) {
    if (!e || !id) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (world < 1 || rank < 0 || rank >= world) RMR_FAIL(RMR_ERR_INVALID, "rank %d / world %d", rank, world);
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->comm) RMR_FAIL(RMR_ERR_INVALID, "engine already has a communicator (rmr_comm_destroy first)");
    Rccl *r;
    RMR_TRY(rccl_api(&r));
    RMR_HIP(hipSetDevice(e->device));
    NcclId u;
    memcpy(u.internal, id, RMR_COMM_ID_BYTES);
    void *comm = nullptr;
    RMR_NCCL(r, r->CommInitRank(&comm, world, u, rank));
    e->comm = comm;
    e->comm_rank = rank;
    e->comm_world = world;
    return 0;
}

int rmr_comm_destroy(rmr_engine *e) {
    if (!e) RMR_FAIL(RMR_ERR_INVALID, "engine is NULL");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->comm) return 0;
    Rccl *r;
    RMR_TRY(rccl_api(&r));
    RMR_HIP(hipSetDevice(e->device));
    RMR_HIP(hipStreamSynchronize(e->stream));
    void *c = e->comm;
    e->comm = nullptr;
    e->comm_world = 1;
    e->comm_rank = 0;
    RMR_NCCL(r, r->CommDestroy(c));
    return 0;
}

int rmr_allreduce_counts(rmr_engine *e, int64_t *counts, int n, int mem) {
    if (!e || !counts) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n < 1 || n > 4096) RMR_FAIL(RMR_ERR_INVALID, "n %d not in [1,4096]", n);
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->comm || e->comm_world == 1) return 0;  // one process: the sum over ranks is the input
    Rccl *r;
    RMR_TRY(rccl_api(&r));
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE) {
        RMR_NCCL(r, r->AllReduce(counts, counts, (size_t)n, kNcclInt64, kNcclSum, e->comm, e->stream));
        return 0;
    }
    Stage st{e};
    RMR_TRY(st.init(Stage::pad((size_t)n * 8) + 1024));
    int64_t *dc = st.take<int64_t>(n);
    H2D(dc, counts, (size_t)n * 8);
    RMR_NCCL(r, r->AllReduce(dc, dc, (size_t)n, kNcclInt64, kNcclSum, e->comm, e->stream));
    D2H(counts, dc, (size_t)n * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_motif_flags(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads,
                    const rmr_motif_set *motifs, uint8_t *flags, int mem) {
    if (!e || !int_seq || !seq_off || !motifs || !flags) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads");
    if (motifs->n_motifs < 1 || motifs->n_motifs > 8) RMR_FAIL(RMR_ERR_INVALID, "1..8 motifs supported");
    for (int m = 0; m < motifs->n_motifs; ++m)
        if (motifs->len[m] < 1 || motifs->len[m] > 16 || motifs->focus_pos[m] >= motifs->len[m] ||
            motifs->focus_pos[m] < -64)
            RMR_FAIL(RMR_ERR_INVALID, "motif %d: length %d / focus %d unsupported", m, motifs->len[m], motifs->focus_pos[m]);
    if (n_reads == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    int64_t total = 0;
    if (mem == RMR_MEM_HOST) total = seq_off[n_reads];
    else RMR_HIP(hipMemcpy(&total, seq_off + n_reads, 8, hipMemcpyDeviceToHost));
    if (total <= 0) return 0;
    if (mem == RMR_MEM_DEVICE) return launch_motif(e, int_seq, seq_off, (int)n_reads, total, *motifs, flags);
    Stage st{e};
    RMR_TRY(st.init(2 * Stage::pad((size_t)total) + Stage::pad((size_t)(n_reads + 1) * 8) + 4096));
    int8_t *ds = st.take<int8_t>(total);
    int64_t *d_off = st.take<int64_t>(n_reads + 1);
    uint8_t *df = st.take<uint8_t>(total);
    H2D(ds, int_seq, (size_t)total);
    H2D(d_off, seq_off, (size_t)(n_reads + 1) * 8);
    RMR_TRY(launch_motif(e, ds, d_off, (int)n_reads, total, *motifs, df));
    D2H(flags, df, (size_t)total);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_vbz_decode(rmr_engine *e, const uint8_t *svb, const int64_t *row_off, const int32_t *row_samples,
                   int64_t n_rows, int16_t *out, int mem) {
    if (!e || !svb || !row_off || !row_samples || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_rows < 0 || n_rows > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_rows");
    if (n_rows == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::vector<int64_t> ro((size_t)n_rows + 1), oo((size_t)n_rows + 1);
    std::vector<int32_t> rn((size_t)n_rows);
    if (mem == RMR_MEM_HOST) {
        memcpy(ro.data(), row_off, ro.size() * 8);
        memcpy(rn.data(), row_samples, rn.size() * 4);
    } else {
        RMR_HIP(hipMemcpy(ro.data(), row_off, ro.size() * 8, hipMemcpyDeviceToHost));
        RMR_HIP(hipMemcpy(rn.data(), row_samples, rn.size() * 4, hipMemcpyDeviceToHost));
    }
    oo[0] = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (rn[r] < 0 || ro[r + 1] < ro[r] || ro[r + 1] - ro[r] < ((int64_t)rn[r] + 7) / 8 + rn[r])
            RMR_FAIL(RMR_ERR_INVALID, "corrupt VBZ signal block (row %lld)", (long long)r);
        oo[r + 1] = oo[r] + rn[r];
    }
    const int64_t nbytes = ro[n_rows], nout = oo[n_rows];
    Stage st{e};
    RMR_TRY(st.init(Stage::pad((size_t)nbytes + 16) + 2 * Stage::pad((size_t)(n_rows + 1) * 8) + 2 * Stage::pad((size_t)n_rows * 4) +
                    Stage::pad((size_t)nout * 2 + 16) + 8192));
    int64_t *d_oo = st.take<int64_t>(n_rows + 1);
    int32_t *d_st = st.take<int32_t>(n_rows);
    H2D(d_oo, oo.data(), oo.size() * 8);
    RMR_HIP(hipMemsetAsync(d_st, 0, (size_t)n_rows * 4, e->stream));
    const uint8_t *d_svb = svb;
    const int64_t *d_ro = row_off;
    const int32_t *d_rn = row_samples;
    int16_t *d_out = out;
    if (mem == RMR_MEM_HOST) {
        uint8_t *b = st.take<uint8_t>(nbytes + 16);
        int64_t *o = st.take<int64_t>(n_rows + 1);
        int32_t *c = st.take<int32_t>(n_rows);
        d_out = st.take<int16_t>(nout + 8);
        H2D(b, svb, (size_t)nbytes);
        H2D(o, row_off, ro.size() * 8);
        H2D(c, row_samples, rn.size() * 4);
        d_svb = b; d_ro = o; d_rn = c;
    }
    RMR_TRY(launch_vbz(e, d_svb, d_ro, d_rn, d_oo, n_rows, d_out, d_st));
    std::vector<int32_t> hst((size_t)n_rows);
    D2H(hst.data(), d_st, (size_t)n_rows * 4);
    if (mem == RMR_MEM_HOST) D2H(out, d_out, (size_t)nout * 2);
    RMR_HIP(hipStreamSynchronize(e->stream));
    for (int64_t r = 0; r < n_rows; ++r)
        if (hst[r]) RMR_FAIL(RMR_ERR_INVALID, "corrupt VBZ signal block (row %lld)", (long long)r);
    return 0;
}

int rmr_forward(rmr_model *m, const float *sigs, const float *seqs, int64_t n, float *logits, int mem) {
    if (!m || !sigs || !seqs || !logits) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n <= 0) return 0;
    rmr_engine *e = m->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE) return run_pipeline(m, sigs, seqs, nullptr, 0, nullptr, 0, nullptr, 0, 0, n, logits);
    const size_t L = m->L, EC = 4 * (size_t)m->desc.kmer_len, no = m->desc.num_out;
    Stage st{e};
    RMR_TRY(st.init(Stage::pad(n * L * 4) + Stage::pad(n * EC * L * 4) + Stage::pad(n * no * 4) + 4096));
    float *ds = st.take<float>(n * L);
    float *dq = st.take<float>(n * EC * L);
    float *dl = st.take<float>(n * no);
    H2D(ds, sigs, n * L * 4);
    H2D(dq, seqs, n * EC * L * 4);
    RMR_TRY(run_pipeline(m, ds, dq, nullptr, 0, nullptr, 0, nullptr, 0, 0, n, dl));
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
    // one blob, host (pinned) and device images with the same offsets: everything the extraction kernels read; the
    // geometry rows behind it travel in a second, small copy
    size_t off = 0;
    auto seg = [&off](size_t bytes) { const size_t o = off; off += Stage::pad(bytes); return o; };
    const size_t o_dacs = seg(ns * 2 + 16), o_map = seg((nb + 1) * 8), o_seq = seg(nb + 16), o_foc = seg(nc * 8), o_off = seg(6 * 8),
                 o_sc = seg(2 * 8), o_cr = seg((nc + 1) * 4), blob_bytes = off, o_geo = seg(nc * 48), in_bytes = off;
    const size_t out_bytes = Stage::pad((size_t)nc * no * 4) + 256;
    RMR_TRY(e->ensure_pin_call(in_bytes + out_bytes));
    char *hp = reinterpret_cast<char *>(e->pin_call);
    // The staging buffer is pinned host memory the GPU can address: for ONE read the kernels fetch the read's arrays from it
    // across PCIe themselves and write the logits back into it (150 KB in, 2.5 KB out) instead of three queued copies, each
    // of which cost a launch on the host and a blit kernel + a dependency gap on the stream - a sixth of the call
    // (profiles/NOTES_r05.md section 1d).  RMR_CALL_READ_ZERO_COPY: bit 0 the read's arrays, bit 1 the chunk geometry,
    // bit 2 the logits; 0 = the copies.
    static const int zc = 7;
    char *hp_dev = nullptr;
    if (zc) RMR_HIP(hipHostGetDevicePointer(reinterpret_cast<void **>(&hp_dev), hp, 0));
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
    // The arena is sized before the widths of the chunk rows are known, for chunks of up to `cap` bases (a chunk of L samples
    // holds more only where bases have no samples of their own: then it grows to the exact number below, before anything that
    // depends on it is queued).
    Stage st{e};
    const int64_t cap = std::min<int64_t>(nb + 1, 2 * (int64_t)L + 8);
    auto arena_bytes = [&](int64_t msl_) {
        return in_bytes + Stage::pad(ns * 4 + 16) + Stage::pad((size_t)nc * L * 4) + Stage::pad((size_t)nc * (msl_ + r->kb + r->ka + 1)) +
               Stage::pad((size_t)nc * (msl_ + 2) * 2) + Stage::pad(nc * 2) + Stage::pad(nc * 8) + Stage::pad((size_t)nc * no * 4) + 8192;
    };
    // the read's arrays first and on their way ...
    RMR_TRY(st.init(arena_bytes(cap)));
    char *dp = st.take<char>(in_bytes);
    char *arena_in = dp;
    if (zc & 1) dp = hp_dev;
    else RMR_HIP(hipMemcpyAsync(dp, hp, blob_bytes, hipMemcpyHostToDevice, e->stream));
    rmr_reads d{};
    d.n_reads = 1;
    d.dacs = reinterpret_cast<const int16_t *>(dp + o_dacs);
    d.seq_to_sig = reinterpret_cast<const int64_t *>(dp + o_map);
    d.int_seq = reinterpret_cast<const int8_t *>(dp + o_seq);
    d.focus_bases = reinterpret_cast<const int64_t *>(dp + o_foc);
    d.sig_off = reinterpret_cast<const int64_t *>(dp + o_off);
    d.seq_off = d.sig_off + 2;
    d.focus_off = d.sig_off + 4;
    d.shift = reinterpret_cast<const double *>(dp + o_sc);
    d.scale = d.shift + 1;
    d.cc_before = r->cc_before; d.cc_after = r->cc_after; d.kb = r->kb; d.ka = r->ka;
    d.base_start_justify = r->base_start_justify; d.offset = r->offset;
    const int32_t *chunk_read = reinterpret_cast<const int32_t *>(dp + o_cr);
    const int64_t *dgeo = reinterpret_cast<const int64_t *>(((zc & 2) ? hp_dev : arena_in) + o_geo);
    float *dsig = st.take<float>(ns + 4);
    RMR_TRY(launch_geometry(e, d, 0, chunk_read, dsig, ns, nullptr, nullptr, nullptr));  // n_chunks 0: the signal normalisation alone
    // ... then, while they cross PCIe and the signal is normalised, the geometry of the chunks on the host: integer
    // arithmetic on the mapping - the function the geometry kernel runs (rmr_geometry.h), its searches started at the focus
    // base when the mapping is monotone.  The widths of the chunk rows are then known without asking the GPU: the whole call
    // is queued behind one another and waited for once.
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
    if (msl > cap) {  // zero-dwell bases made a chunk wider than the arena was sized for: start over with the exact size
        RMR_HIP(hipStreamSynchronize(e->stream));
        st = Stage{e};
        RMR_TRY(st.init(arena_bytes(msl)));
        dp = st.take<char>(in_bytes);
        arena_in = dp;
        if (zc & 1) dp = hp_dev;
        else RMR_HIP(hipMemcpyAsync(dp, hp, blob_bytes, hipMemcpyHostToDevice, e->stream));
        d.dacs = reinterpret_cast<const int16_t *>(dp + o_dacs);
        d.seq_to_sig = reinterpret_cast<const int64_t *>(dp + o_map);
        d.int_seq = reinterpret_cast<const int8_t *>(dp + o_seq);
        d.focus_bases = reinterpret_cast<const int64_t *>(dp + o_foc);
        d.sig_off = reinterpret_cast<const int64_t *>(dp + o_off);
        d.seq_off = d.sig_off + 2;
        d.focus_off = d.sig_off + 4;
        d.shift = reinterpret_cast<const double *>(dp + o_sc);
        d.scale = d.shift + 1;
        chunk_read = reinterpret_cast<const int32_t *>(dp + o_cr);
        dgeo = reinterpret_cast<const int64_t *>(((zc & 2) ? hp_dev : arena_in) + o_geo);
        dsig = st.take<float>(ns + 4);
        RMR_TRY(launch_geometry(e, d, 0, chunk_read, dsig, ns, nullptr, nullptr, nullptr));
    }
    if (!(zc & 2)) RMR_HIP(hipMemcpyAsync(arena_in + o_geo, hp + o_geo, (size_t)nc * 48, hipMemcpyHostToDevice, e->stream));
    const int seq_w = (int)std::max<int64_t>(msl + r->kb + r->ka, r->kb + r->ka + 1), map_w = (int)std::max<int64_t>(msl + 1, 2);
    float *dsignal = st.take<float>((size_t)nc * L);
    int8_t *dseqs = st.take<int8_t>((size_t)nc * seq_w);
    int16_t *dmaps = st.take<int16_t>((size_t)nc * map_w);
    int16_t *dlens = st.take<int16_t>(nc);
    int64_t *drfb = st.take<int64_t>(nc);
    float *dlog = st.take<float>((size_t)nc * no);
    float *hlog = reinterpret_cast<float *>(hp + in_bytes);
    if (zc & 4) dlog = reinterpret_cast<float *>(hp_dev + in_bytes);
    RMR_TRY(launch_fill(e, d, nc, chunk_read, dsig, dgeo, dsignal, dseqs, seq_w, dmaps, map_w, dlens, drfb));
    RMR_TRY(run_pipeline(m, dsignal, nullptr, dseqs, seq_w, dmaps, map_w, dlens, r->kb, r->ka, nc, dlog));
    if (!(zc & 4)) RMR_HIP(hipMemcpyAsync(hlog, dlog, (size_t)nc * no * 4, hipMemcpyDeviceToHost, e->stream));
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
        RMR_TRY(run_pipeline(m, signal, nullptr, seqs, seq_w, maps, map_w, lens, kb, ka, n, logits));
        if (label_counts) RMR_TRY(launch_count(e, logits, n, no, label_counts));
        return 0;
    }
    const size_t L = m->L;
    Stage st{e};
    RMR_TRY(st.init(Stage::pad(n * L * 4) + Stage::pad((size_t)n * seq_w) + Stage::pad((size_t)n * map_w * 2) +
                    Stage::pad(n * 2) + Stage::pad((size_t)n * no * 4) + 8192));
    float *dsig = st.take<float>(n * L);
    int8_t *ds = st.take<int8_t>((size_t)n * seq_w);
    int16_t *dm = st.take<int16_t>((size_t)n * map_w);
    int16_t *dl = st.take<int16_t>(n);
    float *dlog = st.take<float>((size_t)n * no);
    int64_t *dc = st.take<int64_t>(16);
    const int64_t hsb = tune_int("RMR_HOST_SUBBATCH", 131072);
    if (hsb > 0 && n > hsb) {
        // pipelined upload: the CPU copies sub-batch i+1 into a pinned slot and the aux stream uploads it
        // while the kernels of sub-batch i run on the main stream
        const size_t o_seq = Stage::pad((size_t)hsb * L * 4), o_map = o_seq + Stage::pad((size_t)hsb * seq_w);
        const size_t o_len = o_map + Stage::pad((size_t)hsb * map_w * 2), slot_b = o_len + Stage::pad((size_t)hsb * 2);
        RMR_TRY(e->ensure_pinned(2 * slot_b));
        const int nthr = (int)4;
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
            RMR_TRY(run_pipeline(m, dsig + (size_t)c0 * L, nullptr, ds + (size_t)c0 * seq_w, seq_w, dm + (size_t)c0 * map_w,
                                 map_w, dl + c0, kb, ka, nb, dlog + (size_t)c0 * no));
        }
    } else {
        H2D(dsig, signal, n * L * 4);
        H2D(ds, seqs, (size_t)n * seq_w);
        H2D(dm, maps, (size_t)n * map_w * 2);
        H2D(dl, lens, (size_t)n * 2);
        RMR_TRY(run_pipeline(m, dsig, nullptr, ds, seq_w, dm, map_w, dl, kb, ka, n, dlog));
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
