// engine.hip — the engine of libremora_hip.so: error text, kernel names, engine lifetime and synchronisation, the scratch
// arenas and pinned buffers, per-device kernel attributes, the per-kernel HIP-event profiler and the poison kernel.  The entry
// points that compute live in api_forward.hip, api_data.hip and comm.cpp.  See include/remora_hip.h for the contract of every
// entry point and the reference interface (file:line) each one replaces.
#include <memory>

#include "rmr_internal.h"

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
    "fused_front", "rescale_quantiles", "sig3_front", "seq2_front", "probe_max_diff", "probe_nonfinite", "winograd_form",
    "base_metrics", "region_metrics", "region_signals", "site_kmer_levels", "modbam_sites", "rescale_points", "theil_sen_fit",
    "duplex_dp", "duplex_traceback", "duplex_lines", "duplex_backtrack", "train_gemm", "train_wgrad", "train_reduce", "train_bn", "train_lstm",
    "train_loss", "train_adamw", "train_aux", "read_index_build", "read_index_lookup", "pileup_emit", "pileup_flush", "ref_genome_pack", "pileup_stamp",
    "pileup_pair", "pileup_cover"};
const char *kernel_name(int id) { return (id >= 0 && id < K_NUM) ? k_names[id] : "?"; }

}  // namespace rmr

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
const char *rmr_version(void) { return "remora_hip 0.12 (gfx950)"; }  // 0.12: rmr_read_index_*

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
