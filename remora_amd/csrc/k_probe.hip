// k_probe.hip — the two reductions of the Winograd guard (rmr_model_create / rmr_model_check_winograd, api_forward.hip) over
// the logits of the probe batch in the Winograd form (a) and the direct form (b): max |a - b| and the count of non-finite
// entries in either.  A few thousand floats: a grid-stride pass, lanes -> wave by shuffles, waves -> block through LDS, one
// atomic per block on a word the caller zeroed.  The maximum is taken on the bit pattern of the non-negative float (the
// order of non-negative IEEE floats is the order of their bits as unsigned integers).
#include "rmr_internal.h"

namespace rmr {

namespace {

constexpr int PROBE_THREADS = 256;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// entries that are not finite in both arrays belong to the other kernel's count, not to the maximum
__global__ __launch_bounds__(PROBE_THREADS) void probe_max_diff_kernel(const float *a, const float *b, int64_t n, unsigned *out_bits) {
    __shared__ float part[PROBE_THREADS / 64];
    float mx = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PROBE_THREADS) {
        const float x = a[i], y = b[i];
        if (finite_f(x) && finite_f(y)) {
            const float d = fabsf(x - y);
            if (finite_f(d)) mx = fmaxf(mx, d);
        }
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_down(mx, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PROBE_THREADS / 64; ++w) mx = fmaxf(mx, part[w]);
        atomicMax(out_bits, __float_as_uint(mx));
    }
}

__global__ __launch_bounds__(PROBE_THREADS) void probe_nonfinite_kernel(const float *a, const float *b, int64_t n, unsigned *out_count) {
    __shared__ unsigned part[PROBE_THREADS / 64];
    unsigned cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * PROBE_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PROBE_THREADS)
        cnt += (finite_f(a[i]) ? 0u : 1u) + (finite_f(b[i]) ? 0u : 1u);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PROBE_THREADS / 64; ++w) cnt += part[w];
        if (cnt) atomicAdd(out_count, cnt);
    }
}

}  // namespace

// out[0]: bits of max |a - b|, out[1]: non-finite entries of a and b; both zeroed here, on the engine's stream
int launch_probe_compare(rmr_engine *e, const float *a, const float *b, int64_t n, unsigned *out) {
    if (n <= 0) RMR_FAIL(RMR_ERR_INVALID, "empty probe");
    RMR_HIP(hipMemsetAsync(out, 0, 2 * sizeof(unsigned), e->stream));
    int64_t grid = (n + PROBE_THREADS - 1) / PROBE_THREADS;
    if (grid > (int64_t)e->num_cus) grid = (int64_t)e->num_cus;
    {
        ProfScope ps(e, K_PROBE_DIFF);
        hipLaunchKernelGGL(probe_max_diff_kernel, dim3((unsigned)grid), dim3(PROBE_THREADS), 0, e->stream, a, b, n, out);
        RMR_HIP(hipGetLastError());
    }
    ProfScope ps(e, K_PROBE_NONFINITE);
    hipLaunchKernelGGL(probe_nonfinite_kernel, dim3((unsigned)grid), dim3(PROBE_THREADS), 0, e->stream, a, b, n, out + 1);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
