// k_train.hip - the kernels of the fp32 ConvLSTM_w_ref training step (api_train.hip drives them).
//
// Everything GEMM-shaped - the forward pass, the data gradient and the weight gradient of the convolutions, the LSTM and
// fc products - runs on v_mfma_f32_16x16x4_f32: two kernels for the products over all rows, and one per direction for an
// LSTM step (recurrent product + cell, train_lstm_step_kernel / train_lstm_step_bwd_kernel).  Activations are
// channel-last, so the im2col row of a convolution output (n, l) is one contiguous SPAN of its input, K = taps x channels
// floats from row l * stride of chunk n:
//   train_gemm_kernel   C[r][c] = sum_k A[span(r) + k] B[k][c]; span elements outside the chunk's buffer read as zero,
//                       which makes the data gradient the same product on the output gradient (full correlation, one
//                       polyphase column block per stride phase)
//   train_wgrad_kernel  P[slice][k][c] = sum_{r in slice} A[span(r) + k] dY[span'(r) + c]; train_wgrad_reduce_kernel adds
//                       the slices in fixed order (double) and writes the gradient in the parameter's own layout
// Every sum over rows (weight gradients, BatchNorm statistics, bias gradients, loss) is per-block partials plus a
// second pass in fixed order: no float atomics, the same bits on every run.
#include <climits>

#include "rmr_mma.h"

namespace rmr {

// ---- the two matrix-core kernels ---------------------------------------------------------------------------------------
// 64 rows x 64 columns per block of four waves: a wave owns 16 rows and four 16-column accumulators.  A lane loads four
// consecutive k of its row at once and spends them on four MFMAs (k = k0 + 4 (lane >> 4) + j in MFMA j; B follows the
// same order).  K is a multiple of 4 and every span starts on a multiple of 4 floats (checked by the launcher).
__global__ __launch_bounds__(256) void train_gemm_kernel(const float *__restrict__ A, const TrainSpan sa, const float *__restrict__ B,
                                                         const int ldb, const int K, float *__restrict__ C, const TrainSpan sc,
                                                         const int NC, const long long R, const float *__restrict__ bias) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const long long r = (long long)blockIdx.x * 64 + wave * 16 + lr;
    const int c0 = blockIdx.y * 64;
    long long start = 0, lo = 0, hi = 0;
    const bool rv = r < R;
    if (rv) {
        const long long n = r / sa.rpc;
        const int i = (int)(r - n * sa.rpc);
        lo = n * sa.cs;
        hi = lo + sa.valid;
        start = lo + (long long)i * sa.rs + sa.off;
    }
    f32x4 acc[4] = {};
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int ka = k0 + 4 * lq;
        const long long idx = start + ka;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rv && ka < K && idx >= lo && idx + 3 < hi) a = *reinterpret_cast<const float4 *>(A + idx);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = ka + j;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = c0 + 16 * t + lr;
                const float b = (kk < K && col < NC) ? B[(size_t)kk * ldb + col] : 0.f;
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b, acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const long long ro = (long long)blockIdx.x * 64 + wave * 16 + lq * 4 + reg;
        if (ro >= R) continue;
        const long long n = ro / sc.rpc;
        const int i = (int)(ro - n * sc.rpc);
        const long long within = (long long)i * sc.rs + sc.off;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = c0 + 16 * t + lr;
            if (col >= NC || within + col < 0 || within + col >= sc.valid) continue;
            float v = acc[t][reg];
            if (bias) v += bias[col];
            C[n * sc.cs + within + col] = v;
        }
    }
}

// grid (ceil(K / 64), ceil(NC / 64), slices): rows [slice * rows_per, ...) of R; P[slice][k][c]
__global__ __launch_bounds__(256) void train_wgrad_kernel(const float *__restrict__ A, const TrainSpan sa, const float *__restrict__ D,
                                                          const TrainSpan sd, const int K, const int NC, const long long R,
                                                          const long long rows_per, float *__restrict__ P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int k = blockIdx.x * 64 + wave * 16 + lr;  // the A operand's row of the product: the weight's input index
    const int c0 = blockIdx.y * 64;
    const long long r0 = (long long)blockIdx.z * rows_per;
    const long long r1 = r0 + rows_per < R ? r0 + rows_per : R;
    f32x4 acc[4] = {};
    for (long long rb = r0; rb < r1; rb += 4) {
        const long long r = rb + lq;
        float a = 0.f, b[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < r1) {
            const long long na = r / sa.rpc, nd = r / sd.rpc;
            const long long ia = r - na * sa.rpc, id = r - nd * sd.rpc;
            if (k < K) a = A[na * sa.cs + ia * sa.rs + sa.off + k];
            const float *drow = D + nd * sd.cs + id * sd.rs + sd.off;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = c0 + 16 * t + lr;
                if (col < NC) b[t] = drow[col];
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int ko = blockIdx.x * 64 + wave * 16 + lq * 4 + reg;
        if (ko >= K) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = c0 + 16 * t + lr;
            if (col < NC) P[((size_t)blockIdx.z * K + ko) * NC + col] = acc[t][reg];
        }
    }
}

// grad[c][ic][kw] = sum over slices of P[slice][kw * IC + ic][c] (a linear layer: KW = 1); slices == 0 writes zeros.  One
// block of 64 lanes per element: lane i adds slices i, i + 64, ... in order, lane 0 then adds the 64 lane sums in order.
// refused[0] >= 0 (train_mask_count_kernel found a label out of range): the gradient is left as it was
__global__ __launch_bounds__(64) void train_wgrad_reduce_kernel(const float *__restrict__ P, const int slices, const int K, const int NC, const int IC,
                                                                const int KW, const int *__restrict__ refused, float *__restrict__ grad) {
    __shared__ double red[64];
    const int e = blockIdx.x;
    const int k = e / NC, c = e - k * NC;
    double s = 0.0;
    for (int z = threadIdx.x; z < slices; z += 64) s += (double)P[((size_t)z * K + k) * NC + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x || refused[0] >= 0) return;
    s = 0.0;
    for (int i = 0; i < 64; ++i) s += red[i];
    const int kw = k / IC, ic = k - kw * IC;
    grad[((size_t)c * IC + ic) * KW + kw] = (float)s;
}

// ---- weights in the order the products read them -----------------------------------------------------------------------
// mode 0: out[(kw * IC + ic) * OC + oc] = W[oc][ic][kw]  (forward; a linear layer's transpose with KW = 1)
// mode 1: out[((j' * OC) + oc) * (P * IC) + p * IC + ic] = W[oc][ic][p + P (J - 1 - j')], zero beyond the last tap (data gradient)
__global__ void train_repack_kernel(const float *__restrict__ W, const int OC, const int IC, const int KW, const int P, const int J,
                                    const int mode, float *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (mode == 0) {
        if (e >= OC * IC * KW) return;
        const int oc = e % OC, k = e / OC;
        const int kw = k / IC, ic = k - kw * IC;
        out[e] = W[((size_t)oc * IC + ic) * KW + kw];
    } else {
        if (e >= J * OC * P * IC) return;
        const int col = e % (P * IC), row = e / (P * IC);
        const int p = col / IC, ic = col - p * IC;
        const int jp = row / OC, oc = row - jp * OC;
        const int kw = p + P * (J - 1 - jp);
        out[e] = kw < KW ? W[((size_t)oc * IC + ic) * KW + kw] : 0.f;
    }
}

// ---- column sums over rows: partials per block, second pass in fixed order ---------------------------------------------
// 16 columns x 16 row lanes per block; block b sums rows [b * rows_per, ...).  What is summed (Q quantities per column):
//   COL_SUM   x                                   (BatchNorm mean; bias gradients)
//   COL_VAR   (x - mean)^2                        (biased variance about the mean: never E[x^2] - E[x]^2)
//   COL_BNBWD dU and dU * xhat, dU = dA swish'(u) (BatchNorm backward; u = gamma xhat + beta)
enum { COL_SUM = 0, COL_VAR = 1, COL_BNBWD = 2 };

__device__ __forceinline__ float sigmoidf_(const float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float swish_grad(const float u) {
    const float s = sigmoidf_(u);
    return s * (1.0f + u * (1.0f - s));
}

template <int MODE>
__global__ __launch_bounds__(256) void train_colsum_kernel(const float *__restrict__ X, const int C, const long long R, const long long rows_per,
                                                           const float *__restrict__ stat, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ dA, const int aw,
                                                           const int coff, float *__restrict__ part) {
    constexpr int Q = MODE == COL_BNBWD ? 2 : 1;
    __shared__ float red[Q][16][17];
    const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int c = blockIdx.y * 16 + cl;
    const long long r0 = (long long)blockIdx.x * rows_per;
    const long long r1 = r0 + rows_per < R ? r0 + rows_per : R;
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
        const float mean = MODE != COL_SUM ? stat[c] : 0.f;
        const float rstd = MODE == COL_BNBWD ? stat[C + c] : 0.f;
        const float g = MODE == COL_BNBWD ? gamma[c] : 0.f, bt = MODE == COL_BNBWD ? beta[c] : 0.f;
        for (long long r = r0 + rl; r < r1; r += 16) {
            const float x = X[r * C + c];
            if (MODE == COL_SUM) {
                s0 += x;
            } else if (MODE == COL_VAR) {
                const float d = x - mean;
                s0 = fmaf(d, d, s0);
            } else {
                const float xh = (x - mean) * rstd;
                const float du = dA[r * aw + coff + c] * swish_grad(fmaf(g, xh, bt));
                s0 += du;
                s1 = fmaf(du, xh, s1);
            }
        }
    }
    red[0][rl][cl] = s0;
    if (Q == 2) red[Q - 1][rl][cl] = s1;
    __syncthreads();
    if (rl < Q && c < C) {
        float s = 0.f;
        for (int i = 0; i < 16; ++i) s += red[rl][i][cl];
        part[((size_t)blockIdx.x * Q + rl) * C + c] = s;
    }
}

// second pass, one block of 64 lanes per column: lane i adds the partials of blocks i, i + 64, ... in order, lane 0 then adds
// the 64 lane sums in order.  what: 0 out[c] = sum (plain column sum, e.g. a bias gradient; out2 gets the same value when
// given: lstm bias_hh), 1 stat[c] = mean, 2 stat[C + c] = rstd and the running statistics move (momentum 0.1, unbiased
// variance), 3 out[c] = dgamma, out2[c] = dbeta and stat[2C + c], stat[3C + c] keep them over R for the apply pass.
// refused[0] >= 0 (a label out of range): `stat` is still written, the gradients and the running statistics stay as they were
__global__ __launch_bounds__(64) void train_colsum_final_kernel(const float *__restrict__ part, const int nblk, const int C, const int what,
                                                                const long long R, const int *__restrict__ refused, float *__restrict__ stat,
                                                                float *__restrict__ out, float *__restrict__ out2, float *__restrict__ run_mean,
                                                                float *__restrict__ run_var) {
    __shared__ double red[2][64];
    const int c = blockIdx.x;
    const int Q = what == 3 ? 2 : 1;
    double s0 = 0.0, s1 = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) {
        s0 += (double)part[((size_t)b * Q) * C + c];
        if (Q == 2) s1 += (double)part[((size_t)b * Q + 1) * C + c];
    }
    red[0][threadIdx.x] = s0, red[1][threadIdx.x] = s1;
    __syncthreads();
    if (threadIdx.x) return;
    s0 = s1 = 0.0;
    for (int i = 0; i < 64; ++i) s0 += red[0][i], s1 += red[1][i];
    const bool keep = refused[0] >= 0;
    if (what == 0) {
        if (keep) return;
        out[c] = (float)s0;
        if (out2) out2[c] = (float)s0;
    } else if (what == 1) {
        stat[c] = (float)(s0 / (double)R);
    } else if (what == 2) {
        const double var = s0 / (double)R;
        stat[C + c] = (float)(1.0 / sqrt(var + 1e-5));
        if (keep) return;
        run_mean[c] = 0.9f * run_mean[c] + 0.1f * stat[c];
        run_var[c] = 0.9f * run_var[c] + 0.1f * (float)(var * (double)R / (double)(R - 1));
    } else {
        stat[2 * C + c] = (float)(s0 / (double)R);
        stat[3 * C + c] = (float)(s1 / (double)R);
        if (keep) return;
        out[c] = (float)s1;   // bn.weight gradient
        out2[c] = (float)s0;  // bn.bias gradient
    }
}

// ---- elementwise ---------------------------------------------------------------------------------------------------------
// out[r][coff + c] = swish(gamma xhat + beta), rows of width aw
__global__ void train_bn_swish_kernel(const float *__restrict__ Y, const int C, const long long total, const float *__restrict__ stat,
                                      const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ out, const int aw,
                                      const int coff) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long long r = e / C;
    const int c = (int)(e - r * C);
    const float u = fmaf(gamma[c], (Y[e] - stat[c]) * stat[C + c], beta[c]);
    out[r * aw + coff + c] = u * sigmoidf_(u);
}

// dY = gamma rstd (dU - mean(dU) - xhat mean(dU xhat))
__global__ void train_bn_bwd_kernel(const float *__restrict__ Y, const int C, const long long total, const float *__restrict__ stat,
                                    const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ dA, const int aw,
                                    const int coff, float *__restrict__ dY) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long long r = e / C;
    const int c = (int)(e - r * C);
    const float rstd = stat[C + c];
    const float xh = (Y[e] - stat[c]) * rstd;
    const float du = dA[r * aw + coff + c] * swish_grad(fmaf(gamma[c], xh, beta[c]));
    dY[e] = gamma[c] * rstd * (du - stat[2 * C + c] - xh * stat[3 * C + c]);
}

// sig_conv1 (1 -> OC channels, K = KW is no multiple of 4): y[n][l][oc] = b[oc] + sum_k w[oc][k] sig[n][l + k]
__global__ void train_sig1_kernel(const float *__restrict__ sig, const int L, const int Lout, const int OC, const int KW,
                                  const float *__restrict__ w, const float *__restrict__ b, const long long total, float *__restrict__ y) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int oc = (int)(e % OC);
    const long long row = e / OC;
    const long long n = row / Lout;
    const int l = (int)(row - n * Lout);
    float s = b[oc];
    for (int k = 0; k < KW; ++k) s = fmaf(w[oc * KW + k], sig[n * L + l + k], s);
    y[e] = s;
}

// [n][EC][L] -> [n][L][EC]
__global__ void train_seq_transpose_kernel(const float *__restrict__ in, const int EC, const int L, const long long total, float *__restrict__ out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % EC);
    const long long row = e / EC;
    const long long n = row / L;
    const int l = (int)(row - n * L);
    out[e] = in[(n * EC + c) * L + l];
}

__global__ void train_fill_kernel(float *__restrict__ p, const long long n, const float v, const int *__restrict__ refused) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n && refused[0] < 0) p[e] = v;
}

// ---- LSTM ------------------------------------------------------------------------------------------------------------------
// One step of lstm1.  G[n][t][4S] holds the input half of the gates (x W_ih^T + b_ih + b_hh, one product for all steps); the
// kernel adds h_{t-1} W_hh^T on the matrix cores and applies the cell: G receives the activations (i, f, g, o), Cs / H / Z
// the cell state, h and swish(h).  Only this product is sequential, and it is independent per chunk.  grid (ceil(n / 64),
// S / 16): a wave owns 16 chunks x 16 units and with them the four gate tiles of those units, so the cell runs on the
// accumulators.  WhhT = weight_hh^T, [S][4S].
__global__ __launch_bounds__(256) void train_lstm_step_kernel(float *__restrict__ G, float *__restrict__ Cs, float *__restrict__ H,
                                                              float *__restrict__ Z, const float *__restrict__ WhhT, const int S, const int T,
                                                              const int t, const long long n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const long long r = (long long)blockIdx.x * 64 + wave * 16 + lr;
    const int u = blockIdx.y * 16 + lr;  // < S: S is a multiple of 16
    f32x4 acc[4] = {};
    if (t > 0) {
        const float *hrow = H + (r * T + t - 1) * S;
        for (int k0 = 0; k0 < S; k0 += 16) {
            const int ka = k0 + 4 * lq;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < n) a = *reinterpret_cast<const float4 *>(hrow + ka);
            const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float *w = WhhT + (size_t)(ka + j) * 4 * S + u;
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], w[g * S], acc[g], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const long long ro = (long long)blockIdx.x * 64 + wave * 16 + lq * 4 + reg;
        if (ro >= n) continue;
        float *g = G + (ro * T + t) * 4 * S;
        const float ig = sigmoidf_(g[u] + acc[0][reg]), fg = sigmoidf_(g[S + u] + acc[1][reg]);
        const float gg = tanhf(g[2 * S + u] + acc[2][reg]), og = sigmoidf_(g[3 * S + u] + acc[3][reg]);
        const float cp = t ? Cs[(ro * T + t - 1) * S + u] : 0.f;
        const float c = fmaf(fg, cp, ig * gg);
        const float h = og * tanhf(c);
        g[u] = ig, g[S + u] = fg, g[2 * S + u] = gg, g[3 * S + u] = og;
        Cs[(ro * T + t) * S + u] = c;
        H[(ro * T + t) * S + u] = h;
        Z[(ro * T + t) * S + u] = h * sigmoidf_(h);
    }
}

// The same step backwards.  The gradient into h_t is dgates_{t+1} W_hh (G holds the gate gradients of step t + 1; K = 4S) or,
// at t = T - 1, the gradient that enters from lstm2: dz1[n][u] swish'(h).  dc[n][u] carries the gradient into the cell state
// from step t + 1 and leaves as the one into c_{t-1}.  G's activations of step t are replaced by the gradients of its
// pre-activations.  Same grid; Whh = weight_hh, [4S][S].
__global__ __launch_bounds__(256) void train_lstm_step_bwd_kernel(float *__restrict__ G, const float *__restrict__ Cs, const float *__restrict__ H,
                                                                  const float *__restrict__ Whh, const float *__restrict__ dz1,
                                                                  float *__restrict__ dc, const int S, const int T, const int t,
                                                                  const long long n) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const long long r = (long long)blockIdx.x * 64 + wave * 16 + lr;
    const int u = blockIdx.y * 16 + lr;
    f32x4 acc[2] = {};  // two chains: the dependent latency of one exceeds its issue interval
    if (t < T - 1) {
        const float *grow = G + (r * T + t + 1) * 4 * S;
        for (int k0 = 0; k0 < 4 * S; k0 += 16) {
            const int ka = k0 + 4 * lq;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < n) a = *reinterpret_cast<const float4 *>(grow + ka);
            const float *w = Whh + (size_t)ka * S + u;
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[0], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[S], acc[1], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[2 * S], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[3 * S], acc[1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const long long ro = (long long)blockIdx.x * 64 + wave * 16 + lq * 4 + reg;
        if (ro >= n) continue;
        const long long e = ro * S + u;
        float *g = G + (ro * T + t) * 4 * S;
        const float ig = g[u], fg = g[S + u], gg = g[2 * S + u], og = g[3 * S + u];
        const float cp = t ? Cs[(ro * T + t - 1) * S + u] : 0.f;
        const float tc = tanhf(Cs[(ro * T + t) * S + u]);
        const float d_h = t < T - 1 ? acc[0][reg] + acc[1][reg] : dz1[e] * swish_grad(H[(ro * T + t) * S + u]);
        const float d_c = fmaf(d_h * og, 1.0f - tc * tc, t < T - 1 ? dc[e] : 0.f);
        g[u] = d_c * gg * ig * (1.0f - ig);
        g[S + u] = d_c * cp * fg * (1.0f - fg);
        g[2 * S + u] = d_c * ig * (1.0f - gg * gg);
        g[3 * S + u] = d_h * tc * og * (1.0f - og);
        dc[e] = d_c * fg;
    }
}

// lstm2: one step from a zero state.  G2[n][4S] pre-activations -> activations; z2 = swish(h2); H2 keeps h2, C2 keeps c
__global__ void train_lstm2_kernel(float *__restrict__ G2, float *__restrict__ C2, float *__restrict__ H2, float *__restrict__ Z2, const int S,
                                   const long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long long n = e / S;
    const int s = (int)(e - n * S);
    float *g = G2 + n * 4 * S;
    const float ig = sigmoidf_(g[s]), gg = tanhf(g[2 * S + s]), og = sigmoidf_(g[3 * S + s]);
    const float c = ig * gg;
    const float h = og * tanhf(c);
    g[s] = ig, g[S + s] = 0.f, g[2 * S + s] = gg, g[3 * S + s] = og;
    C2[e] = c, H2[e] = h, Z2[e] = h * sigmoidf_(h);
}

// dz2[n][s] = sum_o dlogits[n][o] fc.weight[o][s], then back through swish and the lstm2 step: G2 receives the gradients
// of its pre-activations (the forget gate's is exactly zero: c_0 = 0)
__global__ void train_lstm2_bwd_kernel(float *__restrict__ G2, const float *__restrict__ C2, const float *__restrict__ H2,
                                       const float *__restrict__ dlog, const float *__restrict__ fcw, const int num_out, const int S,
                                       const long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long long n = e / S;
    const int s = (int)(e - n * S);
    float dz = 0.f;
    for (int o = 0; o < num_out; ++o) dz = fmaf(dlog[n * num_out + o], fcw[o * S + s], dz);
    const float d_h = dz * swish_grad(H2[e]);
    float *g = G2 + n * 4 * S;
    const float ig = g[s], gg = g[2 * S + s], og = g[3 * S + s];
    const float tc = tanhf(C2[e]);
    const float d_c = d_h * og * (1.0f - tc * tc);
    g[s] = d_c * gg * ig * (1.0f - ig);
    g[S + s] = 0.f;
    g[2 * S + s] = d_c * ig * (1.0f - gg * gg);
    g[3 * S + s] = d_h * tc * og * (1.0f - og);
}

// ---- fc, loss ---------------------------------------------------------------------------------------------------------------
// one thread per chunk: logits, the chunk's cross-entropy term and dlogits = (softmax - onehot) mask / count
__global__ void train_fc_loss_kernel(const float *__restrict__ Z2, const float *__restrict__ fcw, const float *__restrict__ fcb, const int S,
                                     const int num_out, const int64_t *__restrict__ labels, const uint8_t *__restrict__ mask,
                                     const int *__restrict__ count, const long long n_chunks, float *__restrict__ logits,
                                     float *__restrict__ dlog, float *__restrict__ loss_part, float *__restrict__ logits_out) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_chunks) return;
    float lg[16];
    float mx = -INFINITY;
    for (int o = 0; o < num_out; ++o) {
        float s = fcb[o];
        for (int k = 0; k < S; ++k) s = fmaf(Z2[n * S + k], fcw[o * S + k], s);
        lg[o] = s;
        logits[n * num_out + o] = s;
        if (logits_out) logits_out[n * num_out + o] = s;
        mx = fmaxf(mx, s);
    }
    float se = 0.f;
    for (int o = 0; o < num_out; ++o) se += expf(lg[o] - mx);
    const float lse = mx + logf(se);
    const int64_t lab = labels[n];
    const bool on = !mask || mask[n];
    const float w = on ? 1.0f / (float)count[0] : 0.f;
    float l = 0.f;
    for (int o = 0; o < num_out; ++o) {
        const float p = expf(lg[o] - lse);
        dlog[n * num_out + o] = (p - (o == lab ? 1.0f : 0.f)) * w;
        if (o == lab) l = lse - lg[o];
    }
    loss_part[n] = on ? l : 0.f;
}

// one block, the first launch of a step: count[0] = the rows the mask keeps (no mask: n); count[1] = the first such row whose
// label is outside 0 .. num_out - 1, or -1.  What writes a gradient or a running statistic later in the step reads count[1]
// (`refused`) and holds its store when a row was found, so that the host, which sees the record with the loss, can refuse the
// call with nothing moved
__global__ __launch_bounds__(256) void train_mask_count_kernel(const uint8_t *__restrict__ mask, const int64_t *__restrict__ labels,
                                                               const int num_out, const long long n, int *__restrict__ count) {
    __shared__ int red[256], first[256];
    int s = 0, bad = INT_MAX;
    for (long long i = threadIdx.x; i < n; i += 256) {
        if (mask && !mask[i]) continue;
        s += 1;
        const int64_t lab = labels[i];
        if ((lab < 0 || lab >= num_out) && bad == INT_MAX) bad = (int)i;
    }
    red[threadIdx.x] = s, first[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[threadIdx.x] += red[threadIdx.x + w];
            first[threadIdx.x] = min(first[threadIdx.x], first[threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) count[0] = red[0], count[1] = first[0] == INT_MAX ? -1 : first[0];
}

// one block, fixed order: loss[0] = sum of the chunks' terms / count; loss[1] = count[1] (the refused row or -1) as bits, so that one
// copy brings both to the host
__global__ __launch_bounds__(256) void train_loss_reduce_kernel(const float *__restrict__ loss_part, const long long n, const int *__restrict__ count,
                                                                float *__restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) s += (double)loss_part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)count[0]), loss[1] = __int_as_float(count[1]);
}

// ---- optimiser --------------------------------------------------------------------------------------------------------------
// torch.optim.AdamW over the flat buffer; tensor_of[e] = index of e's parameter tensor, 255 for a running statistic
__global__ void train_adamw_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                                   const uint8_t *__restrict__ tensor_of, const long long n, const float lr_wd, const float omb1, const float b2,
                                   const float omb2, const float eps, const float step_size, const float bc2_sqrt,
                                   const float *__restrict__ clip) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int t = tensor_of[e];
    if (t == 255) return;
    float gr = g[e];
    if (clip) {
        const float thr = clip[t];
        if (thr >= 0.f) gr = fminf(fmaxf(gr, -thr), thr);
        g[e] = gr;
    }
    float w = p[e];
    w -= lr_wd * w;
    const float mm = m[e] + (gr - m[e]) * omb1;  // exp_avg.lerp_(grad, 1 - beta1)
    const float vv = b2 * v[e] + omb2 * gr * gr;
    m[e] = mm, v[e] = vv;
    const float denom = sqrtf(vv) / bc2_sqrt + eps;
    p[e] = w - step_size * (mm / denom);
}

// max |grad| of one parameter tensor per block
__global__ __launch_bounds__(256) void train_absmax_kernel(const float *__restrict__ g, const long long *__restrict__ off, const long long *__restrict__ size,
                                                           float *__restrict__ out) {
    __shared__ float red[256];
    const float *x = g + off[blockIdx.x];
    const long long n = size[blockIdx.x];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) s = fmaxf(s, fabsf(x[i]));
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static inline unsigned blocks_for(long long total, int per = 256) { return (unsigned)((total + per - 1) / per); }

int train_gemm(rmr_engine *e, const float *A, const TrainSpan &sa, const float *B, int ldb, int K, float *C, const TrainSpan &sc, int NC,
               long long R, const float *bias) {
    if (R <= 0) return 0;
    if (K % 4 || sa.cs % 4 || sa.rs % 4 || sa.off % 4 || sa.valid % 4) RMR_FAIL(RMR_ERR_INVALID, "train_gemm: span not a multiple of 4 floats");
    ProfScope ps(e, K_TRAIN_GEMM);
    hipLaunchKernelGGL(train_gemm_kernel, dim3(blocks_for(R, 64), blocks_for(NC, 64)), dim3(256), 0, e->stream, A, sa, B, ldb, K, C, sc, NC, R, bias);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_wgrad(rmr_engine *e, const float *A, const TrainSpan &sa, const float *D, const TrainSpan &sd, int K, int NC, long long R, int IC,
                int KW, float *part, size_t part_floats, const int *refused, float *grad) {
    int slices = 0;
    long long rows_per = 0;
    if (R > 0) {
        const size_t per = (size_t)K * NC;
        long long want = (R + 255) / 256;
        const long long cap = (long long)(part_floats / per);
        if (cap < 1) RMR_FAIL(RMR_ERR_INVALID, "train_wgrad: partials workspace too small");
        if (want > cap) want = cap;
        rows_per = (R + want - 1) / want;
        rows_per = (rows_per + 3) / 4 * 4;
        slices = (int)((R + rows_per - 1) / rows_per);
        ProfScope ps(e, K_TRAIN_WGRAD);
        hipLaunchKernelGGL(train_wgrad_kernel, dim3(blocks_for(K, 64), blocks_for(NC, 64), slices), dim3(256), 0, e->stream, A, sa, D, sd, K, NC, R,
                           rows_per, part);
        RMR_HIP(hipGetLastError());
    }
    ProfScope ps(e, K_TRAIN_REDUCE);
    hipLaunchKernelGGL(train_wgrad_reduce_kernel, dim3((unsigned)(K * NC)), dim3(64), 0, e->stream, part, slices, K, NC, IC, KW, refused, grad);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_repack(rmr_engine *e, const float *W, int OC, int IC, int KW, int P, int J, int mode, float *out) {
    const long long total = mode == 0 ? (long long)OC * IC * KW : (long long)J * OC * P * IC;
    ProfScope ps(e, K_TRAIN_AUX);
    hipLaunchKernelGGL(train_repack_kernel, dim3(blocks_for(total)), dim3(256), 0, e->stream, W, OC, IC, KW, P, J, mode, out);
    RMR_HIP(hipGetLastError());
    return 0;
}

// the number of row blocks of a column sum over R rows (the partials need blocks * Q * C floats)
int train_colsum_blocks(long long R) {
    long long b = (R + 511) / 512;
    return (int)(b < 1 ? 1 : b > 1024 ? 1024 : b);
}

int train_colsum(rmr_engine *e, int mode, const float *X, int C, long long R, float *stat, const float *gamma, const float *beta, const float *dA,
                 int aw, int coff, float *part, int what, const int *refused, float *out, float *out2, float *run_mean, float *run_var) {
    const int nblk = train_colsum_blocks(R);
    const long long rows_per = (R + nblk - 1) / nblk;
    const dim3 grid(nblk, blocks_for(C, 16));
    {
        ProfScope ps(e, K_TRAIN_BN);
        if (mode == COL_SUM) hipLaunchKernelGGL(train_colsum_kernel<COL_SUM>, grid, dim3(256), 0, e->stream, X, C, R, rows_per, stat, gamma, beta, dA, aw, coff, part);
        else if (mode == COL_VAR) hipLaunchKernelGGL(train_colsum_kernel<COL_VAR>, grid, dim3(256), 0, e->stream, X, C, R, rows_per, stat, gamma, beta, dA, aw, coff, part);
        else hipLaunchKernelGGL(train_colsum_kernel<COL_BNBWD>, grid, dim3(256), 0, e->stream, X, C, R, rows_per, stat, gamma, beta, dA, aw, coff, part);
        RMR_HIP(hipGetLastError());
    }
    ProfScope ps(e, K_TRAIN_REDUCE);
    hipLaunchKernelGGL(train_colsum_final_kernel, dim3((unsigned)C), dim3(64), 0, e->stream, part, nblk, C, what, R, refused, stat, out, out2, run_mean, run_var);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_bn_forward(rmr_engine *e, const float *Y, int C, long long R, float *stat, const float *gamma, const float *beta, float *run_mean,
                     float *run_var, float *part, const int *refused, float *out, int aw, int coff) {
    RMR_TRY(train_colsum(e, COL_SUM, Y, C, R, stat, nullptr, nullptr, nullptr, 0, 0, part, 1, refused, nullptr, nullptr, nullptr, nullptr));
    RMR_TRY(train_colsum(e, COL_VAR, Y, C, R, stat, nullptr, nullptr, nullptr, 0, 0, part, 2, refused, nullptr, nullptr, run_mean, run_var));
    ProfScope ps(e, K_TRAIN_BN);
    hipLaunchKernelGGL(train_bn_swish_kernel, dim3(blocks_for(R * C)), dim3(256), 0, e->stream, Y, C, R * C, stat, gamma, beta, out, aw, coff);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_bn_backward(rmr_engine *e, const float *Y, int C, long long R, float *stat, const float *gamma, const float *beta, const float *dA, int aw,
                      int coff, float *part, const int *refused, float *dgamma, float *dbeta, float *dY, float *dbias) {
    RMR_TRY(train_colsum(e, COL_BNBWD, Y, C, R, stat, gamma, beta, dA, aw, coff, part, 3, refused, dgamma, dbeta, nullptr, nullptr));
    {
        ProfScope ps(e, K_TRAIN_BN);
        hipLaunchKernelGGL(train_bn_bwd_kernel, dim3(blocks_for(R * C)), dim3(256), 0, e->stream, Y, C, R * C, stat, gamma, beta, dA, aw, coff, dY);
        RMR_HIP(hipGetLastError());
    }
    // the convolution's bias gradient: the column sum of dY, zero up to rounding (train-mode BatchNorm removes the channel mean)
    return train_colsum(e, COL_SUM, dY, C, R, stat, nullptr, nullptr, nullptr, 0, 0, part, 0, refused, dbias, nullptr, nullptr, nullptr);
}

int train_bias_grad(rmr_engine *e, const float *D, int C, long long R, float *part, const int *refused, float *out, float *out2) {
    return train_colsum(e, COL_SUM, D, C, R, nullptr, nullptr, nullptr, nullptr, 0, 0, part, 0, refused, out, out2, nullptr, nullptr);
}

int train_sig1(rmr_engine *e, const float *sig, int L, int Lout, int OC, int KW, const float *w, const float *b, long long n, float *y) {
    const long long total = n * Lout * OC;
    ProfScope ps(e, K_TRAIN_AUX);
    hipLaunchKernelGGL(train_sig1_kernel, dim3(blocks_for(total)), dim3(256), 0, e->stream, sig, L, Lout, OC, KW, w, b, total, y);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_seq_transpose(rmr_engine *e, const float *in, int EC, int L, long long n, float *out) {
    const long long total = n * L * EC;
    ProfScope ps(e, K_TRAIN_AUX);
    hipLaunchKernelGGL(train_seq_transpose_kernel, dim3(blocks_for(total)), dim3(256), 0, e->stream, in, EC, L, total, out);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_fill(rmr_engine *e, float *p, long long n, float v, const int *refused) {
    if (n <= 0) return 0;
    ProfScope ps(e, K_TRAIN_AUX);
    hipLaunchKernelGGL(train_fill_kernel, dim3(blocks_for(n)), dim3(256), 0, e->stream, p, n, v, refused);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_lstm_step(rmr_engine *e, float *G, float *Cs, float *H, float *Z, const float *WhhT, int S, int T, int t, long long n) {
    ProfScope ps(e, K_TRAIN_LSTM);
    hipLaunchKernelGGL(train_lstm_step_kernel, dim3(blocks_for(n, 64), S / 16), dim3(256), 0, e->stream, G, Cs, H, Z, WhhT, S, T, t, n);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_lstm_step_bwd(rmr_engine *e, float *G, const float *Cs, const float *H, const float *Whh, const float *dz1, float *dc, int S, int T, int t,
                        long long n) {
    ProfScope ps(e, K_TRAIN_LSTM);
    hipLaunchKernelGGL(train_lstm_step_bwd_kernel, dim3(blocks_for(n, 64), S / 16), dim3(256), 0, e->stream, G, Cs, H, Whh, dz1, dc, S, T, t, n);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_lstm2(rmr_engine *e, float *G2, float *C2, float *H2, float *Z2, int S, long long n) {
    ProfScope ps(e, K_TRAIN_LSTM);
    hipLaunchKernelGGL(train_lstm2_kernel, dim3(blocks_for(n * S)), dim3(256), 0, e->stream, G2, C2, H2, Z2, S, n * S);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_lstm2_bwd(rmr_engine *e, float *G2, const float *C2, const float *H2, const float *dlog, const float *fcw, int num_out, int S, long long n) {
    ProfScope ps(e, K_TRAIN_LSTM);
    hipLaunchKernelGGL(train_lstm2_bwd_kernel, dim3(blocks_for(n * S)), dim3(256), 0, e->stream, G2, C2, H2, dlog, fcw, num_out, S, n * S);
    RMR_HIP(hipGetLastError());
    return 0;
}

// the first launch of a step: count[0] = rows in the loss, count[1] = the first of them with a label outside 0 .. num_out - 1 or -1
int train_count_rows(rmr_engine *e, const uint8_t *mask, const int64_t *labels, int num_out, long long n, int *count) {
    ProfScope ps(e, K_TRAIN_LOSS);
    hipLaunchKernelGGL(train_mask_count_kernel, dim3(1), dim3(256), 0, e->stream, mask, labels, num_out, n, count);
    RMR_HIP(hipGetLastError());
    return 0;
}

// count: what train_count_rows left; loss[0] the mean cross-entropy, loss[1] the bits of count[1]
int train_fc_loss(rmr_engine *e, const float *Z2, const float *fcw, const float *fcb, int S, int num_out, const int64_t *labels, const uint8_t *mask,
                  const int *count, long long n, float *logits, float *dlog, float *loss_part, float *logits_out, float *loss) {
    ProfScope ps(e, K_TRAIN_LOSS);
    hipLaunchKernelGGL(train_fc_loss_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, e->stream, Z2, fcw, fcb, S, num_out, labels, mask, count, n, logits,
                       dlog, loss_part, logits_out);
    hipLaunchKernelGGL(train_loss_reduce_kernel, dim3(1), dim3(256), 0, e->stream, loss_part, n, count, loss);
    RMR_HIP(hipGetLastError());
    return 0;
}

// lr_wd = lr * weight_decay, omb = 1 - beta, step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step): formed in double by the caller
int train_adamw(rmr_engine *e, float *p, float *g, float *m, float *v, const uint8_t *tensor_of, long long n, float lr_wd, float omb1, float b2,
                float omb2, float eps, float step_size, float bc2_sqrt, const float *clip) {
    ProfScope ps(e, K_TRAIN_ADAMW);
    hipLaunchKernelGGL(train_adamw_kernel, dim3(blocks_for(n)), dim3(256), 0, e->stream, p, g, m, v, tensor_of, n, lr_wd, omb1, b2, omb2, eps, step_size, bc2_sqrt, clip);
    RMR_HIP(hipGetLastError());
    return 0;
}

int train_absmax(rmr_engine *e, const float *g, const long long *off, const long long *size, int n_tensors, float *out) {
    ProfScope ps(e, K_TRAIN_ADAMW);
    hipLaunchKernelGGL(train_absmax_kernel, dim3(n_tensors), dim3(256), 0, e->stream, g, off, size, out);
    RMR_HIP(hipGetLastError());
    return 0;
}

}  // namespace rmr
