// Device building blocks shared by the matrix-core kernels (k_*.hip): the vector types of the MFMA operands, the 16-bit
// MFMA wrapper, the fp32 -> 16-bit split of the bf16x3 / bf16x6 / f16x3 pipelines with its part-product schedule, the
// 16-bit packers, the LSTM cell on pre-scaled gate rows and the fast integer division.  Each exists once, here; f32x2 and
// the transcendentals come from rmr_math.h.
#pragma once
#include "rmr_internal.h"
#include "rmr_math.h"

namespace rmr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// x / d for 0 <= x < 2^24, d < 2^12 (make_fastdiv, rmr_internal.h)
__device__ __forceinline__ int fdiv(int x, FastDiv d) { return (int)(((float)x + 0.5f) * d.inv); }

// The 16-bit operand type is a template parameter of every 16-bit kernel: F16 = false -> bf16 (8 exponent / 7 mantissa bits;
// BASELINE configs[3]/[4] name it), true -> IEEE half (5 / 10 bits: eight times finer rounding at the same matrix rate
// - v_mfma_f32_16x16x32_f16 and _bf16 are both 16 cycles; activations here are O(1..10), far from half's 65504).
template <bool F16>
__device__ __forceinline__ f32x4 mfma16(const uint4 a, const uint4 b, const f32x4 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// split x into NP bf16 parts, returned as fp32 bit patterns whose low 16 bits are zero.  F16 (dtype f16x3, NP = 2): two IEEE
// half parts instead - hi = half(x), lo = half(x - hi), each in the high 16 bits of its word like the bf16 parts: 22
// significand bits from three products (hi hi, hi lo, lo hi), where two bf16 parts carry 16
template <int NP, bool F16 = false>
__device__ __forceinline__ void split16(float x, unsigned (&p)[NP]) {
    if constexpr (F16) {
        static_assert(NP == 2, "the half split has two parts");
        const _Float16 hi = (_Float16)x;
        const _Float16 lo = (_Float16)(x - (float)hi);
        p[0] = (unsigned)__builtin_bit_cast(unsigned short, hi) << 16;
        p[1] = (unsigned)__builtin_bit_cast(unsigned short, lo) << 16;
    } else if (NP == 1) {  // round to nearest even
        const unsigned b = __float_as_uint(x);
        p[0] = (b + 0x7fffu + ((b >> 16) & 1u)) & 0xffff0000u;
    } else {
        float r = x;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const unsigned b = __float_as_uint(r);
            if (i + 1 < NP || NP == 3) {
                p[i] = b & 0xffff0000u;  // truncation: exact remainder chain
            } else {
                p[i] = (b + 0x7fffu + ((b >> 16) & 1u)) & 0xffff0000u;  // last of two: round
            }
            r -= __uint_as_float(p[i]);
        }
    }
}

// part-product schedule: pairs (a part, b part)
template <int NP> struct Prod;
template <> struct Prod<1> { static constexpr int N = 1; static constexpr int A[1] = {0}; static constexpr int B[1] = {0}; };
template <> struct Prod<2> { static constexpr int N = 3; static constexpr int A[3] = {0, 0, 1}; static constexpr int B[3] = {0, 1, 0}; };
template <> struct Prod<3> { static constexpr int N = 6; static constexpr int A[6] = {0, 0, 1, 0, 2, 1}; static constexpr int B[6] = {0, 1, 0, 2, 0, 1}; };

// two parts of split16 (fp32 patterns, the value in the high half) -> one dword of two 16-bit elements
__device__ __forceinline__ unsigned pack2(unsigned lo_elem, unsigned hi_elem) { return (lo_elem >> 16) | hi_elem; }
// four fp32 -> four bf16 / half, round to nearest even: 8 bytes
template <bool F16>
__device__ __forceinline__ uint2 pack4(const float a, const float b, const float c, const float d) {
    if constexpr (F16) {
        const f16x4 o = {(_Float16)a, (_Float16)b, (_Float16)c, (_Float16)d};
        return __builtin_bit_cast(uint2, o);
    } else {
        const bf16x4 o = {(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
        return __builtin_bit_cast(uint2, o);
    }
}

// One LSTM unit.  acc rows are pre-scaled on the host: [0] i, [1] f, [3] o by -log2(e); [2] g by 2 log2(e).  c is the cell
// state (updated), the return value is h.
__device__ __forceinline__ float lstm_cell(const f32x4 acc, float &c) {
    const float ig = fast_rcp(1.0f + __builtin_amdgcn_exp2f(acc[0]));
    const float fg = fast_rcp(1.0f + __builtin_amdgcn_exp2f(acc[1]));
    const float gg = fmaf(-2.0f, fast_rcp(1.0f + __builtin_amdgcn_exp2f(acc[2])), 1.0f);
    const float og = fast_rcp(1.0f + __builtin_amdgcn_exp2f(acc[3]));
    c = fmaf(fg, c, ig * gg);
    const float tc = fmaf(-2.0f, fast_rcp(1.0f + __builtin_amdgcn_exp2f(c * 2.8853900817779268f)), 1.0f);
    return og * tc;
}

// The lane's TWO units at once: everything that is not an exp or a rcp works on register pairs (v_pk_add_f32,
// v_pk_fma_f32, v_pk_mul_f32: 11 packed + 20 transcendental instructions instead of 22 + 20; the VALU is the bound of the
// kernels that use it).  Packed and scalar fp32 operations round alike: same bits as two lstm_cell calls, which
// -DRMR_LSTM_PAIRS=0 makes it.
#ifndef RMR_LSTM_PAIRS
#define RMR_LSTM_PAIRS 1
#endif
__device__ __forceinline__ f32x2 exp2_2(const f32x2 v) { return f32x2{__builtin_amdgcn_exp2f(v.x), __builtin_amdgcn_exp2f(v.y)}; }
__device__ __forceinline__ f32x2 rcp_2(const f32x2 v) { return f32x2{fast_rcp(v.x), fast_rcp(v.y)}; }
// Tried and dropped (profiles/r03_lstm_shared_rcp_ab.log): sharing reciprocals - sig(i) tanh(g) = (G - 1) / ((1 + A)(1 + G)),
// sig(o) tanh(c) = (C - 1) / ((1 + O)(1 + C)), 5 exp + 3 rcp per unit instead of 5 + 5 - ran 2.42 against 2.37 ns/chunk: the
// step is bound by the recurrent chain (h -> MFMA -> gates -> h), which the extra multiply in front of each rcp lengthens.
__device__ __forceinline__ f32x2 lstm_cell2(const f32x4 acc0, const f32x4 acc1, float &c0, float &c1) {
    if (!RMR_LSTM_PAIRS) return f32x2{lstm_cell(acc0, c0), lstm_cell(acc1, c1)};
    const f32x2 ig = rcp_2(exp2_2(f32x2{acc0[0], acc1[0]}) + 1.0f);
    const f32x2 fg = rcp_2(exp2_2(f32x2{acc0[1], acc1[1]}) + 1.0f);
    const f32x2 gr = rcp_2(exp2_2(f32x2{acc0[2], acc1[2]}) + 1.0f);
    const f32x2 og = rcp_2(exp2_2(f32x2{acc0[3], acc1[3]}) + 1.0f);
    const f32x2 gg = __builtin_elementwise_fma(f32x2{-2.0f, -2.0f}, gr, f32x2{1.0f, 1.0f});
    const f32x2 c = __builtin_elementwise_fma(fg, f32x2{c0, c1}, ig * gg);
    c0 = c.x;
    c1 = c.y;
    const f32x2 tr = rcp_2(exp2_2(c * 2.8853900817779268f) + 1.0f);
    const f32x2 tc = __builtin_elementwise_fma(f32x2{-2.0f, -2.0f}, tr, f32x2{1.0f, 1.0f});
    return og * tc;
}

}  // namespace rmr
