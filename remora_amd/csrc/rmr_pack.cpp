// rmr_pack.h: parse the canonical blob, fold BN, pack every layer into its kernels' fragment layouts - on the host, no HIP.
#include "rmr_pack.h"

#include <cmath>
#include <cstring>

namespace rmr {

// ---- blob ---------------------------------------------------------------------------------
static size_t conv_count(const ConvSpec &s) { return (size_t)s.oc * s.ic * s.kw + 5 * (size_t)s.oc; }

std::vector<ConvSpec> conv_specs(const rmr_model_desc &d) {
    const int sz = d.size, ec = 4 * d.kmer_len;
    if (d.arch == RMR_ARCH_CONV_LSTM)
        return {{1, 4, 5, 1}, {4, 16, 5, 1}, {16, sz, 9, 3}, {ec, 16, 5, 1}, {16, sz, 13, 3}, {2 * sz, sz, 5, 1}};
    return {{1, 4, 11, 1}, {4, 16, 11, 1}, {16, sz, 9, 3}, {ec, 16, 11, 1}, {16, 32, 11, 1},
            {32, sz, 9, 3}, {2 * sz, sz, 5, 1}, {sz, sz, 5, 1}, {sz, sz, 3, 2}, {sz, sz, 3, 2}};
}

// The channel count the kernels run a network of `size` channels at (models/ConvLSTM_w_ref.py:11-37 and Conv_w_ref.py:11-42
// are parametric in `size`, the CLI takes any int: src/remora/parsers.py:858-862).  Up to 64 the kernels with register-resident
// weight slices exist for 16 / 32 / 64; above, the streamed-weight kernels (k_stream.hip) take any multiple of 16 up to 256.
// Channels between `size` and the padded count carry zero weights and zero bias: swish(0) = 0 and an LSTM unit with zero
// weights stays at c = h = 0 exactly, and a zero product added to an fp32 sum leaves it unchanged - the logits are those of
// the unpadded network (pad_model_blob below; rmr_model_pad_weights exposes the transform).
int padded_size(int size, int dtype) {
    if (size <= 16) return 16;
    if (size <= 32) return 32;
    if (size <= 64) return 64;
    return dtype == 0 ? (size + 15) & ~15 : (size + 31) & ~31;  // the 16-bit MFMA takes K in steps of 32 (k_stream16.hip)
}

bool desc_ok(const rmr_model_desc &d) {
    if (d.arch != RMR_ARCH_CONV_LSTM && d.arch != RMR_ARCH_CONV_ONLY) return false;
    if (d.size < 1 || d.dtype < 0 || d.dtype > 5 || padded_size(d.size, d.dtype) > kMaxPaddedSize) return false;
    const int sp = padded_size(d.size, d.dtype);
    if (d.kmer_len < 1 || d.kmer_len > 64) return false;
    if (d.num_out < 1 || d.num_out > 16) return false;
    if (d.dtype < 0 || d.dtype > 5) return false;  // 5 = f16x3: two-part IEEE half split on the unfused kernels
    if (d.dtype == 4 && sp <= 64 && (sp != 64 || (d.kmer_len != 9 && d.kmer_len != 6))) return false;  // half up to 64 channels: the fused kernels only
    if (d.dtype != 0 && (d.arch != RMR_ARCH_CONV_LSTM || sp % 32)) return false;
    if (d.dtype != 0 && sp > 64 && d.dtype != 1 && d.dtype != 4) return false;  // above 64 channels: fp32, bf16 or f16 (the split dtypes stop at 64)
    return true;
}

size_t weight_count(const rmr_model_desc &d) {
    size_t n = 0;
    for (auto &s : conv_specs(d)) n += conv_count(s);
    const size_t H = d.size;
    if (d.arch == RMR_ARCH_CONV_LSTM) {
        n += 2 * (2 * 4 * H * H + 2 * 4 * H);
        n += (size_t)d.num_out * H + d.num_out;
    } else {
        n += (size_t)d.num_out * H * 3 + d.num_out;
    }
    return n;
}

// The canonical blob (include/remora_hip.h, rmr_model_create) of the same network with `sp` channels where `d` has d.size:
// zero weights / bias for the added output channels (BatchNorm of an added channel: gamma 1, beta 0, mean 0, var 1 - it folds
// to weight 0, bias 0), zero columns for the added input channels; merge_conv1 reads cat = [signal branch | sequence branch],
// so its input channel sz + c moves to sp + c.
std::vector<float> pad_model_blob(const rmr_model_desc &d, const float *w, int sp) {
    const int sz = d.size;
    rmr_model_desc pd = d;
    pd.size = sp;
    const std::vector<ConvSpec> ts = conv_specs(d), ps = conv_specs(pd);
    size_t total = 0;
    for (auto &s : ps) total += conv_count(s);
    const size_t H = sz, HP = sp;
    if (d.arch == RMR_ARCH_CONV_LSTM) total += 2 * (2 * 4 * HP * HP + 2 * 4 * HP) + (size_t)d.num_out * HP + d.num_out;
    else total += (size_t)d.num_out * HP * 3 + d.num_out;
    std::vector<float> o(total, 0.0f);
    const float *p = w;
    float *q = o.data();
    const size_t merge1 = d.arch == RMR_ARCH_CONV_LSTM ? 5 : 6;
    for (size_t li = 0; li < ts.size(); ++li) {
        const ConvSpec &t = ts[li], &u = ps[li];
        for (int oc = 0; oc < t.oc; ++oc)
            for (int ic = 0; ic < t.ic; ++ic) {
                const int icp = (li == merge1 && ic >= sz) ? sp + (ic - sz) : ic;
                memcpy(q + ((size_t)oc * u.ic + icp) * u.kw, p + ((size_t)oc * t.ic + ic) * t.kw, (size_t)t.kw * sizeof(float));
            }
        p += (size_t)t.oc * t.ic * t.kw;
        q += (size_t)u.oc * u.ic * u.kw;
        for (int part = 0; part < 5; ++part) {  // bias, gamma, beta, mean, var
            memcpy(q, p, (size_t)t.oc * sizeof(float));
            if (part == 1 || part == 4)
                for (int oc = t.oc; oc < u.oc; ++oc) q[oc] = 1.0f;
            p += t.oc;
            q += u.oc;
        }
    }
    if (d.arch == RMR_ARCH_CONV_LSTM) {
        for (int l = 0; l < 2; ++l) {
            for (int m = 0; m < 2; ++m) {  // weight_ih, weight_hh: [4H][H], row = gate * H + unit
                for (int g = 0; g < 4; ++g)
                    for (size_t r = 0; r < H; ++r) memcpy(q + ((size_t)g * HP + r) * HP, p + ((size_t)g * H + r) * H, H * sizeof(float));
                p += 4 * H * H;
                q += 4 * HP * HP;
            }
            for (int m = 0; m < 2; ++m) {  // bias_ih, bias_hh: [4H]
                for (int g = 0; g < 4; ++g) memcpy(q + (size_t)g * HP, p + (size_t)g * H, H * sizeof(float));
                p += 4 * H;
                q += 4 * HP;
            }
        }
        for (int oo = 0; oo < d.num_out; ++oo) memcpy(q + (size_t)oo * HP, p + (size_t)oo * H, H * sizeof(float));
        p += (size_t)d.num_out * H;
        q += (size_t)d.num_out * HP;
    } else {  // fc over flatten([size][3]): index c * 3 + t, channels first - the added channels sit behind the real ones
        for (int oo = 0; oo < d.num_out; ++oo) memcpy(q + (size_t)oo * HP * 3, p + (size_t)oo * H * 3, H * 3 * sizeof(float));
        p += (size_t)d.num_out * H * 3;
        q += (size_t)d.num_out * HP * 3;
    }
    memcpy(q, p, (size_t)d.num_out * sizeof(float));
    return o;
}

Folded fold(const ConvSpec &s, const float *&p) {
    Folded f;
    f.s = s;
    const size_t nw = (size_t)s.oc * s.ic * s.kw;
    const float *w = p; p += nw;
    const float *b = p; p += s.oc;
    const float *g = p; p += s.oc;
    const float *beta = p; p += s.oc;
    const float *mean = p; p += s.oc;
    const float *var = p; p += s.oc;
    f.w.resize(nw);
    f.b.resize(s.oc);
    for (int o = 0; o < s.oc; ++o) {
        // eval-mode BatchNorm1d, eps = 1e-5 (torch default; the reference folds the same
        // way for its Dorado export, src/remora/model_util.py:199-221)
        const double sc = (double)g[o] / std::sqrt((double)var[o] + 1e-5);
        for (size_t i = 0; i < (size_t)s.ic * s.kw; ++i)
            f.w[(size_t)o * s.ic * s.kw + i] = (float)((double)w[(size_t)o * s.ic * s.kw + i] * sc);
        f.b[o] = (float)(((double)b[o] - (double)mean[o]) * sc + (double)beta[o]);
    }
    return f;
}

// ---- fragment packers ---------------------------------------------------------------------
// fp32 A fragments of the 16x16x4 MFMA: lane (q, m) of k group g holds k = 16 g + 4 q + j (j = 0..3) of row m of the tile;
// `by_lane` false: [tile][group][j][64 lanes] (one dword per lane and k-step), true: [tile][group][64 lanes][4 j] (16 B per lane)
template <class At>
static std::vector<float> pack_a32(int tiles, int groups, bool by_lane, At at /* (tile, m, k) -> float */) {
    std::vector<float> o((size_t)tiles * groups * 256);
    for (int t = 0; t < tiles; ++t)
        for (int g = 0; g < groups; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j)
                    o[((size_t)t * groups + g) * 256 + (by_lane ? lane * 4 + j : j * 64 + lane)] = at(t, lane & 15, 16 * g + 4 * (lane >> 4) + j);
    return o;
}

static inline uint32_t f2u(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static inline float u2f(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
static inline uint32_t rne_bf16(uint32_t b) { return (b + 0x7fffu + ((b >> 16) & 1u)) & 0xffff0000u; }
static inline uint32_t half_hi(_Float16 h) { uint16_t b; memcpy(&b, &h, 2); return (uint32_t)b << 16; }
// One fp32 value as np 16-bit operand parts, each in the HIGH half of its word (host twin of the device split16 in rmr_mma.h).
// bf16: the parts before the last truncated, each taking what the previous ones left of x; the last rounded to nearest even
// (np = 1, 2) or truncated (np = 3).  f16: hi = half(x) (round to nearest even; the compiler's conversion), np = 2 adds
// lo = half(x - hi) (dtype f16x3).
static void split16(float x, int np, bool f16, uint32_t *p) {
    if (f16) {
        const _Float16 hi = (_Float16)x;
        p[0] = half_hi(hi);
        if (np > 1) p[1] = half_hi((_Float16)(x - (float)hi));
        return;
    }
    float r = x;
    for (int i = 0; i < np; ++i) {
        const uint32_t b = f2u(r);
        p[i] = (i + 1 < np || np == 3) ? (b & 0xffff0000u) : rne_bf16(b);
        r -= u2f(p[i]);
    }
}

// 16-bit A fragments of the 16x16x32 MFMA: lane (q, m) of k-step s holds k = 32 s + 8 q + j (j = 0..7) of row m of the tile,
// two values per dword (even j in the low half), as np split parts: [tile][k-step][np][64 lanes][4 dwords]
template <class At>
static std::vector<float> pack_a16(int tiles, int ksteps, int np, bool f16, At at /* (tile, m, k) -> float */) {
    std::vector<uint32_t> o((size_t)tiles * ksteps * np * 256);
    for (int t = 0; t < tiles; ++t)
        for (int s = 0; s < ksteps; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                uint32_t parts[8][3];
                for (int j = 0; j < 8; ++j) split16(at(t, lane & 15, 32 * s + 8 * (lane >> 4) + j), np, f16, parts[j]);
                for (int p = 0; p < np; ++p)
                    for (int i = 0; i < 4; ++i)
                        o[(((size_t)t * ksteps + s) * np + p) * 256 + lane * 4 + i] = (parts[2 * i][p] >> 16) | parts[2 * i + 1][p];
            }
    std::vector<float> f(o.size());
    memcpy(f.data(), o.data(), o.size() * 4);
    return f;
}

// conv weights as 16-bit A fragments [oc/16][ksteps][np][64 lanes] x 16 B, k = tap * C + channel (C >= ic: the row width of
// the operand in LDS); taps >= kw and channels >= ic are zero; `scale` applied in float64
static std::vector<float> conv_a16(const Folded &f, int C, int ksteps, int np, bool f16, double scale = 1.0) {
    const ConvSpec &s = f.s;
    return pack_a16(s.oc / 16, ksteps, np, f16, [&](int t, int m, int k) {
        const int tap = k / C, ch = k % C;
        return tap < s.kw && ch < s.ic ? (float)(scale * (double)f.w[((size_t)(16 * t + m) * s.ic + ch) * s.kw + tap]) : 0.0f;
    });
}

// Winograd F(4, 5) and F(4, 3) filter transforms in natural point order (0, 1, -1, 2, -2, [1/2, -1/2,] inf): k_wino.hip and
// k_conv_front.hip hold BT and AT; oracle/winograd.py derives all three.  The kernels' x orders put the points 1, -1, 2, -2
// in wave half 0 and 0, 1/2, -1/2, inf in half 1 (F(4, 5)), or +1, -1, 0 and +2, -2, inf (F(4, 3)).
const double G5[8][5] = {{1.0 / 4, 0, 0, 0, 0},
                         {1.0 / 18, 1.0 / 18, 1.0 / 18, 1.0 / 18, 1.0 / 18},
                         {1.0 / 18, -1.0 / 18, 1.0 / 18, -1.0 / 18, 1.0 / 18},
                         {1.0 / 360, 1.0 / 180, 1.0 / 90, 1.0 / 45, 2.0 / 45},
                         {1.0 / 360, -1.0 / 180, 1.0 / 90, -1.0 / 45, 2.0 / 45},
                         {16.0 / 45, 8.0 / 45, 4.0 / 45, 2.0 / 45, 1.0 / 45},
                         {16.0 / 45, -8.0 / 45, 4.0 / 45, -2.0 / 45, 1.0 / 45},
                         {0, 0, 0, 0, 1.0 / 4}};
const double G3[6][3] = {{1.0 / 4, 0, 0}, {1.0 / 6, 1.0 / 6, 1.0 / 6}, {1.0 / 6, -1.0 / 6, 1.0 / 6},
                         {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1.0}};
const int F45_KERNEL_ORDER[8] = {1, 2, 3, 4, 0, 5, 6, 7}, F43_KERNEL_ORDER[6] = {1, 2, 0, 3, 4, 5};
const int NATURAL_ORDER[8] = {0, 1, 2, 3, 4, 5, 6, 7};

// in float64 from the folded fp32 weights, ONE rounding to fp32; taps past the layer's width (3 t + p >= kw) are zero
std::vector<float> wino_filter(const Folded &f, const double *G, int r, const int *order, int nx, int P) {
    const ConvSpec &s = f.s;
    const int NG = s.ic / 16;
    return pack_a32(s.oc / 16, nx * P * NG, false, [&](int t, int m, int k) {
        const int grp = k >> 4, ic = 16 * (grp % NG) + (k & 15), p = grp / NG % P, x = order[grp / NG / P];
        double u = 0.0;
        for (int tap = 0; tap < r; ++tap)
            if (P * tap + p < s.kw) u += G[x * r + tap] * (double)f.w[((size_t)(16 * t + m) * s.ic + ic) * s.kw + P * tap + p];
        return (float)u;
    });
}

// gate pre-scale used by lstm_step (k_lstm.hip): sigmoid(x) = 1/(1+2^(-x log2 e)) for i,f,o;
// tanh(x) = 1 - 2/(1+2^(2x log2 e)) for g.  torch gate order i,f,g,o.
static const double kLog2e = 1.4426950408889634;
static inline double gate_scale(int gate) { return gate == 2 ? 2.0 * kLog2e : -kLog2e; }

// [4H][H] row-major (row = gate * H + unit) -> fp32 fragments, 16 units of gate gates[gi] per tile, pre-scaled if `prescale`:
// [H/16 waves][ngates][H/4 k-steps][64] (k_lstm.hip), or `stream`: [H/16 waves][H/16 k groups][ngates][64 lanes][4] (k_stream.hip)
static std::vector<float> lstm_a32(const float *w, int H, const int *gates, int ngates, bool prescale, bool stream) {
    const int W = H / 16;
    auto at = [&](int wv, int gi, int m, int k) {
        const double sc = prescale ? gate_scale(gates[gi]) : 1.0;
        return (float)((double)w[(size_t)(gates[gi] * H + 16 * wv + m) * H + k] * sc);
    };
    if (stream)
        return pack_a32(W, W * ngates, true, [&](int t, int m, int k) { return at(t, (k >> 4) % ngates, m, 16 * ((k >> 4) / ngates) + (k & 15)); });
    return pack_a32(W * ngates, W, false, [&](int t, int m, int k) { return at(t / ngates, t % ngates, m, k); });
}

// [4H][H] row-major (H = 64) -> [4 waves][64 k in lstm_head_kernel's order: position (g * 4 + j) * 4 + q = k 16 g + 4 q + j][64 lanes],
// lane l = gate gates[l & 3] (a negative entry: zeros) of unit 16 w + (l >> 2)   (lstm_small_kernel, k_lstm.hip)
static std::vector<float> lstm_small(const float *w, const int *gates, bool prescale) {
    const int H = 64;
    std::vector<float> ap((size_t)4 * H * 64);
    for (int wv = 0; wv < 4; ++wv)
        for (int g = 0; g < 4; ++g)
            for (int j = 0; j < 4; ++j)
                for (int q = 0; q < 4; ++q)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int gate = gates[lane & 3], unit = 16 * wv + (lane >> 2), k = 16 * g + 4 * q + j;
                        const double sc = prescale && gate >= 0 ? gate_scale(gate) : 1.0;
                        ap[((size_t)wv * H + (g * 4 + j) * 4 + q) * 64 + lane] =
                            gate < 0 ? 0.0f : (float)((double)w[(size_t)(gate * H + unit) * H + k] * sc);
                    }
    return ap;
}

// LSTM weights as 16-bit tiles with UNIT-MAJOR rows, T tiles per wave: row m of tile t of wave wv is (unit 4T wv + T (m >> 2) + t,
// gate m & 3): [H/4T waves][T][H/32 k-steps][np][64 lanes] x 16 B; gate rows pre-scaled; `skip_f` zeroes the f rows (lstm2:
// c0 = 0).  T = 2: k_lstm_x16.hip / k_lstm_x16s.hip (H = 64); T = 4: k_stream16.hip (H above 64)
static std::vector<float> lstm_units_a16(const float *w, int H, int T, bool skip_f, int np, bool f16) {
    return pack_a16(H / 4, H / 32, np, f16, [&](int tile, int m, int k) {
        const int gate = m & 3, unit = 4 * T * (tile / T) + T * (m >> 2) + tile % T;
        return (skip_f && gate == 1) ? 0.0f : (float)((double)w[(size_t)(gate * H + unit) * H + k] * gate_scale(gate));
    });
}
// matching biases [H/4T][T][4 q][4 gates]: (b_ih + b_hh) of unit 4T wv + T q + t, pre-scaled
static std::vector<float> lstm_units_bias(const float *bih, const float *bhh, int H, int T, bool skip_f) {
    std::vector<float> o((size_t)4 * H);
    for (int i = 0; i < 4 * H; ++i) {
        const int gate = i & 3, tile = i >> 4, unit = 4 * T * (tile / T) + T * ((i >> 2) & 3) + tile % T;
        o[i] = (skip_f && gate == 1) ? 0.0f : (float)(((double)bih[gate * H + unit] + (double)bhh[gate * H + unit]) * gate_scale(gate));
    }
    return o;
}

// ---- front: sig_conv1, sig_conv2, seq_conv1 on the VALU ----------------------------------------
// [oc][ic][kw] -> [kw][ic][oc], `scale` applied in float64 (w_sig1 [kw][4], w_sig2 [kw][4][16], wt_seq1 [kw][EC][16])
static std::vector<float> tap_major(const Folded &f, double scale = 1.0) {
    const ConvSpec &s = f.s;
    std::vector<float> o(f.w.size());
    for (int t = 0; t < s.kw; ++t)
        for (int ic = 0; ic < s.ic; ++ic)
            for (int oc = 0; oc < s.oc; ++oc)
                o[((size_t)t * s.ic + ic) * s.oc + oc] = (float)((double)f.w[((size_t)oc * s.ic + ic) * s.kw + t] * scale);
    return o;
}
// seq_conv1 as the gather table of k-mer position kp and base b: [kw][K][5][16], row 4 = zeros (missing base)
static std::vector<float> seq1_gather_table(const Folded &q1, int K) {
    const int kw = q1.s.kw, ec = q1.s.ic;
    std::vector<float> o((size_t)kw * K * 80, 0.0f);
    for (int t = 0; t < kw; ++t)
        for (int kp = 0; kp < K; ++kp)
            for (int b = 0; b < 4; ++b)
                for (int oc = 0; oc < 16; ++oc) o[(((size_t)t * K + kp) * 5 + b) * 16 + oc] = q1.w[((size_t)oc * ec + 4 * kp + b) * kw + t];
    return o;
}
static std::vector<float> scaled(const std::vector<float> &v, double scale) {
    std::vector<float> o(v.size());
    for (size_t i = 0; i < v.size(); ++i) o[i] = (float)((double)v[i] * scale);
    return o;
}

// ---- per model ------------------------------------------------------------------------------
// one conv layer on the fp32 MFMA path: the direct form's fragments (k = tap * ic + channel), the bias, and U = G W where a
// Winograd kernel takes the layer (k_wino.hip, k_conv_front.hip)
static int pack_conv(const Folded &f, const std::string &name, ConvLayer *out, const Upload &upload) {
    const ConvSpec &s = f.s;
    if (s.ic % 16 || s.oc % 16) RMR_FAIL(RMR_ERR_INVALID, "conv %dx%d not MFMA-tileable", s.ic, s.oc);
    out->ic = s.ic; out->oc = s.oc; out->kw = s.kw; out->stride = s.stride;
    const bool streamed = s.oc > 64 || s.ic > 128;  // a layer of a network with more than 64 channels: k_stream.hip's order
    const std::vector<float> ap = pack_a32(s.oc / 16, s.kw * s.ic / 16, streamed, [&](int t, int m, int k) {
        return f.w[((size_t)(16 * t + m) * s.ic + k % s.ic) * s.kw + k / s.ic];
    });
    RMR_TRY(upload(name + (streamed ? ".apack4" : ".apack"), ap, streamed ? &out->apack4 : &out->apack));
    RMR_TRY(upload(name + ".bias", f.b, &out->bias));
    if (streamed || s.oc != 64) return 0;
    if (s.stride == 1 && s.kw == 5 && (s.ic == 64 || s.ic == 128))  // merge_conv1 / merge_conv2: F(4, 5), wino_kernel's x order
        return upload(name + ".wpack", wino_filter(f, G5[0], 5, F45_KERNEL_ORDER, 8, 1), &out->wpack);
    // stride 3 as three phase filters w_p[m] = w[3 m + p]: sig_conv3 (sig3_front_wino_kernel; 3 taps, F(4, 3), natural order),
    // Conv_w_ref's seq_conv3 (wino_s3_kernel; F(4, 3) in its x order, K of a point's GEMM = (phase, channel)), seq_conv2
    // (seq2_front_wino_kernel; 5, 4 and 4 taps, all as F(4, 5) with a zero fifth tap, natural order)
    if (s.stride == 3 && s.kw == 9 && (s.ic == 16 || s.ic == 32))
        return upload(name + ".wpack", wino_filter(f, G3[0], 3, s.ic == 16 ? NATURAL_ORDER : F43_KERNEL_ORDER, 6, 3), &out->wpack);
    if (s.stride == 3 && s.kw == 13 && s.ic == 16) return upload(name + ".wpack", wino_filter(f, G5[0], 5, NATURAL_ORDER, 8, 3), &out->wpack);
    return 0;
}

// 16-bit A fragments of a whole layer, k = tap * ic + channel: the split parts of k_conv_bf16s.hip (ic 16 or a multiple of
// 32: a k-step never straddles two taps except in pairs of 16-channel taps), or one part for k_stream16.hip
static int pack_conv16(const Folded &f, int np, bool f16, float **dev, const std::string &name, const Upload &upload) {
    const ConvSpec &s = f.s;
    if (s.ic != 16 && s.ic % 32) RMR_FAIL(RMR_ERR_INVALID, "split conv needs ic 16 or a multiple of 32 (got %d)", s.ic);
    return upload(name, conv_a16(f, s.ic, (s.kw * s.ic + 31) / 32, np, f16), dev);
}

int pack_model(const rmr_model_desc &desc, const float *weights, size_t n_floats, ModelWeights *m, const Upload &upload) {
    const size_t want = weight_count(desc);
    if (want != n_floats) RMR_FAIL(RMR_ERR_INVALID, "internal: padded weight blob has %zu floats, expected %zu", n_floats, want);
    m->desc = desc;
    m->nparts = desc.dtype == 4 ? 1 : (desc.dtype == 5 ? 2 : desc.dtype);  // 0 fp32 MFMA; 1 bf16; 2 bf16x3 (2-part split); 3 bf16x6 (3-part split)
    m->split_f16 = desc.dtype == 5;  // f16x3: the two parts are IEEE half
    m->f16 = desc.dtype == 4;        // 4: one-part operands as IEEE half (fused kernels)
    const int sz = desc.size, K = desc.kmer_len, L = desc.chunk_len, np = m->nparts;

    const float *p = weights;
    std::vector<Folded> convs;
    for (auto &s : conv_specs(desc)) convs.push_back(fold(s, p));

    // ---- geometry ----
    const int kw1 = convs[0].s.kw;
    m->L = L;
    m->P1 = L - kw1 + 1;
    m->P2 = m->P1 - kw1 + 1;
    if (m->P2 < 9) RMR_FAIL(RMR_ERR_INVALID, "chunk_len %d too short for this architecture", L);
    m->P3 = (m->P2 - 9) / 3 + 1;
    if (desc.arch == RMR_ARCH_CONV_LSTM) {
        if ((m->P1 - 13) / 3 + 1 != m->P3) RMR_FAIL(RMR_ERR_INVALID, "branch lengths differ");
        m->T = m->P3 - 4;
        if (m->T < 1) RMR_FAIL(RMR_ERR_INVALID, "chunk_len %d too short", L);
    } else {
        m->PQ2 = m->P1 - 10;
        if (m->PQ2 < 9 || (m->PQ2 - 9) / 3 + 1 != m->P3) RMR_FAIL(RMR_ERR_INVALID, "branch lengths differ");
        m->T = m->P3 - 4;
        m->T2 = m->T - 4;
        m->T3 = (m->T2 - 3) / 2 + 1;
        m->T4 = (m->T3 - 3) / 2 + 1;
        if (m->T2 < 3 || m->T3 < 3 || m->T4 != 3)
            RMR_FAIL(RMR_ERR_INVALID, "Conv_w_ref needs 3 final positions (fc in = size*3), chunk_len %d gives %d", L, m->T4);
    }

#define PUT(field, host) RMR_TRY(upload(#field, host, &m->field))
    // ---- front weights ----
    m->front.kw1 = kw1;
    PUT(front.w_sig1, tap_major(convs[0]));
    PUT(front.b_sig1, convs[0].b);
    PUT(front.w_sig2, tap_major(convs[1]));
    PUT(front.b_sig2, convs[1].b);
    PUT(front.wt_seq1, tap_major(convs[3]));
    PUT(front.wt5_seq1, seq1_gather_table(convs[3], K));
    PUT(front.b_seq1, convs[3].b);
    RMR_TRY(pack_conv(convs[2], "sig3", &m->sig3, upload));
    RMR_TRY(pack_conv(convs[4], "seq2", &m->seq2, upload));
    if (desc.arch != RMR_ARCH_CONV_LSTM) {
        RMR_TRY(pack_conv(convs[5], "seq3", &m->seq3, upload));
        RMR_TRY(pack_conv(convs[6], "merge1", &m->merge1, upload));
        RMR_TRY(pack_conv(convs[7], "merge2", &m->merge2, upload));
        RMR_TRY(pack_conv(convs[8], "merge3", &m->merge3, upload));
        RMR_TRY(pack_conv(convs[9], "merge4", &m->merge4, upload));
        const float *wfc = p; p += (size_t)desc.num_out * sz * 3;
        const float *bfc = p; p += desc.num_out;
        PUT(w_fc, std::vector<float>(wfc, wfc + (size_t)desc.num_out * sz * 3));
        PUT(b_fc, std::vector<float>(bfc, bfc + desc.num_out));
    } else {
        RMR_TRY(pack_conv(convs[5], "merge1", &m->merge1, upload));
        if (np > 0) {
            for (ConvLayer *c : {&m->sig3, &m->seq2, &m->merge1}) c->split_f16 = m->split_f16;
            RMR_TRY(pack_conv16(convs[2], np, m->split_f16, &m->sig3.spack, "sig3.spack", upload));
            RMR_TRY(pack_conv16(convs[4], np, m->split_f16, &m->seq2.spack, "seq2.spack", upload));
            RMR_TRY(pack_conv16(convs[5], np, m->split_f16, &m->merge1.spack, "merge1.spack", upload));
        }
        if (np == 1 && sz > 64) {  // k_stream16.hip: the three size-wide layers
            RMR_TRY(pack_conv16(convs[2], 1, m->f16, &m->sig3.apack16, "sig3.apack16", upload));
            RMR_TRY(pack_conv16(convs[4], 1, m->f16, &m->seq2.apack16, "seq2.apack16", upload));
            RMR_TRY(pack_conv16(convs[5], 1, m->f16, &m->merge1.apack16, "merge1.apack16", upload));
        }
        if (np == 1 && sz == 64 && (K == 9 || K == 6) && kw1 == 5) {  // operands of the fused front kernel
            const int cg = (4 * K + 7) / 8;
            PUT(fused.a_sig2, conv_a16(convs[1], 4, 1, 1, m->f16));
            PUT(fused.a_seq1, conv_a16(convs[3], 8 * cg, (5 * cg * 8 + 31) / 32, 1, m->f16, kLog2e));
            PUT(fused.a_sig3, conv_a16(convs[2], 16, 5, 1, m->f16));
            PUT(fused.a_seq2, conv_a16(convs[4], 16, 7, 1, m->f16));
            PUT(fused.a_merge1, conv_a16(convs[5], 2 * sz, 20, 1, m->f16));
            PUT(fused.w_sig1, tap_major(convs[0], kLog2e));
            PUT(fused.b_sig1, scaled(convs[0].b, kLog2e));
            PUT(fused.b_sig2, scaled(convs[1].b, kLog2e));
            PUT(fused.b_seq1, scaled(convs[3].b, kLog2e));
            PUT(fused.b_sig3, scaled(convs[2].b, kLog2e));
            PUT(fused.b_seq2, scaled(convs[4].b, kLog2e));
            PUT(fused.b_merge1, scaled(convs[5].b, kLog2e));
        }
        const int H = sz;
        const float *wih1 = p; p += (size_t)4 * H * H;
        const float *whh1 = p; p += (size_t)4 * H * H;
        const float *bih1 = p; p += 4 * H;
        const float *bhh1 = p; p += 4 * H;
        const float *wih2 = p; p += (size_t)4 * H * H;
        p += (size_t)4 * H * H;  // lstm2.weight_hh_l0 multiplies h0 == 0: never reaches the output
        const float *bih2 = p; p += 4 * H;
        const float *bhh2 = p; p += 4 * H;
        const float *wfc = p; p += (size_t)desc.num_out * H;
        const float *bfc = p; p += desc.num_out;
        const int g4[4] = {0, 1, 2, 3}, g3[3] = {0, 2, 3};
        if (H > 64) {  // k_stream.hip
            PUT(lstm.t_ih1, lstm_a32(wih1, H, g4, 4, true, true));
            PUT(lstm.t_hh1, lstm_a32(whh1, H, g4, 4, true, true));
            PUT(lstm.t_ih2, lstm_a32(wih2, H, g3, 3, false, true));
        } else {
            PUT(lstm.a_ih1, lstm_a32(wih1, H, g4, 4, true, false));
            PUT(lstm.a_hh1, lstm_a32(whh1, H, g4, 4, true, false));
            PUT(lstm.a_ih2, lstm_a32(wih2, H, g3, 3, false, false));
            if (H == 64 && np == 0) {  // the four-chunk kernel of small batches (one read per call)
                const int g3z[4] = {0, 2, 3, -1};
                PUT(lstm.q_ih1, lstm_small(wih1, g4, true));
                PUT(lstm.q_hh1, lstm_small(whh1, g4, true));
                PUT(lstm.q_ih2, lstm_small(wih2, g3z, false));
            }
        }
        if (np > 0) {  // gate-major split fragments: 16 units of one gate per tile, [H/16 waves][4 gates] tiles, pre-scaled
            auto split_a = [&](const float *w) {
                return pack_a16(H / 4, H / 32, np, m->split_f16, [&](int t, int mm, int k) {
                    return (float)((double)w[(size_t)((t % 4) * H + 16 * (t / 4) + mm) * H + k] * gate_scale(t % 4));
                });
            };
            PUT(lstm.s_ih1, split_a(wih1));
            PUT(lstm.s_hh1, split_a(whh1));
        }
        if (np >= 2 && H == 64) {  // split operands in the x16 layout (k_lstm_x16s.hip)
            PUT(lstm.xs_ih, lstm_units_a16(wih1, H, 2, false, np, m->split_f16));
            PUT(lstm.xs_hh, lstm_units_a16(whh1, H, 2, false, np, m->split_f16));
            PUT(lstm.xs_ih2, lstm_units_a16(wih2, H, 2, true, np, m->split_f16));
        }
        if (np == 1 && H > 64) {  // k_stream16.hip
            PUT(lstm.s16_ih, lstm_units_a16(wih1, H, 4, false, 1, m->f16));
            PUT(lstm.s16_hh, lstm_units_a16(whh1, H, 4, false, 1, m->f16));
            PUT(lstm.s16_ih2, lstm_units_a16(wih2, H, 4, true, 1, m->f16));
            PUT(lstm.s16_b1, lstm_units_bias(bih1, bhh1, H, 4, false));
            PUT(lstm.s16_b2, lstm_units_bias(bih2, bhh2, H, 4, true));
        }
        if (np == 1 && H == 64) {  // k_lstm_x16.hip
            PUT(lstm.x_ih, lstm_units_a16(wih1, H, 2, false, 1, m->f16));
            PUT(lstm.x_hh, lstm_units_a16(whh1, H, 2, false, 1, m->f16));
            PUT(lstm.x_ih2, lstm_units_a16(wih2, H, 2, true, 1, m->f16));
        }
        if (np >= 1 && H == 64) {
            PUT(lstm.x_b1, lstm_units_bias(bih1, bhh1, H, 2, false));
            PUT(lstm.x_b2, lstm_units_bias(bih2, bhh2, H, 2, true));
        }
        std::vector<float> b1(4 * H), b2(3 * H);
        for (int i = 0; i < 4 * H; ++i) b1[i] = (float)(((double)bih1[i] + (double)bhh1[i]) * gate_scale(i / H));
        for (int gi = 0; gi < 3; ++gi)
            for (int u = 0; u < H; ++u) b2[gi * H + u] = bih2[g3[gi] * H + u] + bhh2[g3[gi] * H + u];
        PUT(lstm.b1, b1);
        PUT(lstm.b2, b2);
        PUT(lstm.w_fc, std::vector<float>(wfc, wfc + (size_t)desc.num_out * H));
        PUT(lstm.b_fc, std::vector<float>(bfc, bfc + desc.num_out));
    }
#undef PUT
    if ((size_t)(p - weights) != n_floats) RMR_FAIL(RMR_ERR_INVALID, "internal: blob walk mismatch");
    return 0;
}

}  // namespace rmr
