// The weights of a model as the kernels read them: the canonical blob (include/remora_hip.h, rmr_model_create) parsed,
// BatchNorm folded, and every layer packed into the fragment layouts of its kernels.  Plain C++, no HIP: pack_model hands
// each finished host buffer to an `upload` callback - api_forward.hip copies it to the device, tests/c/model_packs.cpp digests
// it on the CPU.  rmr_pack.cpp holds the code.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/remora_hip.h"

namespace rmr {

// ---- error plumbing -------------------------------------------------------------------
void set_error(const char *fmt, ...);
#define RMR_FAIL(code, ...)            \
    do {                               \
        ::rmr::set_error(__VA_ARGS__); \
        return (code);                 \
    } while (0)
#define RMR_TRY(expr)          \
    do {                       \
        int _rc = (expr);      \
        if (_rc != 0) return _rc; \
    } while (0)

// One convolution executed on the MFMA path: out[oc][n] = sum_{tap,ic} W[oc][ic][tap] * in
struct ConvLayer {
    int ic = 0, oc = 0, kw = 0, stride = 1;
    float *apack = nullptr;  // device, fragment order [oc/16][kw*ic/4][64]
    float *wpack = nullptr;  // device, Winograd F(4,5) fragments U = G W: [oc/16][8 * ic/4][64] (k_wino.hip; fp32 5-tap stride-1 layers of 64 output channels)
    float *apack4 = nullptr; // device, streamed-kernel order [oc/16][kw*ic/16][64][4] (k_stream.hip; layers of networks with > 64 channels)
    float *apack16 = nullptr; // device, 16-bit A fragments [oc/16][ceil(kw*ic/32)][64 lanes] x 16 B, k = tap * ic + channel (k_stream16.hip)
    float *spack = nullptr;  // device, split-bf16 fragments [oc/16][steps][nparts][64] x 16 B (dtype != 0)
    float *bias = nullptr;   // device, folded bias [oc]
    int kid = 0;             // profiling id
    bool split_f16 = false;  // spack holds two IEEE half parts (dtype f16x3) instead of bf16 parts (launch_conv_split sees no model)
};

struct FrontWeights {
    int kw1 = 5;               // kernel width of sig_conv1, sig_conv2, seq_conv1
    float *w_sig1 = nullptr;   // [kw1][4]
    float *b_sig1 = nullptr;   // [4]
    float *w_sig2 = nullptr;   // [kw1][4 ic][16 oc]
    float *b_sig2 = nullptr;   // [16]
    float *wt_seq1 = nullptr;  // [kw1][K][4 base][16 oc] == [kw1][EC][16] (dense seq_conv1)
    float *wt5_seq1 = nullptr; // [kw1][K][5][16]: gather table, row 4 = zeros (missing base)
    float *b_seq1 = nullptr;   // [16]
};

// bf16 A fragments of the fused front kernel (k_fused.hip): [oc/16][k-steps][64 lanes] x 16 B, k = tap * C + channel
// Activations travel scaled by log2(e) inside that kernel: sig_conv1 / seq_conv1 (raw inputs) have weights AND bias
// scaled, the other layers only the bias.
struct FusedWeights {
    float *a_sig2 = nullptr, *a_seq1 = nullptr, *a_sig3 = nullptr, *a_seq2 = nullptr, *a_merge1 = nullptr;
    float *w_sig1 = nullptr, *b_sig1 = nullptr, *b_sig2 = nullptr, *b_seq1 = nullptr, *b_sig3 = nullptr, *b_seq2 = nullptr,
          *b_merge1 = nullptr;
};

struct LstmWeights {
    float *a_ih1 = nullptr, *a_hh1 = nullptr;  // [H/16 waves][4 gates][H/4][64]
    float *b1 = nullptr;                       // [4H]  b_ih + b_hh
    float *a_ih2 = nullptr;                    // [H/16][3 gates i,g,o][H/4][64]
    float *b2 = nullptr;                       // [3H]  (i,g,o) b_ih + b_hh
    float *w_fc = nullptr, *b_fc = nullptr;    // [num_out][H], [num_out]
    // split-bf16 fragments (dtype != 0): [H/16][4 gates][H/32][nparts][64 lanes] x 16 B
    float *s_ih1 = nullptr, *s_hh1 = nullptr;
    // k_lstm_x16.hip (plain bf16, size 64): unit-major tiles [8 waves][2 tiles][2 k-steps][64 lanes] x 16 B, biases
    // [8][2][4 q][4 gates]; lstm2 with a zero f row
    float *x_ih = nullptr, *x_hh = nullptr, *x_ih2 = nullptr, *x_b1 = nullptr, *x_b2 = nullptr;
    float *xs_ih = nullptr, *xs_hh = nullptr, *xs_ih2 = nullptr;  // the same fragments as NP split parts (k_lstm_x16s.hip)
    // k_stream.hip (more than 64 hidden units, fp32): [H/16 waves][H/16 k groups][4 gates (lstm2: 3)][64 lanes][4]
    float *t_ih1 = nullptr, *t_hh1 = nullptr, *t_ih2 = nullptr;
    // lstm_small_kernel (k_lstm.hip; 64 hidden units, fp32, batches of a few hundred chunks): [4 waves][64 k in issue order][64 lanes],
    // lane l = gate l & 3 (lstm2: i, g, o, zero) of unit 16 w + (l >> 2)
    float *q_ih1 = nullptr, *q_hh1 = nullptr, *q_ih2 = nullptr;
    // k_stream16.hip (more than 64 hidden units, bf16 / f16): [H/16 waves][4 tiles][H/32 k-steps][64 lanes] x 16 B, row m of tile t of
    // wave w = (unit 16 w + 4 (m >> 2) + t, gate m & 3), pre-scaled; biases [H/16][4][4 q][4 gates]
    float *s16_ih = nullptr, *s16_hh = nullptr, *s16_ih2 = nullptr, *s16_b1 = nullptr, *s16_b2 = nullptr;
};

// What pack_model derives from a desc and its blob: the operand format, the chunk geometry and the (device) buffers
struct ModelWeights {
    rmr_model_desc desc{};  // desc.size: the channel count the kernels run at (padded_size)
    int nparts = 0;  // 0: fp32 MFMA path; 1..3: bf16 MFMA with 1 / 2 / 3-part split operands
    bool split_f16 = false;  // dtype f16x3: nparts == 2 and the parts are IEEE half (hi, lo)
    bool f16 = false;  // dtype 4: nparts == 1 with IEEE-half operands in the fused kernels (k_fused.hip, k_lstm_x16.hip)
    FrontWeights front;
    // conv_lstm: sig3, seq2, merge1;  conv_only: sig3, seq2, seq3, merge1..4
    ConvLayer sig3, seq2, seq3, merge1, merge2, merge3, merge4;
    LstmWeights lstm;
    FusedWeights fused;  // plain-bf16 ConvLSTM only
    float *w_fc = nullptr, *b_fc = nullptr;  // conv_only head: [num_out][size*3]
    // derived geometry
    int L = 0, P1 = 0, P2 = 0, P3 = 0, PQ2 = 0, T = 0, T2 = 0, T3 = 0, T4 = 0;
};

struct ConvSpec { int ic, oc, kw, stride; };

struct Folded {
    ConvSpec s;
    std::vector<float> w;  // [oc][ic][kw] folded
    std::vector<float> b;  // [oc]
};

constexpr int kMaxPaddedSize = 256;
std::vector<ConvSpec> conv_specs(const rmr_model_desc &d);
int padded_size(int size, int dtype = 0);
bool desc_ok(const rmr_model_desc &d);
size_t weight_count(const rmr_model_desc &d);  // floats of the blob of a desc_ok desc
std::vector<float> pad_model_blob(const rmr_model_desc &d, const float *w, int sp);
Folded fold(const ConvSpec &s, const float *&p);

// Winograd filter transform U = G W: r filter taps (phase p of a stride-P layer: tap 3 t + p), G in natural point order
// (0, 1, -1, 2, -2, [1/2, -1/2,] inf), the kernel's x order `order` of nx points; fp32 fragments
// [oc/16][((x * P + p) * (ic/16) + g) * 4 + j][64 lanes], lane (q, m): output channel 16 tile + m, input channel 16 g + 4 q + j
extern const double G5[8][5], G3[6][3];
extern const int F45_KERNEL_ORDER[8], F43_KERNEL_ORDER[6], NATURAL_ORDER[8];
std::vector<float> wino_filter(const Folded &f, const double *G, int r, const int *order, int nx, int P);

// `upload(name, host, &dev)`: one finished buffer; `name` is its field in ModelWeights ("sig3.apack", "lstm.x_b1", "w_fc")
using Upload = std::function<int(const std::string &name, const std::vector<float> &host, float **dev)>;
// Fold and pack the blob of `desc` (a size the kernels run at: padded_size is the identity on it) into `m`
int pack_model(const rmr_model_desc &desc, const float *weights, size_t n_floats, ModelWeights *m, const Upload &upload);

}  // namespace rmr
