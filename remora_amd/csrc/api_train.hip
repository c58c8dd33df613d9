// api_train.hip - the training entry points of libremora_hip.so (rmr_trainer_*): one fp32 ConvLSTM_w_ref training step as
// launches of the kernels of k_train.hip.  Parameters and running statistics live in one device buffer in the order of
// rmr_model_create's blob; gradients and the two Adam moments are buffers of the same layout.  The workspace (every
// pre-BatchNorm convolution output, the LSTM's gates and states, the gradients on the way back, the partials of the
// fixed-order reductions) is allocated once, for max_batch chunks.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "rmr_internal.h"

using namespace rmr;

namespace {

struct Tensor {
    std::string name;
    size_t off, size;
    bool param;
};

// one convolution + BatchNorm + swish
struct Layer {
    int IC, OC, KW, st, Lin, Lout;
    size_t w, b, g, be, rm, rv;  // offsets in the flat buffers
    const float *in = nullptr;   // the input activations [n][Lin][IC] (sig_conv1: the signal)
    float *ypre = nullptr;       // [n][Lout][OC] before BatchNorm: kept for the backward pass
    float *out = nullptr;        // swish(bn(ypre)) in rows of aw floats from column coff
    int aw = 0, coff = 0;
    float *d_out = nullptr;      // the gradient with respect to `out`, same rows
    float *d_in = nullptr;       // the gradient with respect to `in` (nullptr: a first layer)
    float *Bf = nullptr, *Bd = nullptr;  // the weights as the forward / data-gradient products read them
    float *stat = nullptr;       // mean, rstd, mean(dU), mean(dU xhat): 4 OC floats
    int P() const { return st; }
    int J() const { return (KW + st - 1) / st; }
    int rows_in() const { return (Lin + st - 1) / st; }  // rows of the data-gradient product per chunk
    TrainSpan span_in() const { return TrainSpan{Lout, (long long)Lin * IC, st * IC, 0, (long long)Lin * IC}; }
};

TrainSpan plain(int width) { return TrainSpan{1, width, 0, 0, width}; }

}  // namespace

struct rmr_trainer {
    rmr_engine *eng = nullptr;
    int S = 0, KL = 0, EC = 0, NO = 0, L = 0, T = 0;
    int64_t max_batch = 0;
    size_t n_floats = 0;
    std::vector<Tensor> tensors;
    int n_params = 0;
    float *params = nullptr, *grads = nullptr, *m1 = nullptr, *m2 = nullptr;
    uint8_t *tensor_of = nullptr;
    long long *p_off = nullptr, *p_size = nullptr;  // the parameter tensors (device), named_parameters order
    float *clip = nullptr, *absmax = nullptr;
    float *ws = nullptr;
    size_t ws_floats = 0;
    int64_t step = 0, batches_tracked = 0;

    Layer sig1, sig2, sig3, seq1, seq2, merge;
    // lstm / fc offsets
    size_t l1_wih, l1_whh, l1_bih, l1_bhh, l2_wih, l2_whh, l2_bih, l2_bhh, fc_w, fc_b;
    // workspace
    float *in_sig, *in_seq, *seqT, *cat, *x, *G, *Cs, *H, *Z1, *G2, *C2, *H2, *Z2, *logits, *dlog, *loss_part, *loss, *dz1, *dc, *dx, *dcat, *da2,
        *da1, *daq1, *dY, *part_w, *part_c, *WihT1, *WhhT1, *WihT2, *bsum1, *bsum2;
    size_t part_w_floats = 0;
    int64_t *in_labels = nullptr;
    uint8_t *in_mask = nullptr;
    int *count = nullptr;
};

namespace {

__global__ void train_add2_kernel(const float *a, const float *b, int n, float *out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) out[e] = a[e] + b[e];
}

void add_conv(rmr_trainer *t, Layer &l, const char *conv, const char *bn, int IC, int OC, int KW, int st, int Lin, size_t &at) {
    l.IC = IC, l.OC = OC, l.KW = KW, l.st = st, l.Lin = Lin, l.Lout = (Lin - KW) / st + 1;
    auto push = [&](const std::string &name, size_t size, bool param) {
        t->tensors.push_back(Tensor{name, at, size, param});
        at += size;
        return at - size;
    };
    l.w = push(std::string(conv) + ".weight", (size_t)OC * IC * KW, true);
    l.b = push(std::string(conv) + ".bias", OC, true);
    l.g = push(std::string(bn) + ".weight", OC, true);
    l.be = push(std::string(bn) + ".bias", OC, true);
    l.rm = push(std::string(bn) + ".running_mean", OC, false);
    l.rv = push(std::string(bn) + ".running_var", OC, false);
}

int conv_forward(rmr_trainer *t, Layer &l, int64_t n) {
    rmr_engine *e = t->eng;
    const long long R = n * l.Lout;
    RMR_TRY(train_gemm(e, l.in, l.span_in(), l.Bf, l.OC, l.KW * l.IC, l.ypre, plain(l.OC), l.OC, R, t->params + l.b));
    return train_bn_forward(e, l.ypre, l.OC, R, l.stat, t->params + l.g, t->params + l.be, t->params + l.rm, t->params + l.rv, t->part_c,
                            t->count + 1, l.out, l.aw, l.coff);
}

int conv_backward(rmr_trainer *t, Layer &l, int64_t n) {
    rmr_engine *e = t->eng;
    const long long R = n * l.Lout;
    RMR_TRY(train_bn_backward(e, l.ypre, l.OC, R, l.stat, t->params + l.g, t->params + l.be, l.d_out, l.aw, l.coff, t->part_c, t->count + 1,
                              t->grads + l.g, t->grads + l.be, t->dY, t->grads + l.b));
    RMR_TRY(train_wgrad(e, l.in, l.span_in(), t->dY, plain(l.OC), l.KW * l.IC, l.OC, R, l.IC, l.KW, t->part_w, t->part_w_floats, t->count + 1,
                        t->grads + l.w));
    if (!l.d_in) return 0;
    // the data gradient: rows q of P * IC columns, dX[P q + p][ic] = sum_j sum_oc dY[q - j][oc] W[oc][ic][p + P j]
    const int rows = l.rows_in();
    const TrainSpan sa{rows, (long long)l.Lout * l.OC, l.OC, -(l.J() - 1) * l.OC, (long long)l.Lout * l.OC};
    const TrainSpan sc{rows, (long long)l.Lin * l.IC, l.P() * l.IC, 0, (long long)l.Lin * l.IC};
    return train_gemm(e, t->dY, sa, l.Bd, l.P() * l.IC, l.J() * l.OC, l.d_in, sc, l.P() * l.IC, n * rows, nullptr);
}

int forward_backward(rmr_trainer *t, const float *sig, const float *seq, const int64_t *labels, const uint8_t *mask, int64_t n, float *logits_dev) {
    rmr_engine *e = t->eng;
    const int S = t->S, T = t->T, NO = t->NO;
    float *P = t->params, *Gr = t->grads;
    // count[0]: the rows in the loss; count[1] (`refused`): the first of them whose label is out of range, or -1.  Every later store
    // to a gradient or a running statistic is held when it is set, and the caller refuses the call once it has read the record
    const int *refused = t->count + 1;
    RMR_TRY(train_count_rows(e, mask, labels, NO, n, t->count));
    // ---- the weights in product order ----
    for (Layer *l : {&t->sig2, &t->sig3, &t->seq1, &t->seq2, &t->merge}) RMR_TRY(train_repack(e, P + l->w, l->OC, l->IC, l->KW, 1, 1, 0, l->Bf));
    for (Layer *l : {&t->sig2, &t->sig3, &t->seq2, &t->merge}) RMR_TRY(train_repack(e, P + l->w, l->OC, l->IC, l->KW, l->P(), l->J(), 1, l->Bd));
    RMR_TRY(train_repack(e, P + t->l1_wih, 4 * S, S, 1, 1, 1, 0, t->WihT1));
    RMR_TRY(train_repack(e, P + t->l1_whh, 4 * S, S, 1, 1, 1, 0, t->WhhT1));
    RMR_TRY(train_repack(e, P + t->l2_wih, 4 * S, S, 1, 1, 1, 0, t->WihT2));
    {
        ProfScope ps(e, K_TRAIN_AUX);  // b_ih + b_hh of both LSTMs
        hipLaunchKernelGGL(train_add2_kernel, dim3((4 * S + 255) / 256), dim3(256), 0, e->stream, P + t->l1_bih, P + t->l1_bhh, 4 * S, t->bsum1);
        hipLaunchKernelGGL(train_add2_kernel, dim3((4 * S + 255) / 256), dim3(256), 0, e->stream, P + t->l2_bih, P + t->l2_bhh, 4 * S, t->bsum2);
        RMR_HIP(hipGetLastError());
    }

    // ---- forward ----
    {
        Layer &l = t->sig1;
        l.in = sig;
        RMR_TRY(train_sig1(e, sig, l.Lin, l.Lout, l.OC, l.KW, P + l.w, P + l.b, n, l.ypre));
        RMR_TRY(train_bn_forward(e, l.ypre, l.OC, n * l.Lout, l.stat, P + l.g, P + l.be, P + l.rm, P + l.rv, t->part_c, refused, l.out, l.aw, l.coff));
    }
    RMR_TRY(conv_forward(t, t->sig2, n));
    RMR_TRY(conv_forward(t, t->sig3, n));
    RMR_TRY(train_seq_transpose(e, seq, t->EC, t->L, n, t->seqT));
    RMR_TRY(conv_forward(t, t->seq1, n));
    RMR_TRY(conv_forward(t, t->seq2, n));
    RMR_TRY(conv_forward(t, t->merge, n));
    // lstm1: the input half of every step's gates in one product, then the T steps
    RMR_TRY(train_gemm(e, t->x, plain(S), t->WihT1, 4 * S, S, t->G, plain(4 * S), 4 * S, n * T, t->bsum1));
    for (int s = 0; s < T; ++s) RMR_TRY(train_lstm_step(e, t->G, t->Cs, t->H, t->Z1, t->WhhT1, S, T, s, n));
    // lstm2: one step from a zero state on lstm1's last output (z[-1] after the second flip is lstm2's FIRST step)
    const TrainSpan last{1, (long long)T * S, 0, (T - 1) * S, (long long)T * S};
    RMR_TRY(train_gemm(e, t->Z1, last, t->WihT2, 4 * S, S, t->G2, plain(4 * S), 4 * S, n, t->bsum2));
    RMR_TRY(train_lstm2(e, t->G2, t->C2, t->H2, t->Z2, S, n));
    RMR_TRY(train_fc_loss(e, t->Z2, P + t->fc_w, P + t->fc_b, S, NO, labels, mask, t->count, n, t->logits, t->dlog, t->loss_part, logits_dev, t->loss));

    // ---- backward ----
    RMR_TRY(train_wgrad(e, t->Z2, plain(S), t->dlog, plain(NO), S, NO, n, S, 1, t->part_w, t->part_w_floats, refused, Gr + t->fc_w));
    RMR_TRY(train_bias_grad(e, t->dlog, NO, n, t->part_c, refused, Gr + t->fc_b, nullptr));
    RMR_TRY(train_lstm2_bwd(e, t->G2, t->C2, t->H2, t->dlog, P + t->fc_w, NO, S, n));
    RMR_TRY(train_wgrad(e, t->Z1, last, t->G2, plain(4 * S), S, 4 * S, n, S, 1, t->part_w, t->part_w_floats, refused, Gr + t->l2_wih));
    RMR_TRY(train_fill(e, Gr + t->l2_whh, (long long)4 * S * S, 0.f, refused));  // h_0 = 0: exactly zero
    RMR_TRY(train_bias_grad(e, t->G2, 4 * S, n, t->part_c, refused, Gr + t->l2_bih, Gr + t->l2_bhh));
    RMR_TRY(train_gemm(e, t->G2, plain(4 * S), P + t->l2_wih, S, 4 * S, t->dz1, plain(S), S, n, nullptr));
    // lstm1: the gradient enters at step T - 1 only; dh_{t-1} = dgates_t W_hh is the sequential part
    for (int s = T - 1; s >= 0; --s) RMR_TRY(train_lstm_step_bwd(e, t->G, t->Cs, t->H, P + t->l1_whh, t->dz1, t->dc, S, T, s, n));
    RMR_TRY(train_gemm(e, t->G, plain(4 * S), P + t->l1_wih, S, 4 * S, t->dx, plain(S), S, n * T, nullptr));
    RMR_TRY(train_wgrad(e, t->x, plain(S), t->G, plain(4 * S), S, 4 * S, n * T, S, 1, t->part_w, t->part_w_floats, refused, Gr + t->l1_wih));
    {
        const TrainSpan sa{T - 1, (long long)T * S, S, 0, (long long)T * S};
        const TrainSpan sd{T - 1, (long long)T * 4 * S, 4 * S, 4 * S, (long long)T * 4 * S};
        RMR_TRY(train_wgrad(e, t->H, sa, t->G, sd, S, 4 * S, n * (T - 1), S, 1, t->part_w, t->part_w_floats, refused, Gr + t->l1_whh));
    }
    RMR_TRY(train_bias_grad(e, t->G, 4 * S, n * T, t->part_c, refused, Gr + t->l1_bih, Gr + t->l1_bhh));
    RMR_TRY(conv_backward(t, t->merge, n));
    RMR_TRY(conv_backward(t, t->sig3, n));
    RMR_TRY(conv_backward(t, t->sig2, n));
    RMR_TRY(conv_backward(t, t->sig1, n));
    RMR_TRY(conv_backward(t, t->seq2, n));
    return conv_backward(t, t->seq1, n);
}

float *which_buffer(rmr_trainer *t, int which) {
    switch (which) {
        case RMR_TRAIN_PARAMS: return t->params;
        case RMR_TRAIN_GRADS: return t->grads;
        case RMR_TRAIN_ADAM_M: return t->m1;
        case RMR_TRAIN_ADAM_V: return t->m2;
    }
    return nullptr;
}

}  // namespace

extern "C" {

void rmr_trainer_destroy(rmr_trainer *t) {
    if (!t) return;
    (void)hipSetDevice(t->eng->device);
    (void)hipStreamSynchronize(t->eng->stream);
    for (void *p : {(void *)t->params, (void *)t->grads, (void *)t->m1, (void *)t->m2, (void *)t->tensor_of, (void *)t->p_off, (void *)t->p_size,
                    (void *)t->clip, (void *)t->absmax, (void *)t->ws})
        if (p) (void)hipFree(p);
    delete t;
}

int rmr_trainer_create(rmr_engine *e, const rmr_model_desc *desc, const float *blob, size_t n_floats, int64_t max_batch, rmr_trainer **out) {
    if (!e || !desc || !blob || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (desc->arch != RMR_ARCH_CONV_LSTM) RMR_FAIL(RMR_ERR_INVALID, "training is built for ConvLSTM_w_ref only: a Conv_w_ref model is refused");
    if (desc->dtype != 0) RMR_FAIL(RMR_ERR_INVALID, "training is fp32 only: the 16-bit and split dtypes (dtype %d) are refused", desc->dtype);
    if (desc->size < 16 || desc->size > 256 || desc->size % 16)
        RMR_FAIL(RMR_ERR_INVALID,
                 "training needs a size that is a multiple of 16 from 16 to 256, got %d (zero-weight channel padding is no identity under "
                 "train-mode BatchNorm)", desc->size);
    if (desc->kmer_len < 1 || desc->kmer_len > 21) RMR_FAIL(RMR_ERR_INVALID, "training needs a k-mer length of 1..21, got %d", desc->kmer_len);
    if (desc->chunk_len < 29) RMR_FAIL(RMR_ERR_INVALID, "training needs a chunk length of at least 29, got %d", desc->chunk_len);
    if (desc->chunk_len > (1 << 20)) RMR_FAIL(RMR_ERR_INVALID, "training needs a chunk length of at most 1048576, got %d", desc->chunk_len);
    if (desc->num_out < 2 || desc->num_out > 16) RMR_FAIL(RMR_ERR_INVALID, "training needs num_out of 2..16, got %d", desc->num_out);
    if (max_batch < 2 || max_batch > (1 << 20)) RMR_FAIL(RMR_ERR_INVALID, "max_batch must be 2..1048576, got %lld", (long long)max_batch);
    if (n_floats != rmr_model_weight_count(desc))
        RMR_FAIL(RMR_ERR_INVALID, "state blob has %zu floats, the network has %zu", n_floats, rmr_model_weight_count(desc));

    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::unique_ptr<rmr_trainer, void (*)(rmr_trainer *)> t(new rmr_trainer(), rmr_trainer_destroy);
    t->eng = e;
    const int S = t->S = desc->size, L = t->L = desc->chunk_len, NO = t->NO = desc->num_out;
    t->KL = desc->kmer_len;
    const int EC = t->EC = 4 * desc->kmer_len;
    t->max_batch = max_batch;
    t->n_floats = n_floats;
    size_t at = 0;
    add_conv(t.get(), t->sig1, "sig_conv1", "sig_bn1", 1, 4, 5, 1, L, at);
    add_conv(t.get(), t->sig2, "sig_conv2", "sig_bn2", 4, 16, 5, 1, t->sig1.Lout, at);
    add_conv(t.get(), t->sig3, "sig_conv3", "sig_bn3", 16, S, 9, 3, t->sig2.Lout, at);
    add_conv(t.get(), t->seq1, "seq_conv1", "seq_bn1", EC, 16, 5, 1, L, at);
    add_conv(t.get(), t->seq2, "seq_conv2", "seq_bn2", 16, S, 13, 3, t->seq1.Lout, at);
    add_conv(t.get(), t->merge, "merge_conv1", "merge_bn", 2 * S, S, 5, 1, t->sig3.Lout, at);
    if (t->seq2.Lout != t->sig3.Lout || t->merge.Lout < 1) RMR_FAIL(RMR_ERR_INVALID, "unexpected layer geometry at chunk length %d", L);
    const int T = t->T = t->merge.Lout;
    auto push = [&](const char *name, size_t size) {
        t->tensors.push_back(Tensor{name, at, size, true});
        at += size;
        return at - size;
    };
    t->l1_wih = push("lstm1.weight_ih_l0", (size_t)4 * S * S), t->l1_whh = push("lstm1.weight_hh_l0", (size_t)4 * S * S);
    t->l1_bih = push("lstm1.bias_ih_l0", 4 * S), t->l1_bhh = push("lstm1.bias_hh_l0", 4 * S);
    t->l2_wih = push("lstm2.weight_ih_l0", (size_t)4 * S * S), t->l2_whh = push("lstm2.weight_hh_l0", (size_t)4 * S * S);
    t->l2_bih = push("lstm2.bias_ih_l0", 4 * S), t->l2_bhh = push("lstm2.bias_hh_l0", 4 * S);
    t->fc_w = push("fc.weight", (size_t)NO * S), t->fc_b = push("fc.bias", NO);
    if (at != n_floats) RMR_FAIL(RMR_ERR_INVALID, "internal: tensor table covers %zu of %zu floats", at, n_floats);

    // ---- parameter-side buffers ----
    const size_t bytes = n_floats * sizeof(float);
    RMR_HIP(hipMalloc(&t->params, bytes));
    RMR_HIP(hipMalloc(&t->grads, bytes));
    RMR_HIP(hipMalloc(&t->m1, bytes));
    RMR_HIP(hipMalloc(&t->m2, bytes));
    RMR_HIP(hipMalloc(&t->tensor_of, n_floats));
    RMR_HIP(hipMemcpy(t->params, blob, bytes, hipMemcpyHostToDevice));
    RMR_HIP(hipMemset(t->grads, 0, bytes));
    RMR_HIP(hipMemset(t->m1, 0, bytes));
    RMR_HIP(hipMemset(t->m2, 0, bytes));
    std::vector<uint8_t> tof(n_floats, 255);
    std::vector<long long> poff, psize;
    for (const Tensor &x : t->tensors) {
        if (!x.param) continue;
        std::memset(tof.data() + x.off, (int)poff.size(), x.size);
        poff.push_back((long long)x.off), psize.push_back((long long)x.size);
    }
    t->n_params = (int)poff.size();
    RMR_HIP(hipMemcpy(t->tensor_of, tof.data(), n_floats, hipMemcpyHostToDevice));
    RMR_HIP(hipMalloc(&t->p_off, poff.size() * sizeof(long long)));
    RMR_HIP(hipMalloc(&t->p_size, poff.size() * sizeof(long long)));
    RMR_HIP(hipMemcpy(t->p_off, poff.data(), poff.size() * sizeof(long long), hipMemcpyHostToDevice));
    RMR_HIP(hipMemcpy(t->p_size, psize.data(), poff.size() * sizeof(long long), hipMemcpyHostToDevice));
    RMR_HIP(hipMalloc(&t->clip, poff.size() * sizeof(float)));
    RMR_HIP(hipMalloc(&t->absmax, poff.size() * sizeof(float)));

    // ---- workspace: sized in a first pass, carved in a second ----
    const size_t N = (size_t)max_batch;
    Layer *layers[6] = {&t->sig1, &t->sig2, &t->sig3, &t->seq1, &t->seq2, &t->merge};
    size_t dY_floats = 0, part_w = 0;
    long long max_rows = 0;
    auto part_for = [&](size_t K, size_t NC, size_t R) {
        size_t slices = (R + 255) / 256;
        if (slices > 64) slices = 64;
        if (slices < 1) slices = 1;
        part_w = std::max(part_w, K * NC * slices);
    };
    for (Layer *l : layers) {
        dY_floats = std::max(dY_floats, N * l->Lout * l->OC);
        part_for((size_t)l->KW * l->IC, l->OC, N * l->Lout);
        max_rows = std::max(max_rows, (long long)(N * l->Lout));
    }
    part_for(S, 4 * S, N * T);
    part_for(S, NO, N);
    t->part_w_floats = part_w;
    const size_t part_c = (size_t)train_colsum_blocks(max_rows) * 2 * (size_t)(4 * S);
    for (int pass = 0; pass < 2; ++pass) {
        size_t off = 0;
        auto take = [&](size_t floats) {
            float *p = t->ws ? t->ws + off : nullptr;
            off += (floats + 63) / 64 * 64;
            return p;
        };
        t->in_sig = take(N * L), t->in_seq = take(N * EC * L), t->seqT = take(N * L * EC);
        t->in_labels = reinterpret_cast<int64_t *>(take(N * 2));
        t->in_mask = reinterpret_cast<uint8_t *>(take((N + 3) / 4));
        t->count = reinterpret_cast<int *>(take(2));  // rows in the loss; the first row with a label out of range or -1
        for (Layer *l : layers) {
            l->ypre = take(N * l->Lout * l->OC);
            l->stat = take(4 * (size_t)l->OC);
            l->Bf = take((size_t)l->KW * l->IC * l->OC);
            l->Bd = take((size_t)l->J() * l->OC * l->P() * l->IC);
        }
        float *a1 = take(N * t->sig1.Lout * 4), *a2 = take(N * t->sig2.Lout * 16), *aq1 = take(N * t->seq1.Lout * 16);
        t->cat = take(N * t->sig3.Lout * 2 * S);
        t->x = take(N * T * S);
        t->dx = take(N * T * S), t->dcat = take(N * t->sig3.Lout * 2 * S), t->da2 = take(N * t->sig2.Lout * 16);
        t->da1 = take(N * t->sig1.Lout * 4), t->daq1 = take(N * t->seq1.Lout * 16);
        t->G = take(N * T * 4 * S), t->Cs = take(N * T * S), t->H = take(N * T * S), t->Z1 = take(N * T * S);
        t->G2 = take(N * 4 * S), t->C2 = take(N * S), t->H2 = take(N * S), t->Z2 = take(N * S);
        t->logits = take(N * NO), t->dlog = take(N * NO), t->loss_part = take(N), t->loss = take(2);  // the loss; count[1]'s bits
        t->dz1 = take(N * S), t->dc = take(N * S);
        t->dY = take(dY_floats), t->part_w = take(part_w), t->part_c = take(part_c);
        t->WihT1 = take((size_t)4 * S * S), t->WhhT1 = take((size_t)4 * S * S), t->WihT2 = take((size_t)4 * S * S);
        t->bsum1 = take(4 * S), t->bsum2 = take(4 * S);
        t->sig1.out = a1, t->sig1.aw = 4, t->sig1.d_out = t->da1, t->sig1.d_in = nullptr;
        t->sig2.in = a1, t->sig2.out = a2, t->sig2.aw = 16, t->sig2.d_out = t->da2, t->sig2.d_in = t->da1;
        t->sig3.in = a2, t->sig3.out = t->cat, t->sig3.aw = 2 * S, t->sig3.coff = 0, t->sig3.d_out = t->dcat, t->sig3.d_in = t->da2;
        t->seq1.in = t->seqT, t->seq1.out = aq1, t->seq1.aw = 16, t->seq1.d_out = t->daq1, t->seq1.d_in = nullptr;
        t->seq2.in = aq1, t->seq2.out = t->cat, t->seq2.aw = 2 * S, t->seq2.coff = S, t->seq2.d_out = t->dcat, t->seq2.d_in = t->daq1;
        t->merge.in = t->cat, t->merge.out = t->x, t->merge.aw = S, t->merge.d_out = t->dx, t->merge.d_in = t->dcat;
        if (pass == 0) {
            t->ws_floats = off;
            hipError_t err = hipMalloc(&t->ws, off * sizeof(float));
            if (err != hipSuccess) {
                t->ws = nullptr;
                set_error("hipMalloc(%zu) for the training workspace of %lld chunks failed: %s", off * sizeof(float), (long long)max_batch,
                          hipGetErrorString(err));
                return RMR_ERR_NOMEM;
            }
        }
    }
    *out = t.release();
    return 0;
}

int rmr_trainer_forward_backward(rmr_trainer *t, const float *sigs, const float *seqs, const int64_t *labels, const uint8_t *mask, int64_t n,
                                 float *loss, float *logits, int mem) {
    if (!t || !sigs || !seqs || !labels || !loss) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n > t->max_batch) RMR_FAIL(RMR_ERR_INVALID, "batch of %lld chunks exceeds the trainer's max_batch %lld", (long long)n, (long long)t->max_batch);
    if (n < 2) RMR_FAIL(RMR_ERR_INVALID, "train-mode BatchNorm needs a batch of at least 2 chunks, got %lld", (long long)n);
    rmr_engine *e = t->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    float *logits_dev = nullptr;
    const int64_t *labels_in = labels;
    if (mem == RMR_MEM_HOST) {
        // host labels are checked before anything is staged; device labels by the step's first kernel (below)
        for (int64_t i = 0; i < n; ++i)
            if ((!mask || mask[i]) && (labels[i] < 0 || labels[i] >= t->NO))
                RMR_FAIL(RMR_ERR_INVALID, "label %lld of chunk %lld is outside 0..num_out-1 (num_out %d)", (long long)labels[i], (long long)i, t->NO);
        RMR_HIP(hipMemcpyAsync(t->in_sig, sigs, (size_t)n * t->L * sizeof(float), hipMemcpyHostToDevice, e->stream));
        RMR_HIP(hipMemcpyAsync(t->in_seq, seqs, (size_t)n * t->EC * t->L * sizeof(float), hipMemcpyHostToDevice, e->stream));
        RMR_HIP(hipMemcpyAsync(t->in_labels, labels, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
        if (mask) RMR_HIP(hipMemcpyAsync(t->in_mask, mask, (size_t)n, hipMemcpyHostToDevice, e->stream));
        sigs = t->in_sig, seqs = t->in_seq, labels = t->in_labels;
        if (mask) mask = t->in_mask;
    } else {
        logits_dev = logits;
    }
    RMR_TRY(forward_backward(t, sigs, seqs, labels, mask, n, logits_dev));
    float got[2] = {0.f, 0.f};  // the loss and, as bits, the first chunk in the loss with a label out of range or -1
    RMR_HIP(hipMemcpyAsync(got, t->loss, sizeof(got), hipMemcpyDeviceToHost, e->stream));
    if (mem == RMR_MEM_HOST && logits)
        RMR_HIP(hipMemcpyAsync(logits, t->logits, (size_t)n * t->NO * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    RMR_HIP(hipStreamSynchronize(e->stream));
    int32_t row;
    std::memcpy(&row, &got[1], sizeof(row));
    if (row >= 0) {  // device labels: the kernels held every store to a gradient or a running statistic
        int64_t lab = 0;
        RMR_HIP(hipMemcpy(&lab, labels_in + row, sizeof(lab), hipMemcpyDeviceToHost));
        RMR_FAIL(RMR_ERR_INVALID, "label %lld of chunk %d is outside 0..num_out-1 (num_out %d)", (long long)lab, (int)row, t->NO);
    }
    *loss = got[0];
    t->batches_tracked += 1;
    return 0;
}

int rmr_trainer_grad_absmax(rmr_trainer *t, float *out) {
    if (!t || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    rmr_engine *e = t->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    RMR_TRY(train_absmax(e, t->grads, t->p_off, t->p_size, t->n_params, t->absmax));
    RMR_HIP(hipMemcpyAsync(out, t->absmax, t->n_params * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_trainer_adamw_step(rmr_trainer *t, double lr, double beta1, double beta2, double eps, double weight_decay, const float *clip) {
    if (!t) RMR_FAIL(RMR_ERR_INVALID, "trainer is NULL");
    rmr_engine *e = t->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (clip) RMR_HIP(hipMemcpyAsync(t->clip, clip, t->n_params * sizeof(float), hipMemcpyHostToDevice, e->stream));
    t->step += 1;
    const double bc1 = 1.0 - std::pow(beta1, (double)t->step);
    const double bc2_sqrt = std::sqrt(1.0 - std::pow(beta2, (double)t->step));
    RMR_TRY(train_adamw(e, t->params, t->grads, t->m1, t->m2, t->tensor_of, (long long)t->n_floats, (float)(lr * weight_decay), (float)(1.0 - beta1),
                        (float)beta2, (float)(1.0 - beta2), (float)eps, (float)(lr / bc1), (float)bc2_sqrt, clip ? t->clip : nullptr));
    if (clip) RMR_HIP(hipStreamSynchronize(e->stream));  // the caller's vector is free on return
    return 0;
}

int rmr_trainer_read(rmr_trainer *t, int which, float *out, size_t n_floats) {
    if (!t || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    rmr_engine *e = t->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    if (which == RMR_TRAIN_COUNTERS) {
        if (n_floats != 3) RMR_FAIL(RMR_ERR_INVALID, "the counters are 3 floats");
        out[0] = (float)t->step, out[1] = (float)t->batches_tracked;
        out[2] = (float)((double)t->ws_floats * sizeof(float) / (double)t->max_batch);
        return 0;
    }
    const float *src = which_buffer(t, which);
    if (!src) RMR_FAIL(RMR_ERR_INVALID, "unknown buffer %d", which);
    if (n_floats != t->n_floats) RMR_FAIL(RMR_ERR_INVALID, "the buffer has %zu floats, not %zu", t->n_floats, n_floats);
    RMR_HIP(hipSetDevice(e->device));
    RMR_HIP(hipMemcpyAsync(out, src, n_floats * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_trainer_write(rmr_trainer *t, int which, const float *in, size_t n_floats) {
    if (!t || !in) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    rmr_engine *e = t->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    if (which == RMR_TRAIN_COUNTERS) {
        if (n_floats != 3) RMR_FAIL(RMR_ERR_INVALID, "the counters are 3 floats");
        t->step = (int64_t)in[0], t->batches_tracked = (int64_t)in[1];
        return 0;
    }
    float *dst = which_buffer(t, which);
    if (!dst) RMR_FAIL(RMR_ERR_INVALID, "unknown buffer %d", which);
    if (n_floats != t->n_floats) RMR_FAIL(RMR_ERR_INVALID, "the buffer has %zu floats, not %zu", t->n_floats, n_floats);
    RMR_HIP(hipSetDevice(e->device));
    RMR_HIP(hipMemcpyAsync(dst, in, n_floats * sizeof(float), hipMemcpyHostToDevice, e->stream));
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_trainer_tensor_layout(const rmr_trainer *t, int cap, char *names, int64_t *offsets, int64_t *sizes, int32_t *is_param, int *n_out) {
    if (!t || !n_out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    *n_out = (int)t->tensors.size();
    if (!names && !offsets && !sizes && !is_param) return 0;
    if (cap < *n_out) RMR_FAIL(RMR_ERR_INVALID, "room for %d tensors, the trainer has %d", cap, *n_out);
    for (int i = 0; i < *n_out; ++i) {
        const Tensor &x = t->tensors[i];
        if (names) snprintf(names + (size_t)i * RMR_TRAIN_NAME_LEN, RMR_TRAIN_NAME_LEN, "%s", x.name.c_str());
        if (offsets) offsets[i] = (int64_t)x.off;
        if (sizes) sizes[i] = (int64_t)x.size;
        if (is_param) is_param[i] = x.param ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
