// rmr_pack.h on the CPU (tests/test_host_cpu.py): pack_model - the function rmr_model_create runs - on seeded blobs of a set of
// model descriptions, with an `upload` that records an FNV-1a digest of every buffer instead of copying it to a device.
// Prints, per description, its geometry line and one line per buffer: "<desc> <buffer> <floats> <digest>".  Then the
// Winograd filter transforms on one-hot filters, in every point order a kernel uses: "wino <form> <phase> <x> <tap> <U>", U as the
// fp32 value pack_model uploads, plus the G tables in float64.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "rmr_pack.h"

namespace rmr {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace rmr

using namespace rmr;

static uint64_t fnv1a(const void *p, size_t n) {
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}

// the canonical blob of `d`: every value uniform in [-0.5, 0.5) from a 64-bit LCG, BatchNorm variances in [0.25, 1.25)
static std::vector<float> seeded_blob(const rmr_model_desc &d) {
    std::vector<float> w(weight_count(d));
    uint64_t s = 0x9e3779b97f4a7c15ull;
    for (float &x : w) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        x = (float)(s >> 40) * (1.0f / 16777216.0f) - 0.5f;
    }
    size_t at = 0;
    for (const ConvSpec &c : conv_specs(d)) {
        at += (size_t)c.oc * c.ic * c.kw + 4 * (size_t)c.oc;  // weight, bias, gamma, beta, mean
        for (int o = 0; o < c.oc; ++o) w[at + o] += 0.75f;
        at += c.oc;
    }
    return w;
}

static const char *kDtype[6] = {"fp32", "bf16", "bf16x3", "bf16x6", "f16", "f16x3"};

// as rmr_model_create: the blob padded to the kernels' channel count first
static int run(const rmr_model_desc &d) {
    char tag[64];
    snprintf(tag, sizeof tag, "%s_s%d_k%d_%s", d.arch == RMR_ARCH_CONV_LSTM ? "lstm" : "conv", d.size, d.kmer_len, kDtype[d.dtype]);
    std::vector<float> blob = seeded_blob(d);
    rmr_model_desc pd = d;
    pd.size = padded_size(d.size, d.dtype);
    if (pd.size != d.size) blob = pad_model_blob(d, blob.data(), pd.size);
    std::map<std::string, std::pair<size_t, uint64_t>> got;
    ModelWeights m;
    size_t nbuf = 0;
    const int rc = pack_model(pd, blob.data(), blob.size(), &m, [&](const std::string &name, const std::vector<float> &h, float **dev) {
        if (!got.emplace(name, std::make_pair(h.size(), fnv1a(h.data(), h.size() * sizeof(float)))).second) {
            printf("%s %s uploaded twice\n", tag, name.c_str());
            return -1;
        }
        *dev = reinterpret_cast<float *>(16 * ++nbuf);  // a distinct non-null address per buffer
        return 0;
    });
    if (rc) {
        printf("%s pack_model failed (%d)\n", tag, rc);
        return 1;
    }
    printf("%s geometry nparts=%d split_f16=%d f16=%d L=%d P1=%d P2=%d P3=%d PQ2=%d T=%d T2=%d T3=%d T4=%d kw1=%d\n", tag, m.nparts,
           m.split_f16, m.f16, m.L, m.P1, m.P2, m.P3, m.PQ2, m.T, m.T2, m.T3, m.T4, m.front.kw1);
    for (auto &kv : got) printf("%s %s %zu %016llx\n", tag, kv.first.c_str(), kv.second.first, (unsigned long long)kv.second.second);
    return 0;
}

// U = G W of a one-hot filter - weight 1 at (output 0, input 0, tap P t + p) - at every point x, in the kernel's order; every
// other entry of the packed buffer must be zero
static int wino_one_hot(const char *form, int ic, int kw, int P, const double *G, int r, const int *order, int nx) {
    int bad = 0;
    for (int p = 0; p < P; ++p)
        for (int t = 0; t < r && P * t + p < kw; ++t) {
            Folded f{{ic, 16, kw, P}, std::vector<float>((size_t)16 * ic * kw, 0.0f), std::vector<float>(16, 0.0f)};
            f.w[P * t + p] = 1.0f;
            std::vector<float> u = wino_filter(f, G, r, order, nx, P);
            for (int x = 0; x < nx; ++x) {
                const size_t at = (size_t)(x * P + p) * (ic / 16) * 256;  // tile 0, channel group 0, j 0, lane 0
                printf("wino %s %d %d %d %.9g\n", form, p, x, t, u[at]);
                u[at] = 0.0f;
            }
            for (float v : u) bad += v != 0.0f;
        }
    printf("wino %s misplaced %d\n", form, bad);
    return bad != 0;
}

int main() {
    int bad = 0;
    struct Net { int arch, size, K; };
    const Net nets[] = {{RMR_ARCH_CONV_LSTM, 16, 9},  {RMR_ARCH_CONV_LSTM, 32, 9},  {RMR_ARCH_CONV_LSTM, 64, 9},
                        {RMR_ARCH_CONV_LSTM, 96, 9},  {RMR_ARCH_CONV_LSTM, 128, 9}, {RMR_ARCH_CONV_LSTM, 256, 9},
                        {RMR_ARCH_CONV_LSTM, 64, 6},  {RMR_ARCH_CONV_LSTM, 64, 5},  {RMR_ARCH_CONV_LSTM, 128, 5},
                        {RMR_ARCH_CONV_LSTM, 40, 9},  {RMR_ARCH_CONV_ONLY, 64, 9},  {RMR_ARCH_CONV_ONLY, 96, 9}};
    for (const Net &n : nets)
        for (int dtype = 0; dtype < 6; ++dtype) {
            rmr_model_desc d{};
            d.arch = n.arch;
            d.size = n.size;
            d.kmer_len = n.K;
            d.num_out = 2;
            d.chunk_len = 100;
            d.dtype = dtype;
            if (desc_ok(d)) bad += run(d);
        }
    for (int x = 0; x < 8; ++x)
        for (int t = 0; t < 5; ++t) printf("G5 %d %d %.17g\n", x, t, G5[x][t]);
    for (int x = 0; x < 6; ++x)
        for (int t = 0; t < 3; ++t) printf("G3 %d %d %.17g\n", x, t, G3[x][t]);
    bad += wino_one_hot("f45_kernel", 64, 5, 1, G5[0], 5, F45_KERNEL_ORDER, 8);  // merge_conv1 / merge_conv2: wino_kernel
    bad += wino_one_hot("f45_natural_s3", 16, 13, 3, G5[0], 5, NATURAL_ORDER, 8);  // seq_conv2: seq2_front_wino_kernel
    bad += wino_one_hot("f43_natural_s3", 16, 9, 3, G3[0], 3, NATURAL_ORDER, 6);  // sig_conv3: sig3_front_wino_kernel
    bad += wino_one_hot("f43_kernel_s3", 32, 9, 3, G3[0], 3, F43_KERNEL_ORDER, 6);  // Conv_w_ref seq_conv3: wino_s3_kernel
    return bad != 0;
}
