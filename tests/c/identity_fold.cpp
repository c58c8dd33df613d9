// rmr::fold on the CPU with identity BatchNorm statistics (tests/test_host_model_export.py): a dorado-format model directory
// holds convolutions that are folded already, and rmr_model_create folds once more.  The loader hands it gamma = 1, beta = 0,
// mean = 0, var = float32(1 - 1e-5); the fold's scale is then 1 / sqrt(var + 1e-5) = 1 + 6.8e-9, under the 2^-25 relative half
// ulp of fp32, and every weight and bias has to come back with the bits it went in with.  Values: random mantissas over the
// binades 2^-40 .. 2^40 in both signs, +-0, the three neighbours of every power of two 2^-126 .. 2^127, the largest finite
// value, the smallest normal and denormals.  Prints "identity_fold <values> <mismatches>"; exit status 1 on any mismatch.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

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

static uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

static float from_bits(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}

int main() {
    std::vector<float> vals = {0.0f, -0.0f, 1.0f, -1.0f, 2.0f, -2.0f, 3.4028234663852886e38f, -3.4028234663852886e38f};
    for (int e = 1; e <= 254; ++e)  // 2^(e - 127) and the values one ulp either side of it, both signs
        for (int d = -1; d <= 1; ++d) {
            const uint32_t u = ((uint32_t)e << 23) + (uint32_t)d;
            vals.push_back(from_bits(u));
            vals.push_back(from_bits(u | 0x80000000u));
        }
    for (uint32_t u : {1u, 2u, 3u, 0x1234u, 0x400000u, 0x7fffffu, 0x800000u, 0x800001u}) {  // denormals, the smallest normals
        vals.push_back(from_bits(u));
        vals.push_back(from_bits(u | 0x80000000u));
    }
    uint64_t s = 0x2545f4914f6cdd1dull;
    for (int e = 127 - 40; e <= 127 + 40; ++e)
        for (int i = 0; i < 512; ++i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            vals.push_back(from_bits(((uint32_t)(s >> 63) << 31) | ((uint32_t)e << 23) | (uint32_t)((s >> 20) & 0x7fffffu)));
        }
    // one layer of 8 inputs, kernel width 5: the values fill the weights of `oc` outputs (the last padded with 1) and come
    // round again as the biases
    const int ic = 8, kw = 5, per = ic * kw;
    const int oc = (int)((vals.size() + per - 1) / per);
    std::vector<float> w((size_t)oc * per, 1.0f), b((size_t)oc);
    memcpy(w.data(), vals.data(), vals.size() * sizeof(float));
    for (int o = 0; o < oc; ++o) b[o] = vals[(size_t)o * 37 % vals.size()];
    b[1] = -0.0f;
    std::vector<float> blob(w);
    blob.insert(blob.end(), b.begin(), b.end());
    blob.insert(blob.end(), oc, 1.0f);                    // gamma
    blob.insert(blob.end(), oc, 0.0f);                    // beta
    blob.insert(blob.end(), oc, 0.0f);                    // running mean
    blob.insert(blob.end(), oc, (float)(1.0 - 1e-5));     // running variance: numpy's float32(1 - 1e-5)
    const float *p = blob.data();
    const rmr::Folded f = rmr::fold(rmr::ConvSpec{ic, oc, kw, 1}, p);
    long bad = 0;
    if (p != blob.data() + blob.size() || f.w.size() != w.size() || f.b.size() != b.size()) {
        printf("identity_fold consumed %td of %zu floats\n", p - blob.data(), blob.size());
        return 1;
    }
    for (size_t i = 0; i < w.size(); ++i)
        if (bits(f.w[i]) != bits(w[i])) {
            if (bad++ < 10) printf("weight %zu: %08x -> %08x\n", i, bits(w[i]), bits(f.w[i]));
        }
    for (size_t i = 0; i < b.size(); ++i)  // a bias of -0 comes back as +0 (beta = +0 is added to it): the same number
        if (bits(b[i]) == 0x80000000u ? bits(f.b[i]) << 1 != 0 : bits(f.b[i]) != bits(b[i])) {
            if (bad++ < 10) printf("bias %zu: %08x -> %08x\n", i, bits(b[i]), bits(f.b[i]));
        }
    printf("identity_fold %zu %ld\n", w.size() + b.size(), bad);
    return bad != 0;
}
