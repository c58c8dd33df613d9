// rmr_probe.h on the CPU (tests/test_host_winograd_guard.py): the probe batch of the Winograd guard at the (L, k-mer length)
// given on the command line - every mapping row starts at 0, is non-decreasing and ends at L at index len, every length lies
// within [1, probe_max_len(L)], every base is 0..3 in front of len + kb + ka and the padding value -1 behind it, the signal
// stays within +-5 and the noise chunks have about unit variance; the one-hot tensor of the same batch (the probe of a k-mer
// length the chunk-array entry refuses) is the arrays' encoding.  Prints the FNV-1a digest of the four arrays.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "rmr_probe.h"

using namespace rmr;

static int bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const int L = atoi(argv[1]), K = atoi(argv[2]), kb = (K - 1) / 2, ka = K - 1 - kb;
    const ProbeBatch b = make_probe_batch(L, kb, ka);
    CHECK(b.n == PROBE_CHUNKS && b.n == 256 && b.L == L && b.max_len == probe_max_len(L));
    CHECK(b.seq_w == b.max_len + K - 1 && b.map_w == b.max_len + 1);
    CHECK(b.signal.size() == (size_t)b.n * L && b.seqs.size() == (size_t)b.n * b.seq_w);
    CHECK(b.maps.size() == (size_t)b.n * b.map_w && b.lens.size() == (size_t)b.n);
    int shortest = b.max_len, longest = 0;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < b.n; ++i) {
        const int len = b.lens[i];
        const int16_t *map = &b.maps[(size_t)i * b.map_w];
        const int8_t *seq = &b.seqs[(size_t)i * b.seq_w];
        const float *sig = &b.signal[(size_t)i * L];
        CHECK(len >= 1 && len <= b.max_len);
        if (len < 1 || len > b.max_len) continue;
        shortest = len < shortest ? len : shortest;
        longest = len > longest ? len : longest;
        CHECK(map[0] == 0 && map[len] == L);
        for (int p = 0; p < len; ++p) CHECK(map[p + 1] >= map[p]);
        for (int p = len + 1; p < b.map_w; ++p) CHECK(map[p] == 0);
        for (int p = 0; p < b.seq_w; ++p) CHECK(p < len + K - 1 ? (seq[p] >= 0 && seq[p] <= 3) : seq[p] == -1);
        for (int s = 0; s < L; ++s) {
            CHECK(sig[s] >= -5.0f && sig[s] <= 5.0f);
            if (i < PROBE_NOISE) { s1 += sig[s]; s2 += (double)sig[s] * sig[s]; }
        }
    }
    CHECK(shortest == 1 && longest == b.max_len);  // the two extremes of the geometry are among the structured chunks
    const double cnt = (double)PROBE_NOISE * L, mean = s1 / cnt, var = s2 / cnt - mean * mean;
    CHECK(std::fabs(mean) < 0.05 && std::fabs(var - 1.0) < 0.05);
    // the same batch as the one-hot tensor of the dense entry (probe_one_hot, filled base by base): read sample by sample, the
    // base p that owns sample s puts exactly one 1.0 into the four rows of every slot kp, in row seq[p + kp]
    const std::vector<float> enc = probe_one_hot(b);
    CHECK(enc.size() == (size_t)b.n * 4 * K * L);
    for (int i = 0; i < b.n && enc.size() == (size_t)b.n * 4 * K * L; ++i) {
        const int16_t *map = &b.maps[(size_t)i * b.map_w];
        const int8_t *seq = &b.seqs[(size_t)i * b.seq_w];
        const float *e = &enc[(size_t)i * 4 * K * L];
        long wrong = 0;
        for (int s = 0, p = 0; s < L; ++s) {
            while (p < b.lens[i] && map[p + 1] <= s) ++p;
            for (int kp = 0; kp < K; ++kp)
                for (int base = 0; base < 4; ++base) wrong += e[(size_t)(4 * kp + base) * L + s] != (p < b.lens[i] && seq[p + kp] == base ? 1.0f : 0.0f);
        }
        CHECK(wrong == 0);
    }
    uint64_t h = fnv1a(b.signal.data(), b.signal.size() * sizeof(float));
    h = fnv1a(b.seqs.data(), b.seqs.size(), h);
    h = fnv1a(b.maps.data(), b.maps.size() * sizeof(int16_t), h);
    h = fnv1a(b.lens.data(), b.lens.size() * sizeof(int16_t), h);
    printf("digest %016llx\n%d failed checks\n", (unsigned long long)h, bad);
    return bad != 0;
}
