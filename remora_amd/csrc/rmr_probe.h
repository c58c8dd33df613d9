// rmr_probe.h — the probe batch of the Winograd guard (rmr_model_create, api_forward.hip): 256 chunks in the layout
// rmr_infer_chunks takes, at a model's own chunk length and k-mer context.  Plain C++ without HIP (tests/c/probe_batch.cpp
// digests it on the CPU).  Every value comes from one 64-bit integer generator written out below and from integer
// arithmetic, the signal through a single exact scaling by a power of two: the bytes are the same with every compiler and
// standard library.
//
// Chunks [0, PROBE_NOISE): unit-variance noise clipped at +-5 over random bases and random monotone mappings.  The rest
// cycle through eight structured cases that stress the transforms' large BT / AT entries: constant signal, +-3 alternating
// spikes, one isolated +-5 outlier on a silent chunk, a homopolymer, a dinucleotide repeat, the shortest (one base) and the
// longest (probe_max_len) sequence, and the largest clipped level held over the whole chunk.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace rmr {

constexpr int PROBE_CHUNKS = 256;
constexpr int PROBE_NOISE = 224;

// bases per chunk the probe is laid out for: five samples a base (the ratio of the project's C100 / C200 configurations),
// at least two, never more than the distinct cut points a chunk of L samples has
inline int probe_max_len(int L) {
    int m = L / 5;
    if (m < 2) m = 2;
    return m > L ? L : m;
}

struct ProbeBatch {
    int n = 0, L = 0, kb = 0, ka = 0, max_len = 0, seq_w = 0, map_w = 0;
    std::vector<float> signal;  // [n][L]
    std::vector<int8_t> seqs;   // [n][seq_w], -1 behind the chunk's len + kb + ka bases
    std::vector<int16_t> maps;  // [n][map_w]: 0, the cuts, L at index len, zeros behind it
    std::vector<int16_t> lens;  // [n]
};

// splitmix64 (Steele, Lea, Flood 2014): one add, two xor-shift-multiplies
struct ProbeRng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)((next() >> 33) % (uint64_t)n); }  // (the modulo bias of n << 2^31 is beside the point)
    // Irwin-Hall: twelve 16-bit uniforms, centred, scaled by 2^-16 - mean 0, variance 1, support +-6; the integer sum has
    // 21 bits, the scaling is exact
    float noise() {
        int64_t sum = 0;
        for (int k = 0; k < 3; ++k) {
            const uint64_t r = next();
            sum += (int64_t)(r & 0xFFFF) + (int64_t)((r >> 16) & 0xFFFF) + (int64_t)((r >> 32) & 0xFFFF) + (int64_t)(r >> 48);
        }
        const float v = (float)(2 * sum - 12 * 65535) * (1.0f / 131072.0f);
        return v > 5.0f ? 5.0f : (v < -5.0f ? -5.0f : v);
    }
};

inline ProbeBatch make_probe_batch(int L, int kb, int ka) {
    ProbeBatch b;
    b.n = PROBE_CHUNKS; b.L = L; b.kb = kb; b.ka = ka;
    b.max_len = probe_max_len(L);
    b.seq_w = b.max_len + kb + ka;
    b.map_w = b.max_len + 1;
    b.signal.assign((size_t)b.n * L, 0.0f);
    b.seqs.assign((size_t)b.n * b.seq_w, (int8_t)-1);
    b.maps.assign((size_t)b.n * b.map_w, (int16_t)0);
    b.lens.assign(b.n, (int16_t)0);
    ProbeRng rng{0x52454D4F52414D44ull};
    const int lo = std::max(2, (3 * b.max_len + 9) / 10);  // noise chunks: len ~ U[ceil(0.3 max), max]
    std::vector<int> cuts(L > 1 ? L - 1 : 0);
    for (int i = 0; i < b.n; ++i) {
        const int kind = i < PROBE_NOISE ? -1 : (i - PROBE_NOISE) % 8, variant = i < PROBE_NOISE ? 0 : (i - PROBE_NOISE) / 8;
        float *sig = &b.signal[(size_t)i * L];
        int8_t *seq = &b.seqs[(size_t)i * b.seq_w];
        int16_t *map = &b.maps[(size_t)i * b.map_w];
        // ---- sequence length and mapping: len - 1 distinct cuts out of 1 .. L - 1 (a partial shuffle), sorted ----
        int len = std::min(lo + rng.below(b.max_len - lo + 1), b.max_len);
        if (kind == 5) len = 1;
        if (kind == 6) len = b.max_len;
        for (int c = 0; c < (int)cuts.size(); ++c) cuts[c] = c + 1;
        for (int c = 0; c < len - 1; ++c) std::swap(cuts[c], cuts[c + rng.below((int)cuts.size() - c)]);
        std::sort(cuts.begin(), cuts.begin() + (len - 1));
        for (int c = 0; c < len - 1; ++c) map[c + 1] = (int16_t)cuts[c];
        map[len] = (int16_t)L;
        b.lens[i] = (int16_t)len;
        // ---- bases ----
        for (int p = 0; p < len + kb + ka; ++p) {
            int base = (int)(rng.next() >> 62);
            if (kind == 3) base = variant & 3;                                  // homopolymer
            if (kind == 4) base = (p & 1) ? (variant + 1 + (variant >> 1)) & 3 : variant & 3;  // dinucleotide repeat
            seq[p] = (int8_t)base;
        }
        // ---- signal ----
        const float sign = (variant & 1) ? -1.0f : 1.0f;
        for (int s = 0; s < L; ++s) sig[s] = rng.noise();  // (drawn for every chunk: the stream does not depend on the kind)
        if (kind == 0) for (int s = 0; s < L; ++s) sig[s] = sign * 0.5f * (float)(1 + (variant >> 1));  // constant: +-0.5, +-1
        if (kind == 1) for (int s = 0; s < L; ++s) sig[s] = ((s + variant) & 1) ? -3.0f : 3.0f;
        if (kind == 2) {
            for (int s = 0; s < L; ++s) sig[s] = 0.0f;
            sig[rng.below(L)] = sign * 5.0f;
        }
        if (kind == 7) for (int s = 0; s < L; ++s) sig[s] = sign * 5.0f;
    }
    return b;
}

// The probe batch as the one-hot tensor f32[n][4 K][L] that the dense entry takes (rmr_forward; the reference's
// compute_encoded_kmer_batch): at every sample s of base p's [map[p], map[p + 1]) a 1.0 in row 4 kp + seqs[p + kp] for each of
// the K = kb + ka + 1 slots kp; nothing for a base outside 0 .. 3 or a sample no base owns.
inline std::vector<float> probe_one_hot(const ProbeBatch &b) {
    const int K = b.kb + b.ka + 1;
    std::vector<float> enc((size_t)b.n * 4 * K * b.L, 0.0f);
    for (int i = 0; i < b.n; ++i) {
        const int8_t *seq = &b.seqs[(size_t)i * b.seq_w];
        const int16_t *map = &b.maps[(size_t)i * b.map_w];
        float *e = &enc[(size_t)i * 4 * K * b.L];
        for (int p = 0; p < b.lens[i]; ++p)
            for (int kp = 0; kp < K; ++kp) {
                const int base = seq[p + kp];
                if (base < 0 || base > 3) continue;
                for (int s = std::max<int>(map[p], 0); s < std::min<int>(map[p + 1], b.L); ++s) e[(size_t)(4 * kp + base) * b.L + s] = 1.0f;
            }
    }
    return enc;
}

// FNV-1a over the bytes of an array (the digest tests/c/probe_batch.cpp prints)
inline uint64_t fnv1a(const void *p, size_t bytes, uint64_t h = 0xCBF29CE484222325ull) {
    const unsigned char *c = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 0x100000001B3ull;
    return h;
}

}  // namespace rmr
