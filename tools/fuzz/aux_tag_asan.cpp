// AddressSanitizer + UBSan harness for the aux tag reader of `analyze pileup_modbams --partition-tag` (aux_value and
// rmr_bam_aux_values, remora_amd/csrc/mod_tags.cpp): aux regions built from the grammar with fields of every type - A c C s S i I f
// Z H, and B of every subtype - then every truncation of them and random mutations, each in a buffer of its exact size, so
// that a read at or behind the region's end is ASan's; kind and value are compared with a restatement that goes through the
// bytes by index.  The batch entry is run on the same regions behind leads of random length, on one to three threads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../remora_amd/csrc/mod_tags.cpp"

namespace rmr {
void set_error(const char *, ...) {}
}  // namespace rmr

static size_t width_of(char t) {
    switch (t) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
    }
}

// the restatement: indices into the bytes, every bound asked before a byte is looked at
static int restate(const std::string &s, const char *tag, int64_t *value) {
    int kind = RMR_AUX_ABSENT;
    int64_t found = 0;
    *value = 0;
    size_t i = 0;
    while (s.size() - i >= 3) {
        const char t = s[i + 2];
        const size_t v = i + 3, left = s.size() - v;
        size_t sz = 0;
        if (t == 'Z' || t == 'H') {
            size_t k = v;
            while (k < s.size() && s[k] != 0) ++k;
            if (k == s.size()) return RMR_AUX_UNWALKABLE;
            sz = k - v + 1;
        } else if (t == 'B') {
            if (left < 5) return RMR_AUX_UNWALKABLE;
            const size_t w = s[v] == 'A' ? 0 : width_of(s[v]);
            uint32_t cnt = 0;
            for (int b = 3; b >= 0; --b) cnt = (cnt << 8) | (uint8_t)s[v + 1 + (size_t)b];
            if (w == 0 || cnt > 0x7fffffffu) return RMR_AUX_UNWALKABLE;
            const uint64_t need = 5 + (uint64_t)cnt * w;
            if (need > left) return RMR_AUX_UNWALKABLE;
            sz = (size_t)need;
        } else {
            sz = width_of(t);
            if (sz == 0 || sz > left) return RMR_AUX_UNWALKABLE;
        }
        if (kind == RMR_AUX_ABSENT && s[i] == tag[0] && s[i + 1] == tag[1]) {
            uint64_t u = 0;
            const size_t w = width_of(t);
            for (size_t b = w; b-- > 0;) u = (u << 8) | (uint8_t)s[v + b];
            if (t == 'c' || t == 's' || t == 'i') {
                const uint64_t sign = 1ull << (8 * w - 1);
                found = (u & sign) ? (int64_t)u - (int64_t)(sign << 1) : (int64_t)u;
                kind = RMR_AUX_INT;
            } else if (t == 'C' || t == 'S' || t == 'I') {
                found = (int64_t)u, kind = RMR_AUX_INT;
            } else if (t == 'A') {
                found = (int64_t)u, kind = RMR_AUX_CHAR;
            } else {
                found = (uint8_t)t, kind = RMR_AUX_OTHER_TYPE;
            }
        }
        i = v + sz;
    }
    if (i != s.size()) return RMR_AUX_UNWALKABLE;
    *value = found;
    return kind;
}

static std::string field(std::mt19937_64 &rng, const char *name, char t) {
    std::string out(name, 2);
    out += t;
    auto bytes = [&](size_t n) {
        for (size_t k = 0; k < n; ++k) out += (char)(rng() % 4 == 0 ? (rng() % 2 ? 0xff : 0x80) : rng() & 255);
    };
    if (t == 'Z' || t == 'H') {
        const int n = (int)(rng() % 9);
        for (int k = 0; k < n; ++k) out += (char)('0' + rng() % 70);
        out += '\0';
    } else if (t == 'B') {
        const char sub = "cCsSiIf"[rng() % 7];
        const int32_t cnt = (int32_t)(rng() % 6);
        out += sub;
        out += std::string((const char *)&cnt, 4);
        bytes((size_t)cnt * width_of(sub));
    } else {
        bytes(width_of(t));
    }
    return out;
}

static const char *NAMES[] = {"HP", "PS", "XY", "hp", "H1"};
static long seen[5];

// one region in a buffer of its exact size, through the per-record body
static bool check_region(const std::string &s, const char *tag) {
    uint8_t *buf = (uint8_t *)malloc(s.size() ? s.size() : 1);
    memcpy(buf, s.data(), s.size());
    int64_t got = -1, want = -1;
    const int kind = aux_value(buf, buf + s.size(), tag, &got), wkind = restate(s, tag, &want);
    free(buf);
    if (kind != wkind || got != want) {
        printf("kind %d value %lld, the restatement says %d and %lld (region of %zu bytes)\n", kind, (long long)got, wkind, (long long)want, s.size());
        return false;
    }
    seen[kind] += 1;
    return true;
}

int main() {
    std::mt19937_64 rng(29);
    const char types[] = "AcCsSiIfZHB";
    std::vector<std::string> regions;
    for (int trial = 0; trial < 20000; ++trial) {
        std::string s;
        const int n = (int)(rng() % 6);
        for (int f = 0; f < n; ++f) s += field(rng, NAMES[rng() % 5], types[trial < 11 && f == 0 ? trial : (int)(rng() % 11)]);
        const char *tag = NAMES[rng() % 2];
        if (!check_region(s, tag)) return 1;
        for (size_t cut = 0; cut < s.size(); ++cut)  // every truncation
            if (!check_region(s.substr(0, cut), tag)) return 1;
        for (int m = 0; m < 8 && !s.empty(); ++m) {  // mutations: flipped bytes, then a cut tail
            std::string t = s;
            const int flips = 1 + (int)(rng() % 3);
            for (int f = 0; f < flips; ++f) t[rng() % t.size()] = (char)(rng() % 3 == 0 ? "ABZHcif\0"[rng() % 8] : rng() & 255);
            if (rng() % 3 == 0) t.resize(rng() % (t.size() + 1));
            if (!check_region(t, tag)) return 1;
            if (regions.size() < 4000) regions.push_back(t);
        }
        regions.push_back(s);
    }
    // the batch entry: records of a lead and a region, a tag offset outside the record, no record at all
    for (int trial = 0; trial < 3000; ++trial) {
        const int64_t n = (int64_t)(rng() % 7);
        std::vector<int64_t> raw_off((size_t)n + 1, 0), tags_off((size_t)n), want_v((size_t)n);
        std::vector<int> want_k((size_t)n);
        const char *tag = NAMES[rng() % 2];
        std::string all;
        for (int64_t r = 0; r < n; ++r) {
            const std::string &reg = regions[rng() % regions.size()];
            const int64_t lead = (int64_t)(rng() % 40);
            all += std::string((size_t)lead, 'H') + reg;
            raw_off[(size_t)r + 1] = (int64_t)all.size();
            tags_off[(size_t)r] = lead;
            want_k[(size_t)r] = restate(reg, tag, &want_v[(size_t)r]);
            if (rng() % 50 == 0) {
                tags_off[(size_t)r] = rng() % 2 ? -1 : lead + (int64_t)reg.size() + 1;
                want_k[(size_t)r] = RMR_AUX_UNWALKABLE, want_v[(size_t)r] = 0;
            }
        }
        uint8_t *raw = (uint8_t *)malloc(all.size() ? all.size() : 1);
        memcpy(raw, all.data(), all.size());
        int64_t *value = (int64_t *)malloc(8 * (size_t)(n ? n : 1));
        uint8_t *kind = (uint8_t *)malloc((size_t)(n ? n : 1));
        if (rmr_bam_aux_values(n, raw, raw_off.data(), tags_off.data(), tag, value, kind, 1 + (int)(rng() % 3))) return 1;
        for (int64_t r = 0; r < n; ++r)
            if (kind[r] != want_k[(size_t)r] || value[r] != want_v[(size_t)r]) {
                printf("batch record %lld: kind %d value %lld, the restatement says %d and %lld\n", (long long)r, kind[r], (long long)value[r],
                       want_k[(size_t)r], (long long)want_v[(size_t)r]);
                return 1;
            }
        free(raw), free(value), free(kind);
    }
    uint8_t k1 = 9;
    int64_t v1 = 9;
    const int64_t zero[2] = {0, 0};
    if (rmr_bam_aux_values(0, nullptr, nullptr, nullptr, "HP", nullptr, nullptr, 1) != 0) return 1;
    if (rmr_bam_aux_values(1, nullptr, zero, zero, "H_", &v1, &k1, 1) == 0 || rmr_bam_aux_values(1, nullptr, zero, zero, "1P", &v1, &k1, 1) == 0) return 1;
    if (rmr_bam_aux_values(1, nullptr, zero, zero, "HP", &v1, &k1, 1) != 0 || k1 != RMR_AUX_ABSENT || v1 != 0) return 1;  // an empty record
    printf("aux regions: %ld absent, %ld integer, %ld character, %ld of another type, %ld unwalkable\n", seen[0], seen[1], seen[2], seen[3], seen[4]);
    for (int k = 0; k < 5; ++k)
        if (seen[k] < 1000) return 1;
    return 0;
}
