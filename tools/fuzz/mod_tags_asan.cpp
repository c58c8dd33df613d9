// AddressSanitizer + UBSan harness for the MM / ML tokeniser (rmr_mod_tags_sizes / rmr_mod_tags_fill, remora_amd/csrc/mod_tags.cpp):
// tag regions built from the grammar, then truncated and mutated byte by byte, in record buffers of exact size - every read stays
// inside the record; outputs of exactly the counted size - every write stays inside them; the entries of a record tile its
// delta and ML ranges without a gap, and a status other than 0 owns nothing.
#include <cstdarg>
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

static std::string tag_region(std::mt19937_64 &rng) {
    std::string mm;
    int64_t need = 0;
    const int n_ent = (int)(rng() % 4);
    for (int e = 0; e < n_ent; ++e) {
        mm += "ACGTUN"[rng() % 6];
        mm += "+-"[rng() % 2];
        int codes = 1;
        if (rng() % 4 == 0) {
            mm += std::to_string(rng() % 100000);
        } else {
            codes = 1 + (int)(rng() % 3);
            for (int c = 0; c < codes; ++c) mm += (char)('a' + rng() % 26);
        }
        if (rng() % 3) mm += ".?"[rng() % 2];
        const int n = (int)(rng() % 6);
        for (int k = 0; k < n; ++k) mm += "," + std::to_string(rng() % 50);
        mm += ';';
        need += (int64_t)codes * n;
    }
    std::string out;
    if (rng() % 3 == 0) out += std::string("NMC\x05", 4);
    if (rng() % 8) out += (rng() % 5 ? "MMZ" : "MmZ") + mm + std::string(1, '\0');
    if (rng() % 8) {
        int64_t n = need;
        if (rng() % 6 == 0) n += (int64_t)(rng() % 3) - 1;
        if (n < 0) n = 0;
        const int32_t cnt = (int32_t)n;
        out += rng() % 5 ? "MLBC" : "MlBC";
        out += std::string((const char *)&cnt, 4);
        for (int64_t i = 0; i < n; ++i) out += (char)(rng() & 255);
    }
    if (rng() % 3 == 0) out += std::string("tsi\x07\x00\x00\x00", 7);
    if (rng() % 4 == 0 && !out.empty()) {  // mutations: flipped bytes, a truncated tail
        const int flips = 1 + (int)(rng() % 3);
        for (int f = 0; f < flips; ++f) out[rng() % out.size()] = (char)(rng() & 255);
        if (rng() % 2) out.resize(rng() % (out.size() + 1));
    }
    return out;
}

int main() {
    std::mt19937_64 rng(11);
    long ok = 0, none = 0, bad = 0;
    for (int trial = 0; trial < 20000; ++trial) {
        const int64_t n = (int64_t)(rng() % 6);
        std::vector<int64_t> raw_off((size_t)n + 1, 0), tags_off((size_t)n);
        std::string all;
        for (int64_t r = 0; r < n; ++r) {
            const int64_t lead = (int64_t)(rng() % 40);
            all += std::string((size_t)lead, 'x') + tag_region(rng);
            tags_off[(size_t)r] = lead;
            raw_off[(size_t)r + 1] = (int64_t)all.size();
        }
        uint8_t *raw = (uint8_t *)malloc(all.size() ? all.size() : 1);  // exact size: one byte beyond the last record is ASan's
        memcpy(raw, all.data(), all.size());
        std::vector<int32_t> status((size_t)n + 1);
        std::vector<int64_t> ne((size_t)n + 1), nd((size_t)n + 1), nm((size_t)n + 1);
        const int threads = 1 + (int)(rng() % 3);
        if (rmr_mod_tags_sizes(n, raw, raw_off.data(), tags_off.data(), status.data(), ne.data(), nd.data(), nm.data(), threads)) return 1;
        std::vector<int64_t> eo((size_t)n + 1, 0), dof((size_t)n + 1, 0), mo((size_t)n + 1, 0);
        for (int64_t r = 0; r < n; ++r) {
            if (status[(size_t)r] < 0 || status[(size_t)r] > 2) { printf("status out of range\n"); return 1; }
            if (status[(size_t)r] && (ne[(size_t)r] || nd[(size_t)r] || nm[(size_t)r])) { printf("a skipped record owns something\n"); return 1; }
            eo[(size_t)r + 1] = eo[(size_t)r] + ne[(size_t)r];
            dof[(size_t)r + 1] = dof[(size_t)r] + nd[(size_t)r];
            mo[(size_t)r + 1] = mo[(size_t)r] + nm[(size_t)r];
            (status[(size_t)r] == 0 ? ok : status[(size_t)r] == 1 ? none : bad) += 1;
        }
        rmr_mod_entry *ents = (rmr_mod_entry *)malloc(sizeof(rmr_mod_entry) * (size_t)(eo[(size_t)n] ? eo[(size_t)n] : 1));
        int32_t *deltas = (int32_t *)malloc(4 * (size_t)(dof[(size_t)n] ? dof[(size_t)n] : 1));
        uint8_t *ml = (uint8_t *)malloc((size_t)(mo[(size_t)n] ? mo[(size_t)n] : 1));
        if (rmr_mod_tags_fill(n, raw, raw_off.data(), tags_off.data(), status.data(), eo.data(), dof.data(), mo.data(), ents, deltas, ml, threads)) {
            printf("fill refused its own counts\n");
            return 1;
        }
        for (int64_t r = 0; r < n; ++r) {
            int64_t d = dof[(size_t)r], m = mo[(size_t)r];
            for (int64_t e = eo[(size_t)r]; e < eo[(size_t)r + 1]; ++e) {
                if (ents[e].delta_off != d || ents[e].ml_off != m || ents[e].n_codes < 1 || ents[e].n_codes > RMR_MOD_MAX_CODES || ents[e].n_deltas < 0) {
                    printf("entry ranges do not tile the record\n");
                    return 1;
                }
                for (int64_t k = 0; k < ents[e].n_deltas; ++k)
                    if (deltas[d + k] < 0) { printf("negative delta\n"); return 1; }
                d += ents[e].n_deltas;
                m += (int64_t)ents[e].n_deltas * ents[e].n_codes;
            }
            if (d != dof[(size_t)r + 1] || m != mo[(size_t)r + 1]) { printf("entry ranges do not fill the record\n"); return 1; }
        }
        free(ents), free(deltas), free(ml), free(raw);
    }
    printf("%ld records tokenised, %ld without MM, %ld malformed\n", ok, none, bad);
    return ok > 1000 && bad > 1000 ? 0 : 1;
}
