// AddressSanitizer harness for the FASTA packing arithmetic of `analyze pileup_modbams --ref` (remora_amd/csrc/rmr_ref_pack.h:
// what rmr_ref_genome_load does on the host and what every thread of the pack kernel does, in plain C++).  Random contigs at
// random line widths, LF and CRLF, cut into pieces of random size: the text and each piece live in buffers of exact size, so
// every read the piece plan and the per-thread code make is checked; the packed bytes and the first violation (a byte that
// is no IUPAC letter, a wrong terminator, a line of another width) must equal a byte-by-byte restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../remora_amd/csrc/rmr_ref_pack.h"

using namespace rmr;

static int naive_code(int c) {
    static const char *letters = "ACGTURYSWKMBDHVN";
    static const int codes[16] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 12, 3, 14, 13, 11, 7, 15};
    for (int i = 0; i < 16; ++i)
        if (c == letters[i] || c == letters[i] + 32) return codes[i];
    return 0;
}

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "ref_pack_asan: %s failed at line %d\n", #cond, __LINE__); \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

int main() {
    for (int c = -300; c < 600; ++c) CHECK(iupac_code(c) == ((c >= 0 && c < 256) ? naive_code(c) : 0));
    std::mt19937_64 rng(11);
    const std::string alphabet = "ACGTURYSWKMBDHVNacgturyswkmbdhvn";
    long pieces = 0, violations = 0;
    for (int trial = 0; trial < 60000; ++trial) {
        const int64_t lb = 1 + (int64_t)(rng() % (trial % 3 == 0 ? 4 : 70)), term = 1 + (int64_t)(rng() % 2), W = lb + term;
        const int64_t len = (int64_t)(rng() % (trial % 7 == 0 ? 6 : 400));
        const int64_t piece_bytes = 16 + (int64_t)(rng() % (trial % 5 == 0 ? 8 : 300));
        std::string s;
        for (int64_t i = 0; i < len; ++i) {
            s.push_back(alphabet[rng() % alphabet.size()]);
            if ((i + 1) % lb == 0 && i + 1 < len) s += term == 2 ? "\r\n" : "\n";
        }
        const int kind = (int)(rng() % 4);  // 0, 1: a clean text
        if (kind == 2 && !s.empty()) s[rng() % s.size()] = (char)(rng() % 256);  // any byte anywhere
        if (kind == 3 && s.size() > 2) s.erase(rng() % s.size(), 1);             // a line of another width (or a base less)
        const int64_t S = (int64_t)s.size();
        std::vector<uint8_t> text(s.begin(), s.end());  // exact size
        const int64_t held = ref_bases_of_text(S, lb, W);
        if (kind < 2) CHECK(held == len);
        if (held == 0) continue;
        // the restatement: every byte of the text by its column
        unsigned long long want_bad = ~0ull;
        for (int64_t o = S - 1; o >= 0; --o) {
            const int64_t col = o % W;
            const bool ok = col < lb ? naive_code(text[(size_t)o]) != 0 : text[(size_t)o] == ((term == 2 && col == lb) ? '\r' : '\n');
            if (!ok) want_bad = (unsigned long long)o;
        }
        std::vector<uint8_t> want((size_t)(held + 1) / 2, 0), got((size_t)(held + 1) / 2, 0xEE);
        for (int64_t i = 0; i < held; ++i) want[(size_t)(i / 2)] |= (uint8_t)(naive_code(text[(size_t)((i / lb) * W + i % lb)]) << (4 * (i & 1)));
        // the load: piece by piece, each in a buffer of its own size
        unsigned long long got_bad = ~0ull;
        int64_t end = 0;
        for (int64_t i0 = 0; i0 < held;) {
            int64_t t_lo = -1, t_n = -1;
            const int64_t nb = ref_next_piece(i0, held, lb, W, S, piece_bytes, &t_lo, &t_n);
            CHECK(nb >= 1 && i0 % 2 == 0 && (nb % 2 == 0 || i0 + nb == held));
            CHECK(t_lo == end && t_n >= 1 && t_n <= piece_bytes && t_lo + t_n <= S);
            std::vector<uint8_t> piece(text.begin() + t_lo, text.begin() + t_lo + t_n);
            for (int64_t t = 0; 2 * t < nb; ++t) {
                unsigned long long bad = 0;
                got[(size_t)(i0 / 2 + t)] = (uint8_t)ref_pack_pair(piece.data(), t_lo, t_n, S, i0 + 2 * t, i0 + nb, lb, W, &bad);
                if (bad < got_bad) got_bad = bad;
            }
            end = t_lo + t_n, i0 += nb, ++pieces;
        }
        CHECK(end == S);  // every byte of the text was in a piece
        CHECK(got == want);
        CHECK(got_bad == want_bad);
        if (kind < 2) CHECK(got_bad == ~0ull);
        violations += got_bad != ~0ull;
    }
    std::printf("ref_pack_asan: 60000 contigs in %ld pieces, %ld with a violation found at the restatement's offset\n", pieces, violations);
    return 0;
}
