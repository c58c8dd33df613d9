// The C++ twin of tests/duplex_restate.py for pairs too long for numpy (the 7.8 kb and 24.5 kb fixture pairs): the same
// three-state DP, row by row on one thread, with a 4-bit trace, and the same walk back.  It shares nothing with
// remora_amd/csrc/k_duplex.hip (no strips, no lanes, no skew).  tests/test_host_duplex.py holds it against the numpy form.
//
//   duplex_restate < pairs      one "simplex duplex" pair per line
//   -> per pair one line: status score end_row query_start ref_start ref_end n_runs op:len op:len ...    (M = 0, I = 1, D = 2)
//   -> on stderr: cell updates per second of the fill
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

static const int MATCH = 5, MISMATCH = -4, N_BASE = -2, N_N = -1, OPEN = 10, EXTEND = 2;
static const int32_t NEG = -(1 << 29);  // cannot be entered; scores stay within +-2^28 for sequences below 10^7 bases

static int code(char c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : c == 'N' ? 4 : 5; }
static int subst(int a, int b) { return (a == 4 || b == 4) ? (a == b ? N_N : N_BASE) : (a == b ? MATCH : MISMATCH); }

int main() {
    std::string q, r;
    double cells = 0, secs = 0;
    while (std::cin >> q >> r) {
        const int64_t n = (int64_t)q.size(), m = (int64_t)r.size();
        bool bad = false;
        for (char c : q) bad |= code(c) > 4;
        for (char c : r) bad |= code(c) > 4;
        if (bad) {
            printf("2 0 0 0 0 0 0\n");
            continue;
        }
        std::vector<int> rc(m);
        for (int64_t j = 0; j < m; ++j) rc[j] = code(r[j]);
        const auto t0 = std::chrono::steady_clock::now();
        // trace nibble of cell (i, j), 1-based: bits 0-1 source of H (0 diagonal, 1 E, 2 F), bit 2 E extends, bit 3 F extends
        const int64_t row_bytes = (m + 2) / 2;
        std::vector<uint8_t> T((size_t)((n + 1) * row_bytes), 0);
        std::vector<int32_t> H(m + 1), F(m + 1, NEG);
        H[0] = 0;
        for (int64_t j = 1; j <= m; ++j) H[j] = -(OPEN + EXTEND * (int32_t)(j - 1));
        int64_t best = H[m], best_row = 0;
        for (int64_t i = 1; i <= n; ++i) {
            int32_t diag = H[0], e = NEG;  // H[i-1][0] = 0; E[i][0] cannot be entered
            H[0] = 0;
            const int qi = code(q[i - 1]);
            uint8_t *row = &T[(size_t)(i * row_bytes)];
            for (int64_t j = 1; j <= m; ++j) {
                const int32_t eo = H[j - 1] - OPEN, ee = e - EXTEND;
                e = std::max(eo, ee);
                const int32_t fo = H[j] - OPEN, fe = F[j] - EXTEND;
                const int32_t f = std::max(fo, fe);
                const int32_t d = diag + subst(qi, rc[j - 1]);
                const int32_t g = std::max(e, f), h = std::max(d, g);
                const unsigned nib = (d >= g ? 0u : e >= f ? 1u : 2u) | (ee > eo ? 4u : 0u) | (fe > fo ? 8u : 0u);
                row[j >> 1] |= (uint8_t)(nib << ((j & 1) * 4));
                diag = H[j];
                H[j] = h, F[j] = f;
            }
            if (H[m] > best) best = H[m], best_row = i;
        }
        secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        cells += (double)n * (double)m;
        std::vector<int> path;  // back to front
        int64_t i = best_row, j = m;
        int state = 0;
        while (j > 0) {
            if (i == 0) {
                path.insert(path.end(), (size_t)j, 2);
                j = 0;
                break;
            }
            const unsigned nib = (T[(size_t)(i * row_bytes + (j >> 1))] >> ((j & 1) * 4)) & 15u;
            if (state == 0) {
                state = nib & 3;
                if (state == 0) path.push_back(0), --i, --j;
            } else if (state == 1) {
                path.push_back(2);
                if (!(nib & 4)) state = 0;
                --j;
            } else {
                path.push_back(1);
                if (!(nib & 8)) state = 0;
                --i;
            }
        }
        std::reverse(path.begin(), path.end());
        size_t lo = 0, hi = path.size();
        int64_t query_start = i, ref_start = 0, ref_end = m;
        while (lo < hi && path[lo] != 0) (path[lo] == 2 ? ref_start : query_start) += 1, ++lo;
        while (hi > lo && path[hi - 1] != 0) ref_end -= path[hi - 1] == 2, --hi;
        if (lo == hi) {
            printf("1 0 0 0 0 0 0\n");
            continue;
        }
        std::vector<std::pair<int, int64_t>> runs;
        for (size_t k = lo; k < hi; ++k) {
            if (!runs.empty() && runs.back().first == path[k]) runs.back().second += 1;
            else runs.push_back({path[k], 1});
        }
        printf("0 %lld %lld %lld %lld %lld %zu", (long long)best, (long long)best_row, (long long)query_start, (long long)ref_start,
               (long long)ref_end, runs.size());
        for (auto &run : runs) printf(" %d:%lld", run.first, (long long)run.second);
        printf("\n");
    }
    fprintf(stderr, "%.0f cells in %.3f s = %.3e cell updates/s\n", cells, secs, secs > 0 ? cells / secs : 0.0);
    return 0;
}
