// AddressSanitizer + UBSan harness for rmr_ref_anchor_batch_dir (host code, no GPU): the reference-anchor composition of a BAM
// batch for either signal direction.  Random move tables and CIGARs, both strands, both directions, output slots of exact
// size; every record's status and knots are compared with a straightforward scalar restatement of what the per-read path
// does in numpy: io.parse_move_tag (src/remora/io.py:394-407, reverse_signal: sig_len - query_to_signal[::-1]), then
// make_sequence_coordinate_mapping and map_ref_to_signal (src/remora/data_chunks.py:60-122) as two np.interp passes.  With
// reverse_signal = 0 the result must also be rmr_ref_anchor_batch's.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../remora_amd/csrc/ref_to_signal.cpp"

namespace rmr {
void set_error(const char *, ...) {}
}  // namespace rmr

#pragma STDC FP_CONTRACT OFF

namespace {

// np.interp for one x over ascending xp (the last knot with xp[j] <= x where knots repeat)
double interp(double x, const std::vector<double> &xp, const std::vector<double> &fp) {
    const size_t n = xp.size();
    if (x > xp[n - 1]) return fp[n - 1];
    if (x < xp[0]) return fp[0];
    size_t j = 0;
    for (size_t k = 0; k < n; ++k)
        if (xp[k] <= x) j = k;
    if (j == n - 1 || xp[j] == x) return fp[j];
    const double slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    return slope * (x - xp[j]) + fp[j];
}

// status of one record, its knots in `out` when the status is 0
int restate(const int8_t *m, int64_t mv_len, int64_t sig_len, int64_t seq_len, const uint32_t *cig, int64_t n_ops, bool strand_rev,
            int64_t ref_len, bool reverse_signal, std::vector<int64_t> &out) {
    static const bool MATCH[9] = {true, false, false, false, false, false, false, true, true};
    static const bool QUERY[9] = {true, true, false, false, true, false, false, true, true};
    static const bool REF[9] = {true, false, true, true, false, false, false, true, true};
    if (mv_len < 1) return 8;
    if (m[0] <= 0) return RMR_ERR_INVALID;
    std::vector<int64_t> q2s;
    for (int64_t k = 0; k + 1 < mv_len; ++k)
        if (m[1 + k] != 0) q2s.push_back(k * (int64_t)m[0]);
    q2s.push_back(sig_len);
    if (seq_len >= 0 && (int64_t)q2s.size() - 1 != seq_len) return RMR_ERR_DISCORDANT_SEQ;
    if (mv_len - 1 != sig_len / m[0]) return RMR_ERR_DISCORDANT_SIG;
    if (ref_len < 0) return 9;
    if (reverse_signal) {
        std::vector<int64_t> r(q2s.size());
        for (size_t j = 0; j < q2s.size(); ++j) r[j] = sig_len - q2s[q2s.size() - 1 - j];
        q2s = r;
    }
    std::vector<uint32_t> ops(cig, cig + n_ops);
    if (strand_rev) std::reverse(ops.begin(), ops.end());
    int64_t last_match = -1;
    for (int64_t i = 0; i < n_ops; ++i) {
        if ((ops[(size_t)i] & 0xF) > 8) return 2;
        if (MATCH[ops[(size_t)i] & 0xF]) last_match = i;
    }
    if (last_match < 0) return 3;
    std::vector<double> rk{0.0}, qk{0.0};
    int64_t r = 0, q = 0;
    for (int64_t i = 0; i <= last_match; ++i) {
        const uint32_t op = ops[(size_t)i] & 0xF;
        const int64_t len = (int64_t)(ops[(size_t)i] >> 4);
        if (REF[op]) r += len;
        if (QUERY[op]) q += len;
        if (MATCH[op]) {
            rk.push_back((double)(r - len)); qk.push_back((double)(q - len));
            rk.push_back((double)(r - 1)); qk.push_back((double)(q - 1));
        }
    }
    rk.push_back((double)r);
    qk.push_back((double)q);
    if (r + 1 > ref_len + 1) return 1;
    for (size_t j = 1; j < rk.size(); ++j)
        if (rk[j] < rk[j - 1]) return 4;
    if (r + 1 != ref_len + 1) return 1;
    std::vector<double> idx(q2s.size()), sig(q2s.size());
    for (size_t j = 0; j < q2s.size(); ++j) { idx[j] = (double)j; sig[j] = (double)q2s[j]; }
    out.resize((size_t)r + 1);
    for (int64_t x = 0; x <= r; ++x) out[(size_t)x] = (int64_t)std::floor(interp(interp((double)x, rk, qk), idx, sig));
    return 0;
}

}  // namespace

int main() {
    setvbuf(stdout, nullptr, _IONBF, 0);  // (a failure's message must not die in a buffer when the leak check ends the process)
    std::mt19937_64 rng(23);
    long anchored[2] = {0, 0}, turned_away = 0;
    for (int trial = 0; trial < 3000; ++trial) {
        const int64_t n = 1 + (int64_t)(rng() % 40);
        std::vector<int8_t> mv;
        std::vector<int64_t> mv_off{0}, sig_len, seq_len, cigar_off{0}, ref_len, r2s_off{0};
        std::vector<uint32_t> cigar;
        std::vector<uint8_t> rev;
        for (int64_t i = 0; i < n; ++i) {
            const bool hostile = rng() % 8 == 0;
            const int stride = hostile ? (int)(rng() % 9) - 2 : 1 + (int)(rng() % 6);
            int64_t q = 0, r = 0;
            const int n_ops = 1 + (int)(rng() % 8);
            for (int k = 0; k < n_ops; ++k) {
                const uint32_t op = hostile ? (uint32_t)(rng() % 16) : (uint32_t)("\0\0\0\1\2\3\4\7\10"[rng() % 9]);
                const uint32_t len = (hostile ? 0u : 1u) + (uint32_t)(rng() % 30);
                cigar.push_back((len << 4) | op);
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) q += len;
                if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) r += len;
            }
            cigar_off.push_back((int64_t)cigar.size());
            const int64_t nb = rng() % 9 == 0 ? (int64_t)(rng() % 120) : q;  // bases the move table encodes: mostly the CIGAR's
            if (rng() % 13 != 0) {  // a move table (else: none)
                mv.push_back((int8_t)stride);
                int64_t placed = 0;
                const int64_t moves = nb * 2 + (int64_t)(rng() % 5);
                for (int64_t k = 0; k < moves; ++k) {
                    const bool one = placed < nb && k < 2 * nb && ((rng() & 1) || 2 * nb - k <= nb - placed);  // nb ones in all
                    mv.push_back(hostile ? (int8_t)(rng() % 3 - 1) : (int8_t)one);
                    placed += one;
                }
                const int64_t s = stride > 0 ? stride : 1;
                sig_len.push_back(hostile && rng() % 2 ? (int64_t)(rng() % 2000) : moves * s + (int64_t)(rng() % (uint64_t)s));
            } else {
                sig_len.push_back((int64_t)(rng() % 100));
            }
            mv_off.push_back((int64_t)mv.size());
            seq_len.push_back(rng() % 11 == 0 ? (int64_t)(rng() % 200) : nb);
            const int64_t rl = rng() % 11 == 0 ? -1 : (rng() % 7 == 0 ? (int64_t)(rng() % 300) : r);
            ref_len.push_back(rl);
            r2s_off.push_back(r2s_off.back() + (rl < 0 ? 0 : rl + 1));
            rev.push_back((uint8_t)(rng() & 1));
        }
        if (mv.empty()) mv.push_back(0);
        if (cigar.empty()) cigar.push_back(0);
        const size_t slots = (size_t)(r2s_off.back() > 0 ? r2s_off.back() : 1);
        for (int dir = 0; dir < 2; ++dir) {
            // exact-size output: a write behind the last record's slot is ASan's to see
            int64_t *out = (int64_t *)malloc(sizeof(int64_t) * slots);
            std::vector<int32_t> status((size_t)n, 77);
            const int rc = rmr_ref_anchor_batch_dir(n, mv.data(), mv_off.data(), sig_len.data(), seq_len.data(), cigar.data(), cigar_off.data(),
                                                    rev.data(), ref_len.data(), out, r2s_off.data(), status.data(), dir, 1 + (int)(rng() % 6));
            if (rc != 0) { printf("rmr_ref_anchor_batch_dir rc %d\n", rc); return 1; }
            std::vector<int64_t> want;
            for (int64_t i = 0; i < n; ++i) {
                const int st = restate(mv.data() + mv_off[i], mv_off[i + 1] - mv_off[i], sig_len[i], seq_len[i], cigar.data() + cigar_off[i],
                                       cigar_off[i + 1] - cigar_off[i], rev[i] != 0, ref_len[i], dir != 0, want);
                if (status[i] != st) { printf("trial %d record %lld dir %d: status %d, restatement %d\n", trial, (long long)i, dir, status[i], st); return 1; }
                if (st != 0) { ++turned_away; continue; }
                ++anchored[dir];
                if (memcmp(out + r2s_off[i], want.data(), sizeof(int64_t) * want.size()) != 0) {
                    printf("trial %d record %lld dir %d strand %d: knots differ from the restatement\n", trial, (long long)i, dir, (int)rev[i]);
                    return 1;
                }
            }
            if (dir == 0) {  // the old entry is the new one with direction 0
                int64_t *old_out = (int64_t *)malloc(sizeof(int64_t) * slots);
                std::vector<int32_t> old_status((size_t)n, 77);
                if (rmr_ref_anchor_batch(n, mv.data(), mv_off.data(), sig_len.data(), seq_len.data(), cigar.data(), cigar_off.data(), rev.data(),
                                         ref_len.data(), old_out, r2s_off.data(), old_status.data(), 2) != 0) { printf("rmr_ref_anchor_batch rc\n"); return 1; }
                for (int64_t i = 0; i < n; ++i)
                    if (old_status[i] != status[i] ||
                        (status[i] == 0 && memcmp(old_out + r2s_off[i], out + r2s_off[i], sizeof(int64_t) * (size_t)(ref_len[i] + 1)) != 0)) {
                        printf("rmr_ref_anchor_batch differs from direction 0\n");
                        return 1;
                    }
                free(old_out);
            }
            free(out);
        }
    }
    printf("%ld forward and %ld reversed records anchored and equal to the restatement, %ld turned away\n", anchored[0], anchored[1], turned_away);
    if (anchored[0] < 10000 || anchored[1] < 10000) { printf("too few records anchored to mean anything\n"); return 1; }
    return 0;
}
