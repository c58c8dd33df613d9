// ref_to_signal.cpp — the signal coordinate of every reference position of an alignment, host code (N3 / N4: reference-anchored
// reads of `infer --reference-anchored` and `dataset prepare`).
// replaces: compute_ref_to_signal = map_ref_to_signal(make_sequence_coordinate_mapping(cigar)), src/remora/data_chunks.py:60-122,
// which are two np.interp passes over float64 arrays of the read's length plus a dozen small numpy calls per read - 0.15 ms
// of the 0.33 ms of host time a 9 kb reference-anchored read costs.  Here: one walk over the CIGAR.
//
// The result is the reference's, bit for bit, because the arithmetic is np.interp's:
//   knots (x = reference, y = query): (0, 0), per match run (M = X) its first and its last base, (ref_len, query_len)
//   - operations behind the last match run are dropped first; knots may repeat an x (a leading soft clip, a match run of
//   one base): np.interp takes the LAST knot with x_j <= x, so only segments of positive width are ever evaluated;
//   y(x) = y_j when x == x_j, else slope * (x - x_j) + y_j with slope = (y_j+1 - y_j) / (x_j+1 - x_j) in float64
//   (exact wherever the slope is 1, i.e. inside match runs; a fraction only across deletions / skips);
//   signal(x) = floor(interp(y(x); 0..n-1 -> query_to_signal)): q2s[k] when y == k, q2s[n-1] when y >= n-1, else
//   (q2s[k+1] - q2s[k]) * (y - k) + q2s[k].
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "rmr_internal.h"

namespace {

enum { R2S_OK = 0, R2S_ROOM = 1, R2S_BAD_OP = 2, R2S_NO_MATCH = 3, R2S_EMPTY_RUN = 4 };

// the walk itself; a code instead of a message, so that a batch can run it on worker threads (rmr_ref_anchor_batch)
int ref_to_signal_core(const uint32_t *cigar, int64_t n_ops, int reverse, const int64_t *query_to_signal, int64_t n_knots,
                       int64_t *ref_to_signal, int64_t cap, int64_t *n_out) {
#pragma STDC FP_CONTRACT OFF
    // M I D N S H P = X: aligns a base / consumes the query / consumes the reference
    static const bool MATCH[9] = {true, false, false, false, false, false, false, true, true};
    static const bool QUERY[9] = {true, true, false, false, true, false, false, true, true};
    static const bool REF[9] = {true, false, true, true, false, false, false, true, true};
    auto op_at = [&](int64_t i) { return cigar[reverse ? n_ops - 1 - i : i]; };
    int64_t last_match = -1;
    for (int64_t i = 0; i < n_ops; ++i) {
        const uint32_t op = op_at(i) & 0xF;
        if (op > 8) return R2S_BAD_OP;
        if (MATCH[op]) last_match = i;
    }
    if (last_match < 0) return R2S_NO_MATCH;
    // the knots
    std::vector<int64_t> xs, ys;
    xs.reserve(2 * (size_t)n_ops + 2);
    ys.reserve(2 * (size_t)n_ops + 2);
    xs.push_back(0);
    ys.push_back(0);
    int64_t r = 0, q = 0;
    for (int64_t i = 0; i <= last_match; ++i) {
        const uint32_t c = op_at(i), op = c & 0xF;
        const int64_t len = (int64_t)(c >> 4);
        if (REF[op]) r += len;
        if (QUERY[op]) q += len;
        if (MATCH[op]) {  // (ref_end - len, ref_end - 1): also for a run of length 0, as the reference's arithmetic does
            xs.push_back(r - len);
            ys.push_back(q - len);
            xs.push_back(r - 1);
            ys.push_back(q - 1);
        }
    }
    xs.push_back(r);
    ys.push_back(q);
    const int64_t total = r + 1;
    *n_out = total;
    if (cap < total) return R2S_ROOM;
    for (size_t j = 1; j < xs.size(); ++j)  // np.interp wants ascending x; a run of length 0 behind nothing would break that
        if (xs[j] < xs[j - 1]) return R2S_EMPTY_RUN;
    const int64_t last_knot = n_knots - 1;
    auto signal_at = [&](double y) -> int64_t {
        if (y >= (double)last_knot) return query_to_signal[last_knot];
        const double fk = std::floor(y);
        const int64_t k = (int64_t)fk;
        if (y == fk) return query_to_signal[k];
        const double y0 = (double)query_to_signal[k], slope = ((double)query_to_signal[k + 1] - y0) / (((double)k + 1.0) - (double)k);
        const double prod = slope * (y - fk);
        return (int64_t)std::floor(prod + y0);
    };
    const size_t nk = xs.size();
    for (size_t j = 0; j + 1 < nk; ++j) {
        const int64_t x0 = xs[j], x1 = xs[j + 1];
        if (x1 <= x0) continue;
        const int64_t y0 = ys[j], y1 = ys[j + 1];
        if (y1 - y0 == x1 - x0 && y0 >= 0 && y1 <= last_knot) {  // slope exactly 1 inside the move table: a copy
            for (int64_t x = x0; x < x1; ++x) ref_to_signal[x] = query_to_signal[y0 + (x - x0)];
            continue;
        }
        const double slope = ((double)y1 - (double)y0) / ((double)x1 - (double)x0);
        ref_to_signal[x0] = signal_at((double)y0);
        for (int64_t x = x0 + 1; x < x1; ++x) {
            const double prod = slope * ((double)x - (double)x0);
            ref_to_signal[x] = signal_at(prod + (double)y0);
        }
    }
    ref_to_signal[r] = signal_at((double)ys[nk - 1]);  // x == the last knot: its y
    return R2S_OK;
}

}  // namespace

extern "C" int rmr_ref_to_signal(const uint32_t *cigar, int64_t n_ops, int reverse, const int64_t *query_to_signal, int64_t n_knots,
                                 int64_t *ref_to_signal, int64_t cap, int64_t *n_out) {
    if (!cigar || n_ops < 0 || !query_to_signal || n_knots < 1 || !ref_to_signal || !n_out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    switch (ref_to_signal_core(cigar, n_ops, reverse, query_to_signal, n_knots, ref_to_signal, cap, n_out)) {
    case R2S_OK: return RMR_OK;
    case R2S_BAD_OP: RMR_FAIL(RMR_ERR_INVALID, "Invalid cigar op(s)");
    case R2S_NO_MATCH: RMR_FAIL(RMR_ERR_INVALID, "No match operations found in alignment cigar");
    case R2S_ROOM: RMR_FAIL(RMR_ERR_INVALID, "ref_to_signal needs %lld entries, %lld given", (long long)*n_out, (long long)cap);
    default: RMR_FAIL(RMR_ERR_INVALID, "cigar with an empty match run");
    }
}

// ---- a batch of alignments: move table -> query_to_signal -> ref_to_signal, per record, on native threads ----------------
// replaces, for the records of one BAM batch: io.parse_move_tag (src/remora/io.py:394-407) followed by compute_ref_to_signal
// (src/remora/data_chunks.py:118-122) inside Read.add_alignment (io.py:2066-2084) - the reference-anchored half of the batch
// ingest (remora_amd.io._ingest_batch).  Record i: move table mv[mv_off[i] .. mv_off[i+1]) (first entry = stride), trimmed
// signal length sig_len[i], seq_len[i] bases, CIGAR words cigar[cigar_off[i] .. cigar_off[i+1]) in BAM order (reverse[i]: the
// read-oriented walk runs it backwards), ref_len[i] reference bases (< 0: no reference sequence - the record is skipped with
// status 9).  ref_to_signal of record i goes to r2s[r2s_off[i] .. r2s_off[i] + ref_len[i] + 1).
// status[i]: 0 done; RMR_ERR_INVALID (empty table / stride <= 0), RMR_ERR_DISCORDANT_SEQ, RMR_ERR_DISCORDANT_SIG as
// rmr_parse_moves_batch; 1 "Discordant ref seq lengths" (io.py:2078-2079); 2 "Invalid cigar op(s)"; 3 "No match operations
// found in alignment cigar"; 4 a CIGAR with an empty match run (the caller's array form handles it); 8 no move table;
// 9 move table fine, no reference sequence.
// `reverse_signal` (signal recorded 3'->5'): query_to_signal = sig_len - query_to_signal[::-1] once the move table has passed
// its checks (io.py:401-402), and the walk interpolates in those coordinates.
extern "C" int rmr_ref_anchor_batch_dir(int64_t n, const int8_t *mv, const int64_t *mv_off, const int64_t *sig_len, const int64_t *seq_len,
                                        const uint32_t *cigar, const int64_t *cigar_off, const uint8_t *reverse, const int64_t *ref_len,
                                        int64_t *r2s, const int64_t *r2s_off, int32_t *status, int reverse_signal, int threads) {
    if (n < 0 || !mv_off || !sig_len || !seq_len || !cigar_off || !reverse || !ref_len || !r2s_off || !status || (n > 0 && (!mv || !r2s)))
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    auto work = [&](int64_t i0, int64_t i1) {
        std::vector<int64_t> q2s;
        for (int64_t i = i0; i < i1; ++i) {
            const int8_t *m = mv + mv_off[i];
            const int64_t len = mv_off[i + 1] - mv_off[i];
            if (len < 1) { status[i] = 8; continue; }  // no move table: the caller's business
            if (m[0] <= 0) { status[i] = RMR_ERR_INVALID; continue; }
            const int64_t stride = m[0], nmv = len - 1;
            q2s.clear();
            for (int64_t k = 0; k < nmv; ++k)
                if (m[1 + k] != 0) q2s.push_back(k * stride);
            const int64_t cnt = (int64_t)q2s.size();
            q2s.push_back(sig_len[i]);
            if (seq_len[i] >= 0 && cnt != seq_len[i]) { status[i] = RMR_ERR_DISCORDANT_SEQ; continue; }
            if (nmv != sig_len[i] / stride) { status[i] = RMR_ERR_DISCORDANT_SIG; continue; }
            if (ref_len[i] < 0) { status[i] = 9; continue; }  // (the move table is checked first, as add_alignment does)
            if (reverse_signal) {
                for (int64_t a = 0, b = cnt; a <= b; ++a, --b) {
                    const int64_t lo = sig_len[i] - q2s[(size_t)b], hi = sig_len[i] - q2s[(size_t)a];
                    q2s[(size_t)a] = lo;
                    q2s[(size_t)b] = hi;
                }
            }
            int64_t n_out = 0;
            const int rc = ref_to_signal_core(cigar + cigar_off[i], cigar_off[i + 1] - cigar_off[i], reverse[i] != 0, q2s.data(), (int64_t)q2s.size(),
                                              r2s + r2s_off[i], ref_len[i] + 1, &n_out);
            status[i] = rc == R2S_OK ? (n_out == ref_len[i] + 1 ? 0 : 1) : rc == R2S_ROOM ? 1 : rc;
        }
    };
    if (threads < 1) threads = 1;
    if (threads > 32) threads = 32;
    if (threads == 1 || n < 2 * threads) {
        work(0, n);
        return RMR_OK;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back(work, n * t / threads, n * (t + 1) / threads);
    for (auto &th : pool) th.join();
    return RMR_OK;
}

extern "C" int rmr_ref_anchor_batch(int64_t n, const int8_t *mv, const int64_t *mv_off, const int64_t *sig_len, const int64_t *seq_len,
                                    const uint32_t *cigar, const int64_t *cigar_off, const uint8_t *reverse, const int64_t *ref_len,
                                    int64_t *r2s, const int64_t *r2s_off, int32_t *status, int threads) {
    return rmr_ref_anchor_batch_dir(n, mv, mv_off, sig_len, seq_len, cigar, cigar_off, reverse, ref_len, r2s, r2s_off, status, 0, threads);
}
