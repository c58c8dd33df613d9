// api_data.hip — the data entry points of the C ABI: k-mer encoding, context trimming, move tables, signal histograms, read
// assembly, chunk extraction, label counts, the validation tally, motif scans, the VBZ decode, the site join of `validate from_modbams`, the duplex alignment and the read-id index of a POD5 dataset (the per-site pileup of `analyze pileup_modbams` is api_pileup.hip).  Each RMR_MEM_HOST call
// declares its arrays in a Stage (rmr_stage.h), uploads, launches (k_data.hip, k_vbz.hip, k_modbam.hip, k_duplex.hip, k_read_index.hip) and copies back.
#include <algorithm>
#include <cstring>
#include <new>

#include "rmr_internal.h"
#include "rmr_stage.h"

using namespace rmr;

extern "C" {

int rmr_encode_kmers(rmr_engine *e, int kb, int ka, const int8_t *seqs, int seq_w,
                     const int16_t *maps, int map_w, const int16_t *lens, int64_t n, int sig_len,
                     float *out, int mem) {
    if (!e || !seqs || !maps || !lens || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (kb < 0 || ka < 0 || n < 0 || sig_len <= 0 || seq_w <= 0 || map_w <= 0)
        RMR_FAIL(RMR_ERR_INVALID, "bad sizes");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    const size_t out_b = (size_t)n * 4 * (kb + ka + 1) * sig_len * sizeof(float);
    if (mem == RMR_MEM_DEVICE) return launch_encode(e, kb, ka, seqs, seq_w, maps, map_w, lens, n, sig_len, out);
    Stage st;
    int8_t *ds;
    int16_t *dm, *dl;
    float *dout;
    st.add(&ds, n * seq_w).add(&dm, n * map_w).add(&dl, n).add(&dout, out_b / 4);
    RMR_TRY(st.commit(e));
    H2D(ds, seqs, (size_t)n * seq_w);
    H2D(dm, maps, (size_t)n * map_w * 2);
    H2D(dl, lens, (size_t)n * 2);
    RMR_TRY(launch_encode(e, kb, ka, ds, seq_w, dm, map_w, dl, n, sig_len, dout));
    D2H(out, dout, out_b);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_trim_chunk_context(rmr_engine *e, int sb, int sa, int cb, int ca, int tsc, int8_t *seqs,
                           int seq_w, int16_t *maps, int map_w, int16_t *lens, int64_t n, int mem) {
    if (!e || !seqs || !maps || !lens) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE) return launch_trim(e, sb, sa, cb, ca, tsc, seqs, seq_w, maps, map_w, lens, n);
    Stage st;
    int8_t *ds;
    int16_t *dm, *dl;
    st.add(&ds, n * seq_w).add(&dm, n * map_w).add(&dl, n);
    RMR_TRY(st.commit(e));
    H2D(ds, seqs, (size_t)n * seq_w);
    H2D(dm, maps, (size_t)n * map_w * 2);
    H2D(dl, lens, (size_t)n * 2);
    RMR_TRY(launch_trim(e, sb, sa, cb, ca, tsc, ds, seq_w, dm, map_w, dl, n));
    D2H(seqs, ds, (size_t)n * seq_w);
    D2H(maps, dm, (size_t)n * map_w * 2);
    D2H(lens, dl, (size_t)n * 2);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_parse_moves(rmr_engine *e, const int8_t *mv_tag, int64_t mv_tag_len, int64_t sig_len,
                    int64_t seq_len, int check, int reverse_signal, int64_t *q2s, int64_t *n_out,
                    int mem) {
    if (!e || !mv_tag || !q2s || !n_out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (mv_tag_len < 1) RMR_FAIL(RMR_ERR_INVALID, "empty move tag");
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    Stage st;
    int64_t *dcount, *dq = q2s;
    const int8_t *dmv = mv_tag;
    st.add(&dcount, 1);
    if (mem == RMR_MEM_HOST) st.add(&dmv, mv_tag_len).add(&dq, mv_tag_len + 1);
    RMR_TRY(st.commit(e));
    int8_t stride_h = 0;
    if (mem == RMR_MEM_HOST) {
        H2D((void *)dmv, mv_tag, (size_t)mv_tag_len);
        stride_h = mv_tag[0];
    } else {
        RMR_HIP(hipMemcpyAsync(&stride_h, mv_tag, 1, hipMemcpyDeviceToHost, e->stream));
    }
    RMR_TRY(launch_moves(e, dmv, mv_tag_len, sig_len, reverse_signal, dq, dcount));
    int64_t cnt = 0;
    D2H(&cnt, dcount, 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    if (mem == RMR_MEM_HOST) {
        RMR_HIP(hipMemcpy(q2s, dq, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    }
    *n_out = cnt;
    if (stride_h <= 0) RMR_FAIL(RMR_ERR_INVALID, "move table stride %d", (int)stride_h);
    if (check && seq_len >= 0 && cnt - 1 != seq_len) {
        set_error("Move table discordant with basecalls");
        return RMR_ERR_DISCORDANT_SEQ;
    }
    if (check && (mv_tag_len - 1) != sig_len / stride_h) {
        set_error("Move table discordant with signal");
        return RMR_ERR_DISCORDANT_SIG;
    }
    return 0;
}

int rmr_parse_moves_batch(rmr_engine *e, const int8_t *mv_tags, const int64_t *mv_off, const int64_t *sig_len,
                          const int64_t *seq_len, int64_t n_reads, int check, int reverse_signal, int64_t *q2s,
                          int64_t *counts, int32_t *status, int mem) {
    if (!e || !mv_tags || !mv_off || !sig_len || !seq_len || !q2s || !counts || !status)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE)
        return launch_moves_batch(e, mv_tags, mv_off, sig_len, seq_len, n_reads, check, reverse_signal, q2s, counts, status);
    const int64_t total = mv_off[n_reads];
    if (mv_off[0] != 0 || total < n_reads) RMR_FAIL(RMR_ERR_INVALID, "bad move table offsets");
    Stage st;
    int8_t *dmv;
    int64_t *doff, *dsl, *dql, *dq, *dcnt;
    int32_t *dst;
    st.add(&dmv, total).add(&doff, n_reads + 1).add(&dsl, n_reads).add(&dql, n_reads).add(&dq, total).add(&dcnt, n_reads);
    st.add(&dst, n_reads);
    RMR_TRY(st.commit(e));
    H2D(dmv, mv_tags, (size_t)total);
    H2D(doff, mv_off, (size_t)(n_reads + 1) * 8);
    H2D(dsl, sig_len, (size_t)n_reads * 8);
    H2D(dql, seq_len, (size_t)n_reads * 8);
    RMR_TRY(launch_moves_batch(e, dmv, doff, dsl, dql, n_reads, check, reverse_signal, dq, dcnt, dst));
    D2H(q2s, dq, (size_t)total * 8);
    D2H(counts, dcnt, (size_t)n_reads * 8);
    D2H(status, dst, (size_t)n_reads * 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_signal_histograms(rmr_engine *e, const int16_t *signal, const int64_t *start, const int64_t *len, int64_t n, int32_t *lo, int32_t *hi,
                          const int64_t *hist_off, uint32_t *hist) {
    if (!e || !signal || !start || !len || !lo || !hi || (hist != nullptr) != (hist_off != nullptr)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n < 0 || n > (int64_t)1 << 24) RMR_FAIL(RMR_ERR_INVALID, "bad n");
    if (n == 0) return 0;
    for (int64_t i = 0; i < n; ++i)
        if (start[i] < 0 || len[i] < 0) RMR_FAIL(RMR_ERR_INVALID, "span %lld: negative extent", (long long)i);
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    const size_t nn = (size_t)n;
    Stage st;
    int64_t *d_start, *d_len;
    int32_t *d_lo;
    st.add(&d_start, nn).add(&d_len, nn).add(&d_lo, nn);
    if (!hist) {  // pass 1: the range of every span
        int32_t *d_hi;
        st.add(&d_hi, nn);
        RMR_TRY(st.commit(e));
        H2D(d_start, start, nn * 8);
        H2D(d_len, len, nn * 8);
        RMR_TRY(launch_signal_range(e, signal, d_start, d_len, n, d_lo, d_hi));
        D2H(lo, d_lo, nn * 4);
        D2H(hi, d_hi, nn * 4);
        RMR_HIP(hipStreamSynchronize(e->stream));
        return 0;
    }
    // pass 2: counts over [lo, hi] of every span, at the offsets the caller summed up
    if (hist_off[0] != 0) RMR_FAIL(RMR_ERR_INVALID, "hist_off[0] != 0");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t width = len[i] > 0 ? (int64_t)hi[i] - lo[i] + 1 : 0;
        if (hist_off[i + 1] - hist_off[i] != (width > 0 ? width : 0)) RMR_FAIL(RMR_ERR_INVALID, "span %lld: hist_off does not match hi - lo + 1", (long long)i);
    }
    const size_t total = (size_t)hist_off[n];
    if (total == 0) return 0;
    int64_t *d_off;
    uint32_t *d_hist;
    st.add(&d_off, nn + 1).add(&d_hist, total);
    RMR_TRY(st.commit(e));
    H2D(d_start, start, nn * 8);
    H2D(d_len, len, nn * 8);
    H2D(d_lo, lo, nn * 4);
    H2D(d_off, hist_off, (nn + 1) * 8);
    RMR_HIP(hipMemsetAsync(d_hist, 0, total * 4, e->stream));
    RMR_TRY(launch_signal_hist(e, signal, d_start, d_len, d_lo, d_off, n, d_hist));
    D2H(hist, d_hist, total * 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_assemble_reads_dir(rmr_engine *e, int64_t n_reads, const int16_t *signal, const int64_t *src_start, const int64_t *span_len,
                           int reverse_signal, const int64_t *q2s, const int64_t *q2s_off, const int64_t *seq_len, int16_t *dacs,
                           int64_t dacs_cap, int64_t *s2s, int64_t *d_sig_off, int64_t *d_seq_off, int64_t *sig_off) {
    if (!e || !signal || !src_start || !q2s || !q2s_off || !seq_len || !dacs || !s2s || !d_sig_off || !d_seq_off || !sig_off)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (reverse_signal && !span_len) RMR_FAIL(RMR_ERR_INVALID, "reversed signal needs span_len");
    if (n_reads < 0) RMR_FAIL(RMR_ERR_INVALID, "bad sizes");
    sig_off[0] = 0;
    if (n_reads == 0) return 0;
    const size_t n = (size_t)n_reads;
    if (reverse_signal)
        for (size_t i = 0; i < n; ++i)
            if (span_len[i] < 0 || src_start[i] < 0) RMR_FAIL(RMR_ERR_INVALID, "read %zu: negative signal window", i);
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    Stage st;
    int64_t *d_start, *d_qoff, *d_slen, *d_len, *d_span = nullptr;
    st.add(&d_start, n).add(&d_qoff, n).add(&d_slen, n).add(&d_len, n);
    if (reverse_signal) st.add(&d_span, n);
    RMR_TRY(st.commit(e));
    H2D(d_start, src_start, n * 8);
    H2D(d_qoff, q2s_off, n * 8);
    H2D(d_slen, seq_len, n * 8);
    if (reverse_signal) H2D(d_span, span_len, n * 8);
    RMR_TRY(launch_assemble_lengths(e, q2s, d_qoff, d_slen, d_span, n_reads, d_len));
    std::vector<int64_t> len(n), seq_off(n + 1, 0);
    D2H(len.data(), d_len, n * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < n; ++i) {
        if (len[i] == INT64_MIN) RMR_FAIL(RMR_ERR_INVALID, "read %zu: a mapping that leaves its signal window", i);
        if (len[i] < 0 || seq_len[i] < 0) RMR_FAIL(RMR_ERR_INVALID, "read %zu: a mapping that runs backwards", i);
        sig_off[i + 1] = sig_off[i] + len[i];
        seq_off[i + 1] = seq_off[i] + seq_len[i];
    }
    if (sig_off[n] > dacs_cap) RMR_FAIL(RMR_ERR_INVALID, "dacs capacity %lld < %lld samples", (long long)dacs_cap, (long long)sig_off[n]);
    H2D(d_sig_off, sig_off, (n + 1) * 8);
    H2D(d_seq_off, seq_off.data(), (n + 1) * 8);
    RMR_TRY(launch_assemble_reads(e, signal, d_start, d_span, q2s, d_qoff, d_sig_off, d_seq_off, n_reads, dacs, s2s));
    RMR_HIP(hipStreamSynchronize(e->stream));  // (the pageable offset vectors above are read by the copies)
    return 0;
}

int rmr_assemble_reads(rmr_engine *e, int64_t n_reads, const int16_t *signal, const int64_t *src_start, const int64_t *q2s,
                       const int64_t *q2s_off, const int64_t *seq_len, int16_t *dacs, int64_t dacs_cap, int64_t *s2s,
                       int64_t *d_sig_off, int64_t *d_seq_off, int64_t *sig_off) {
    return rmr_assemble_reads_dir(e, n_reads, signal, src_start, nullptr, 0, q2s, q2s_off, seq_len, dacs, dacs_cap, s2s, d_sig_off, d_seq_off,
                                  sig_off);
}

}  // extern "C"

// ---- chunk extraction ------------------------------------------------------------------------
namespace {

int read_offsets_host(rmr_engine *e, const rmr_reads *r, int mem, std::vector<int64_t> &sig_off,
                      std::vector<int64_t> &seq_off, std::vector<int64_t> &foc_off) {
    const size_t n1 = (size_t)r->n_reads + 1;
    const int64_t *given[3] = {r->sig_off, r->seq_off, r->focus_off}, *kept[3] = {r->host_sig_off, r->host_seq_off, r->host_focus_off};
    std::vector<int64_t> *out[3] = {&sig_off, &seq_off, &foc_off};
    // a device batch whose caller kept host copies of the offsets: three small device-to-host copies (and their syncs) saved per call
    const bool use_kept = mem != RMR_MEM_HOST && kept[0] && kept[1] && kept[2];
    for (int k = 0; k < 3; ++k) {
        out[k]->resize(n1);
        if (mem == RMR_MEM_HOST || use_kept) memcpy(out[k]->data(), use_kept ? kept[k] : given[k], n1 * 8);
        else RMR_HIP(hipMemcpy(out[k]->data(), given[k], n1 * 8, hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i + 1 < n1; ++i)
        if (sig_off[i + 1] < sig_off[i] || seq_off[i + 1] < seq_off[i] || foc_off[i + 1] < foc_off[i])
            RMR_FAIL(RMR_ERR_INVALID, "offsets of read %zu are not increasing", i);
    if (sig_off[0] != 0 || seq_off[0] != 0 || foc_off[0] != 0) RMR_FAIL(RMR_ERR_INVALID, "offsets must start at 0");
    return 0;
}

// the slots declare_reads (rmr_stage.h) declared, filled: the read index of every chunk and the arrays of a host batch
int upload_reads(rmr_engine *e, const rmr_reads *r, int mem, bool need_dacs, const std::vector<int64_t> &foc_off, DevReads *o) {
    const int64_t nr = r->n_reads;
    if (mem == RMR_MEM_DEVICE) {
        // device-resident batch: the read index of every chunk comes from the offsets where they are - no host loop, no
        // upload, no wait (a batch of the reads pipeline paid two of these round trips per extraction, each behind whatever
        // the GPU was running)
        return launch_chunk_read(e, r->focus_off, nr, o->n_chunks, o->chunk_read);
    }
    // read index per chunk (host-built, tiny next to the data itself)
    std::vector<int32_t> cr((size_t)o->n_chunks);
    for (int64_t k = 0; k < nr; ++k)
        for (int64_t i = foc_off[k]; i < foc_off[k + 1]; ++i) cr[(size_t)i] = (int32_t)k;
    H2D(o->chunk_read, cr.data(), cr.size() * 4);
#define RMR_UPLOAD(field, count) H2D((void *)o->d.field, r->field, (size_t)(count) * sizeof(*r->field));
    if (mem == RMR_MEM_HOST) {
        if (need_dacs) RMR_UPLOAD(dacs, o->total_sig)
        RMR_READ_ARRAYS(RMR_UPLOAD)
    }
#undef RMR_UPLOAD
    // the H2D copies above read from host vectors that die with this frame
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

// The groups of one rmr_duplex_align_mode call, in either mode: `bytes[k]` is what live[k] needs of the group's memory.  A job that
// needs more than the budget alone is set aside (`over`); the rest is sorted, largest first, and cut into groups of consecutive jobs
// that fit the budget together.  byte_off: a job's place in its group's memory; max_bytes: the largest group.
struct DuplexPlan {
    std::vector<DuplexJob> jobs;
    std::vector<int64_t> byte_off;
    std::vector<size_t> group_start;
    std::vector<int32_t> over;  // out_idx
    int64_t max_bytes = 0;
};

DuplexPlan plan_duplex_groups(const std::vector<DuplexJob> &live, const std::vector<int64_t> &bytes, int64_t budget) {
    DuplexPlan p;
    std::vector<size_t> order;
    for (size_t k = 0; k < live.size(); ++k) {
        if (bytes[k] > budget) p.over.push_back(live[k].out_idx);
        else order.push_back(k);
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return bytes[x] > bytes[y]; });
    p.group_start.push_back(0);
    int64_t used = 0;
    for (size_t k : order) {
        if (used > 0 && used + bytes[k] > budget) p.group_start.push_back(p.jobs.size()), used = 0;
        p.jobs.push_back(live[k]), p.byte_off.push_back(used);
        used += bytes[k];
        p.max_bytes = std::max(p.max_bytes, used);
    }
    p.group_start.push_back(p.jobs.size());
    return p;
}
}  // namespace

extern "C" {

int rmr_chunk_geometry(rmr_engine *e, const rmr_reads *reads, float *sig_out, int64_t *geo,
                       int64_t *max_seq_len, int mem) {
    if (!e || !reads || !sig_out || !geo || !max_seq_len) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (reads->n_reads < 0) RMR_FAIL(RMR_ERR_INVALID, "n_reads < 0");
    *max_seq_len = 0;
    if (reads->n_reads == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::vector<int64_t> so, qo, fo;
    RMR_TRY(read_offsets_host(e, reads, mem, so, qo, fo));
    const int64_t nr = reads->n_reads, ts = so[nr], tb = qo[nr], nc = fo[nr];
    Stage st;
    DevReads dr;
    int *dmax;
    float *dsig = sig_out;
    int64_t *dgeo = geo;
    declare_reads(st, reads, mem, true, ts, tb, nc, &dr);
    st.add(&dmax, 4);
    if (mem == RMR_MEM_HOST) {
        st.add(&dsig, ts + 1).add(&dgeo, nc * 6 + 1);
    }
    RMR_TRY(st.commit(e));
    RMR_TRY(upload_reads(e, reads, mem, true, fo, &dr));
    RMR_HIP(hipMemsetAsync(dmax, 0, 16, e->stream));
    RMR_TRY(launch_geometry(e, dr.d, nc, dr.chunk_read, dsig, ts, nullptr, dgeo, dmax));
    int hmax = 0;
    D2H(&hmax, dmax, 4);
    if (mem == RMR_MEM_HOST) {
        D2H(sig_out, dsig, (size_t)ts * 4);
        D2H(geo, dgeo, (size_t)nc * 48);
    }
    RMR_HIP(hipStreamSynchronize(e->stream));
    *max_seq_len = hmax;
    return 0;
}

int rmr_chunk_fill(rmr_engine *e, const rmr_reads *reads, const float *sig, const int64_t *geo,
                   float *signal, int8_t *seqs, int seq_w, int16_t *maps, int map_w, int16_t *lens,
                   int64_t *read_focus_bases, int mem) {
    if (!e || !reads || !sig || !geo || !signal || !seqs || !maps || !lens || !read_focus_bases)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (reads->n_reads <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::vector<int64_t> so, qo, fo;
    RMR_TRY(read_offsets_host(e, reads, mem, so, qo, fo));
    const int64_t nr = reads->n_reads, ts = so[nr], tb = qo[nr], nc = fo[nr];
    if (nc == 0) return 0;
    const int L = reads->cc_before + reads->cc_after;
    Stage st;
    DevReads dr;
    float *dsig;
    int64_t *dgeo;
    ChunkSlots c;
    declare_reads(st, reads, mem, false, ts, tb, nc, &dr);
    if (mem != RMR_MEM_DEVICE) {
        st.add(&dsig, ts + 1).add(&dgeo, nc * 6);
        c.declare(st, nc, L, seq_w, map_w);
    }
    RMR_TRY(st.commit(e));
    RMR_TRY(upload_reads(e, reads, mem, false, fo, &dr));
    if (mem == RMR_MEM_DEVICE) return launch_fill(e, dr.d, nc, dr.chunk_read, sig, geo, signal, seqs, seq_w, maps, map_w, lens, read_focus_bases);
    H2D(dsig, sig, (size_t)ts * 4);
    H2D(dgeo, geo, (size_t)nc * 48);
    RMR_TRY(launch_fill(e, dr.d, nc, dr.chunk_read, dsig, dgeo, c.signal, c.seqs, seq_w, c.maps, map_w, c.lens, c.rfb));
    D2H(signal, c.signal, (size_t)nc * L * 4);
    D2H(seqs, c.seqs, (size_t)nc * seq_w);
    D2H(maps, c.maps, (size_t)nc * map_w * 2);
    D2H(lens, c.lens, (size_t)nc * 2);
    D2H(read_focus_bases, c.rfb, (size_t)nc * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_count_labels(rmr_engine *e, const float *logits, int64_t n, int num_out, int64_t *counts,
                     int mem) {
    if (!e || !logits || !counts) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (num_out < 1 || num_out > 16) RMR_FAIL(RMR_ERR_INVALID, "num_out %d not in [1,16]", num_out);
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (mem == RMR_MEM_DEVICE) return launch_count(e, logits, n, num_out, counts);
    Stage st;
    float *dl;
    int64_t *dc;
    st.add(&dl, (size_t)n * num_out).add(&dc, 16);
    RMR_TRY(st.commit(e));
    H2D(dl, logits, (size_t)n * num_out * 4);
    H2D(dc, counts, (size_t)num_out * 8);
    RMR_TRY(launch_count(e, dl, n, num_out, dc));
    D2H(counts, dc, (size_t)num_out * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_validation_tally(rmr_engine *e, const float *logits, const int64_t *labels, int64_t n, int num_out, int num_labels,
                         const int32_t *label_of_column, int64_t *confusion, float *win_prob, uint8_t *call, double *loss_sum) {
    if (!e || !logits || !labels || !label_of_column || !confusion || !win_prob || !call || !loss_sum)
        RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (num_out < 1 || num_out > 16 || num_labels < num_out || num_labels > 16)
        RMR_FAIL(RMR_ERR_INVALID, "num_out %d / num_labels %d not in [1,16], num_labels >= num_out", num_out, num_labels);
    for (int c = 0; c < num_labels; ++c)
        if (label_of_column[c] < -1 || label_of_column[c] >= num_out) RMR_FAIL(RMR_ERR_INVALID, "label_of_column[%d] = %d", c, label_of_column[c]);
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_validation_tally(e, logits, labels, n, num_out, num_labels, label_of_column, confusion, win_prob, call, loss_sum);
}

static int check_motifs(const rmr_motif_set *motifs) {
    if (motifs->n_motifs < 1 || motifs->n_motifs > 8) RMR_FAIL(RMR_ERR_INVALID, "1..8 motifs supported");
    for (int m = 0; m < motifs->n_motifs; ++m)
        if (motifs->len[m] < 1 || motifs->len[m] > 16 || motifs->focus_pos[m] >= motifs->len[m] || motifs->focus_pos[m] < -64)
            RMR_FAIL(RMR_ERR_INVALID, "motif %d: length %d / focus %d unsupported", m, motifs->len[m], motifs->focus_pos[m]);
    return 0;
}

int rmr_motif_focus_counts(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads, const rmr_motif_set *motifs,
                           int64_t *counts) {
    if (!e || !int_seq || !seq_off || !motifs || !counts) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads");
    RMR_TRY(check_motifs(motifs));
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_motif_focus(e, int_seq, seq_off, (int)n_reads, *motifs, counts, nullptr, nullptr);
}

int rmr_motif_focus_fill(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads, const rmr_motif_set *motifs,
                         const int64_t *foc_off, int64_t *focus) {
    if (!e || !int_seq || !seq_off || !motifs || !foc_off || !focus) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads");
    RMR_TRY(check_motifs(motifs));
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_motif_focus(e, int_seq, seq_off, (int)n_reads, *motifs, nullptr, foc_off, focus);
}

int rmr_motif_flags(rmr_engine *e, const int8_t *int_seq, const int64_t *seq_off, int64_t n_reads,
                    const rmr_motif_set *motifs, uint8_t *flags, int mem) {
    if (!e || !int_seq || !seq_off || !motifs || !flags) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_reads < 0 || n_reads > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_reads");
    RMR_TRY(check_motifs(motifs));
    if (n_reads == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    int64_t total = 0;
    if (mem == RMR_MEM_HOST) total = seq_off[n_reads];
    else RMR_HIP(hipMemcpy(&total, seq_off + n_reads, 8, hipMemcpyDeviceToHost));
    if (total <= 0) return 0;
    if (mem == RMR_MEM_DEVICE) return launch_motif(e, int_seq, seq_off, (int)n_reads, total, *motifs, flags);
    Stage st;
    int8_t *ds;
    int64_t *d_off;
    uint8_t *df;
    st.add(&ds, total).add(&d_off, n_reads + 1).add(&df, total);
    RMR_TRY(st.commit(e));
    H2D(ds, int_seq, (size_t)total);
    H2D(d_off, seq_off, (size_t)(n_reads + 1) * 8);
    RMR_TRY(launch_motif(e, ds, d_off, (int)n_reads, total, *motifs, df));
    D2H(flags, df, (size_t)total);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

static int check_modbam_batch(const rmr_modbam_batch *b) {
    if (b->n_records < 0 || b->n_records > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_records");
    if (b->n_mods < 1 || b->n_mods > 7) RMR_FAIL(RMR_ERR_INVALID, "1..7 modified-base codes supported, got %d", b->n_mods);
    if (b->n_refs < 0 || b->n_deltas < 0 || b->n_ml < 0) RMR_FAIL(RMR_ERR_INVALID, "bad sizes");
    if (b->n_records > 0 && (!b->seq_off || !b->cigar_off || !b->flag || !b->ref_id || !b->pos || !b->has || !b->tok_status || !b->ent_off ||
                             !b->truth_off))
        RMR_FAIL(RMR_ERR_INVALID, "NULL array in the batch");
    return 0;
}

int rmr_vbz_decode(rmr_engine *e, const uint8_t *svb, const int64_t *row_off, const int32_t *row_samples,
                   int64_t n_rows, int16_t *out, int mem) {
    if (!e || !svb || !row_off || !row_samples || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_rows < 0 || n_rows > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_rows");
    if (n_rows == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    std::vector<int64_t> ro((size_t)n_rows + 1), oo((size_t)n_rows + 1);
    std::vector<int32_t> rn((size_t)n_rows);
    if (mem == RMR_MEM_HOST) {
        memcpy(ro.data(), row_off, ro.size() * 8);
        memcpy(rn.data(), row_samples, rn.size() * 4);
    } else {
        RMR_HIP(hipMemcpy(ro.data(), row_off, ro.size() * 8, hipMemcpyDeviceToHost));
        RMR_HIP(hipMemcpy(rn.data(), row_samples, rn.size() * 4, hipMemcpyDeviceToHost));
    }
    oo[0] = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        // (a row without samples has no bytes: the kernel's waves leave such rows before they look at them)
        if (rn[r] < 0 || ro[r + 1] < ro[r] || ro[r + 1] - ro[r] < ((int64_t)rn[r] + 7) / 8 + rn[r] || (rn[r] == 0 && ro[r + 1] != ro[r]))
            RMR_FAIL(RMR_ERR_INVALID, "corrupt VBZ signal block (row %lld)", (long long)r);
        oo[r + 1] = oo[r] + rn[r];
    }
    const int64_t nbytes = ro[n_rows], nout = oo[n_rows];
    Stage st;
    int64_t *d_oo;
    int32_t *d_st;
    const uint8_t *d_svb = svb;
    const int64_t *d_ro = row_off;
    const int32_t *d_rn = row_samples;
    int16_t *d_out = out;
    st.add(&d_oo, n_rows + 1).add(&d_st, n_rows);
    if (mem == RMR_MEM_HOST) st.add(&d_svb, nbytes + 16).add(&d_ro, n_rows + 1).add(&d_rn, n_rows).add(&d_out, nout + 8);
    RMR_TRY(st.commit(e));
    H2D(d_oo, oo.data(), oo.size() * 8);
    RMR_HIP(hipMemsetAsync(d_st, 0, (size_t)n_rows * 4, e->stream));
    if (mem == RMR_MEM_HOST) {
        H2D((void *)d_svb, svb, (size_t)nbytes);
        H2D((void *)d_ro, row_off, ro.size() * 8);
        H2D((void *)d_rn, row_samples, rn.size() * 4);
    }
    RMR_TRY(launch_vbz(e, d_svb, d_ro, d_rn, d_oo, n_rows, d_out, d_st));
    std::vector<int32_t> hst((size_t)n_rows);
    D2H(hst.data(), d_st, (size_t)n_rows * 4);
    if (mem == RMR_MEM_HOST) D2H(out, d_out, (size_t)nout * 2);
    RMR_HIP(hipStreamSynchronize(e->stream));
    for (int64_t r = 0; r < n_rows; ++r)
        if (hst[r]) RMR_FAIL(RMR_ERR_INVALID, "corrupt VBZ signal block (row %lld)", (long long)r);
    return 0;
}

int rmr_modbam_site_counts(rmr_engine *e, const rmr_modbam_batch *b, int32_t *ords, int64_t *cig_q, int64_t *cig_r, int64_t *counts,
                           int32_t *status) {
    if (!e || !b || !counts || !status) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    RMR_TRY(check_modbam_batch(b));
    if ((b->n_deltas > 0 && !ords) || !cig_q || !cig_r) RMR_FAIL(RMR_ERR_INVALID, "NULL workspace");
    if (b->n_records == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_modbam_sites(e, *b, ords, cig_q, cig_r, counts, status, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int rmr_modbam_site_fill(rmr_engine *e, const rmr_modbam_batch *b, const int32_t *ords, const int64_t *cig_q, const int64_t *cig_r,
                         const int32_t *status, const int64_t *out_off, float *probs, uint8_t *label, int64_t *qpos, int64_t *rpos) {
    if (!e || !b || !status || !out_off || !probs || !label || !qpos || !rpos) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    RMR_TRY(check_modbam_batch(b));
    if ((b->n_deltas > 0 && !ords) || !cig_q || !cig_r) RMR_FAIL(RMR_ERR_INVALID, "NULL workspace");
    if (b->n_records == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_modbam_sites(e, *b, const_cast<int32_t *>(ords), const_cast<int64_t *>(cig_q), const_cast<int64_t *>(cig_r), nullptr,
                               const_cast<int32_t *>(status), out_off, probs, label, qpos, rpos);
}

int rmr_duplex_align(rmr_engine *e, int64_t n, const uint8_t *bases, const int64_t *q_off, const int64_t *q_len, const int64_t *r_off,
                     const int64_t *r_len, int64_t trace_budget, int32_t *out, const int64_t *run_off, uint32_t *runs,
                     int64_t *n_groups) {
    return rmr_duplex_align_mode(e, n, bases, q_off, q_len, r_off, r_len, trace_budget, RMR_DUPLEX_MODE_FULL, out, run_off, runs, n_groups,
                                 nullptr);
}

int rmr_duplex_align_mode(rmr_engine *e, int64_t n, const uint8_t *bases, const int64_t *q_off, const int64_t *q_len, const int64_t *r_off,
                          const int64_t *r_len, int64_t trace_budget, int mode, int32_t *out, const int64_t *run_off, uint32_t *runs,
                          int64_t *n_groups, int64_t *n_checkpointed) {
    if (n_groups) *n_groups = 0;
    if (n_checkpointed) *n_checkpointed = 0;
    if (!e || n < 0) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    if (mode != RMR_DUPLEX_MODE_FULL && mode != RMR_DUPLEX_MODE_CHECKPOINT && mode != RMR_DUPLEX_MODE_AUTO)
        RMR_FAIL(RMR_ERR_INVALID, "unknown duplex alignment mode %d", mode);
    if (n == 0) return 0;
    if (!bases || !q_off || !q_len || !r_off || !r_len || !out || !run_off || !runs) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n > INT32_MAX) RMR_FAIL(RMR_ERR_INVALID, "too many alignments");
    const int64_t budget = trace_budget > 0 ? trace_budget : RMR_DUPLEX_DEFAULT_TRACE_BYTES;
    // what does not reach the GPU gets its status here
    std::vector<int32_t> hout((size_t)n * RMR_DUPLEX_OUT_FIELDS, 0);
    std::vector<DuplexJob> live;
    int64_t n_bases = 0;
    if (run_off[0] < 0) RMR_FAIL(RMR_ERR_INVALID, "run_off is negative");
    for (int64_t a = 0; a < n; ++a) {
        const int64_t nq = q_len[a], nr = r_len[a];
        if (nq < 0 || nr < 0 || q_off[a] < 0 || r_off[a] < 0) RMR_FAIL(RMR_ERR_INVALID, "negative offset or length (alignment %lld)", (long long)a);
        if (run_off[a + 1] - run_off[a] < 2 * nr + 2)
            RMR_FAIL(RMR_ERR_INVALID, "run_off leaves alignment %lld fewer than 2 r_len + 2 words", (long long)a);
        n_bases = std::max(n_bases, std::max(q_off[a] + nq, r_off[a] + nr));
        int32_t *o = &hout[(size_t)a * RMR_DUPLEX_OUT_FIELDS];
        if (nq == 0 || nr == 0) {
            o[0] = RMR_DUPLEX_EMPTY;
            continue;
        }
        bool ok = true;
        for (int side = 0; side < 2 && ok; ++side) {
            const uint8_t *p = bases + (side ? r_off[a] : q_off[a]);
            for (int64_t i = 0, k = side ? nr : nq; i < k && ok; ++i)
                ok = p[i] == 'A' || p[i] == 'C' || p[i] == 'G' || p[i] == 'T' || p[i] == 'N';
        }
        if (!ok) {
            o[0] = RMR_DUPLEX_BAD_BASE;
            continue;
        }
        if (nq > (1 << 30) || nr > (1 << 30)) {  // fits no budget; below 2^30 every product here stays far inside int64
            o[0] = RMR_DUPLEX_OVER_BUDGET;
            continue;
        }
        DuplexJob j{};
        j.q_off = q_off[a], j.r_off = r_off[a], j.run_off = run_off[a];
        j.n = (int32_t)nq, j.m = (int32_t)nr, j.out_idx = (int32_t)a;
        live.push_back(j);
    }
    // bytes of trace (FULL) or of lines and one strip of trace (CHECKPOINT) of a job: include/remora_hip.h
    auto strips_of = [](const DuplexJob &j) { return ((int64_t)j.n + RMR_DUPLEX_STRIP_ROWS - 1) / RMR_DUPLEX_STRIP_ROWS; };
    auto trace_bytes = [&](const DuplexJob &j) { return strips_of(j) * ((int64_t)j.m + 63) * 256; };
    auto line_bytes = [&](const DuplexJob &j) { return strips_of(j) * (int64_t)j.m * 8; };
    bool ckpt = mode == RMR_DUPLEX_MODE_CHECKPOINT;
    if (mode == RMR_DUPLEX_MODE_AUTO) {  // FULL where that is one group with nothing over the budget
        int64_t left = budget;
        for (size_t k = 0; k < live.size() && !ckpt; ++k) ckpt = trace_bytes(live[k]) > left, left -= trace_bytes(live[k]);
    }
    std::vector<int64_t> bytes;
    for (const DuplexJob &j : live) bytes.push_back(ckpt ? line_bytes(j) + ((int64_t)j.m + 63) * 256 : trace_bytes(j));
    DuplexPlan plan = plan_duplex_groups(live, bytes, budget);
    for (int32_t a : plan.over) hout[(size_t)a * RMR_DUPLEX_OUT_FIELDS] = RMR_DUPLEX_OVER_BUDGET;
    std::vector<DuplexJob> &jobs = plan.jobs;
    if (jobs.empty()) {
        memcpy(out, hout.data(), hout.size() * 4);
        return 0;
    }
    // FULL: the group's memory is trace, the one line of every job lies in the staging arena.  CHECKPOINT: a job's share of the
    // group's memory is its lines, then its strip of trace
    int64_t line_total = 0;
    for (size_t k = 0; k < jobs.size(); ++k) {
        if (ckpt) {
            jobs[k].line_off = plan.byte_off[k] / 8, jobs[k].trace_off = (plan.byte_off[k] + line_bytes(jobs[k])) / 4;
        } else {
            jobs[k].trace_off = plan.byte_off[k] / 4, jobs[k].line_off = line_total;
            line_total += jobs[k].m;
        }
    }
    const std::vector<size_t> &group_start = plan.group_start;

    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    Stage st;
    uint8_t *d_bases;
    DuplexJob *d_jobs;
    int2 *d_line, *d_best;
    uint32_t *d_runs;
    int32_t *d_out;
    st.add(&d_bases, n_bases).add(&d_jobs, jobs.size()).add(&d_line, line_total).add(&d_best, jobs.size()).add(&d_runs, run_off[n])
        .add(&d_out, hout.size());
    RMR_TRY(st.commit(e));
    uint32_t *d_trace = nullptr;
    if (hipMalloc(&d_trace, (size_t)plan.max_bytes) != hipSuccess) {
        (void)hipGetLastError();
        RMR_FAIL(RMR_ERR_HIP, "cannot allocate %lld bytes of alignment trace (lower the trace budget)", (long long)plan.max_bytes);
    }
    auto run = [&]() -> int {
        H2D(d_bases, bases, (size_t)n_bases);
        H2D(d_jobs, jobs.data(), jobs.size() * sizeof(DuplexJob));
        H2D(d_out, hout.data(), hout.size() * 4);
        for (size_t g = 0; g + 1 < group_start.size(); ++g) {
            const size_t k0 = group_start[g];
            const int cnt = (int)(group_start[g + 1] - k0);
            if (ckpt) RMR_TRY(launch_duplex_group_checkpoint(e, d_jobs + k0, cnt, d_bases, d_trace, (int2 *)d_trace, d_best + k0, d_runs, d_out));
            else RMR_TRY(launch_duplex_group(e, d_jobs + k0, cnt, d_bases, d_trace, d_line, d_best + k0, d_runs, d_out));
        }
        D2H(out, d_out, hout.size() * 4);
        D2H(runs, d_runs, (size_t)run_off[n] * 4);
        RMR_HIP(hipStreamSynchronize(e->stream));
        return 0;
    };
    const int rc = run();
    if (rc != 0) (void)hipStreamSynchronize(e->stream);  // nothing may still write the trace when it is freed
    (void)hipFree(d_trace);
    if (rc == 0 && n_groups) *n_groups = (int64_t)group_start.size() - 1;
    if (rc == 0 && n_checkpointed) *n_checkpointed = ckpt ? (int64_t)jobs.size() : 0;
    return rc;
}

int rmr_read_index_create(rmr_engine *e, const uint8_t *keys, const int64_t *values, int64_t n, rmr_read_index **out, int64_t *n_distinct) {
    if (out) *out = nullptr;
    if (n_distinct) *n_distinct = 0;
    if (!e || !out || n < 0 || (n > 0 && (!keys || !values))) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    if (n > (int64_t)INT32_MAX)  // the permutation the sorts carry is 32 bits wide
        RMR_FAIL(RMR_ERR_INVALID, "a read-id index holds up to %lld reads, got %lld (which would need about %lld bytes of device memory to build)",
                 (long long)INT32_MAX, (long long)n, (long long)n * 80);
    rmr_read_index *ix = new (std::nothrow) rmr_read_index();
    if (!ix) RMR_FAIL(RMR_ERR_NOMEM, "out of host memory");
    ix->eng = e;
    if (n > 0) {
        std::lock_guard<std::mutex> lk(e->mu);
        int rc = hipSetDevice(e->device) == hipSuccess ? 0 : RMR_ERR_HIP;
        if (rc != 0) set_error("hipSetDevice(%d) failed", e->device);
        if (rc == 0) rc = read_index_build(e, keys, values, n, ix);
        if (rc != 0) {
            (void)hipStreamSynchronize(e->stream);  // nothing may still write the temporaries or the table when they are freed
            if (ix->mem) (void)hipFree(ix->mem);
            delete ix;
            return rc;
        }
    }
    *out = ix;
    if (n_distinct) *n_distinct = ix->n;
    return 0;
}

int rmr_read_index_lookup(rmr_read_index *ix, const char *names, const int64_t *name_off, int64_t m, int64_t *values_out) {
    if (!ix || !ix->eng || m < 0) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    if (m == 0) return 0;
    if (!name_off || !values_out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (m > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad m");
    const int64_t base = name_off[0], total = name_off[m] - base;
    for (int64_t i = 0; i < m; ++i)
        if (name_off[i + 1] < name_off[i]) RMR_FAIL(RMR_ERR_INVALID, "name_off is not ascending (name %lld)", (long long)i);
    if (total > 0 && !names) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (ix->n == 0 || total == 0) {  // nothing can be found: no launch
        std::fill(values_out, values_out + m, (int64_t)-1);
        return 0;
    }
    rmr_engine *e = ix->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    Stage st;
    char *d_names;
    int64_t *d_off, *d_out;
    st.add(&d_names, total).add(&d_off, m + 1).add(&d_out, m);
    RMR_TRY(st.commit(e));
    H2D(d_names, names + base, (size_t)total);
    H2D(d_off, name_off, (size_t)(m + 1) * 8);
    RMR_TRY(launch_read_index_lookup(e, ix, d_names, d_off, base, m, d_out));
    D2H(values_out, d_out, (size_t)m * 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

void rmr_read_index_destroy(rmr_read_index *ix) {
    if (!ix) return;
    if (ix->mem) {
        (void)hipSetDevice(ix->eng->device);
        (void)hipFree(ix->mem);
    }
    delete ix;
}

}  // extern "C"
