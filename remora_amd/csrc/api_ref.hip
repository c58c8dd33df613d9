// api_ref.hip — the reference genome entry points of the C ABI (rmr_ref_genome_*: the table, its load from FASTA text piece
// by piece through k_ref_genome.hip, the read-back).  The emit that reads it is api_pileup.hip's rmr_pileup_emit_counts / _fill.
#include <algorithm>
#include <new>

#include "rmr_internal.h"
#include "rmr_ref_pack.h"
#include "rmr_stage.h"

using namespace rmr;

namespace {

constexpr int64_t DEFAULT_PIECE_BYTES = (int64_t)64 << 20;

}  // namespace

extern "C" {

int rmr_ref_genome_create(rmr_engine *e, int64_t n_contigs, const int64_t *lens, rmr_ref_genome **out, int64_t *device_bytes) {
    if (out) *out = nullptr;
    if (!e || !out || !lens) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_contigs < 1 || n_contigs > RMR_PILEUP_MAX_CONTIGS)
        RMR_FAIL(RMR_ERR_INVALID, "a reference genome holds 1 to %lld contigs, got %lld", (long long)RMR_PILEUP_MAX_CONTIGS, (long long)n_contigs);
    rmr_ref_genome *g = new (std::nothrow) rmr_ref_genome();
    if (!g) RMR_FAIL(RMR_ERR_NOMEM, "out of host memory");
    g->eng = e, g->n_contigs = n_contigs;
    g->h_off.resize((size_t)n_contigs), g->h_len.resize((size_t)n_contigs);
    int64_t at = 0;
    for (int64_t c = 0; c < n_contigs; ++c) {
        if (lens[c] < 0 || lens[c] > RMR_PILEUP_MAX_POS) {
            delete g;
            RMR_FAIL(RMR_ERR_INVALID, "contig #%lld: a length of 0 to %lld bases, got %lld", (long long)c, (long long)RMR_PILEUP_MAX_POS, (long long)lens[c]);
        }
        g->h_off[(size_t)c] = at, g->h_len[(size_t)c] = lens[c];
        at += (lens[c] + 1) / 2;
    }
    Stage st;  // (for its layout only)
    st.add(&g->data, (size_t)at + 1).add(&g->d_off, (size_t)n_contigs).add(&g->d_len, (size_t)n_contigs).add(&g->first_bad, 1);
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = hipSetDevice(e->device) == hipSuccess ? 0 : RMR_ERR_HIP;
    if (rc != 0) set_error("hipSetDevice(%d) failed", e->device);
    if (rc == 0 && hipMalloc(&g->mem, st.total) != hipSuccess) {
        (void)hipGetLastError();
        g->mem = nullptr;
        set_error("a reference genome of %lld contigs needs %zu bytes of device memory and they could not be allocated", (long long)n_contigs, st.total);
        rc = RMR_ERR_NOMEM;
    }
    if (rc == 0) {
        for (const Stage::Slot &s : st.slots) s.set(s.where, static_cast<char *>(g->mem) + s.off);
        g->bytes = st.total;
        const bool ok = hipMemsetAsync(g->data, 0, (size_t)at + 1, e->stream) == hipSuccess &&
                        hipMemcpyAsync(g->d_off, g->h_off.data(), (size_t)n_contigs * 8, hipMemcpyHostToDevice, e->stream) == hipSuccess &&
                        hipMemcpyAsync(g->d_len, g->h_len.data(), (size_t)n_contigs * 8, hipMemcpyHostToDevice, e->stream) == hipSuccess &&
                        hipStreamSynchronize(e->stream) == hipSuccess;
        if (!ok) set_error("HIP error %s while the reference genome was set up", hipGetErrorString(hipGetLastError())), rc = RMR_ERR_HIP;
    }
    if (rc != 0) {
        if (g->mem) (void)hipFree(g->mem);
        delete g;
        return rc;
    }
    if (device_bytes) *device_bytes = (int64_t)g->bytes;
    *out = g;
    return 0;
}

int rmr_ref_genome_load(rmr_ref_genome *g, int64_t contig, const uint8_t *text, int64_t text_bytes, int64_t line_bases, int64_t line_width,
                        int64_t piece_bytes, int64_t *bad_offset) {
    if (bad_offset) *bad_offset = -1;
    if (!g || !g->eng || (text_bytes > 0 && !text)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (contig < 0 || contig >= g->n_contigs) RMR_FAIL(RMR_ERR_INVALID, "contig #%lld of %lld", (long long)contig, (long long)g->n_contigs);
    const int64_t lb = line_bases, W = line_width, S = text_bytes, len = g->h_len[(size_t)contig];
    if (lb < 1 || (W - lb != 1 && W - lb != 2) || S < 0)
        RMR_FAIL(RMR_ERR_INVALID, "lines of line_bases >= 1 bases and one or two terminator bytes, got line_bases %lld, line_width %lld", (long long)lb,
                 (long long)W);
    const int64_t held = ref_bases_of_text(S, lb, W);
    if (held != len)
        RMR_FAIL(RMR_ERR_INVALID, "contig #%lld: %lld bytes of text in lines of %lld bases hold %lld bases, the table was made for %lld", (long long)contig,
                 (long long)S, (long long)lb, (long long)held, (long long)len);
    if (piece_bytes == 0) piece_bytes = DEFAULT_PIECE_BYTES;
    if (piece_bytes < 16) RMR_FAIL(RMR_ERR_INVALID, "piece_bytes is at least 16, got %lld", (long long)piece_bytes);
    if (len == 0) return 0;
    rmr_engine *e = g->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    uint8_t *buf = nullptr;
    const size_t buf_bytes = (size_t)std::min(piece_bytes, S);
    if (hipMalloc(&buf, buf_bytes) != hipSuccess) {
        (void)hipGetLastError();
        RMR_FAIL(RMR_ERR_NOMEM, "a FASTA piece of %zu bytes could not be allocated on the device (lower piece_bytes)", buf_bytes);
    }
    const unsigned long long none = ~0ull;
    unsigned long long first = none;
    int rc = 0;
    const auto step = [&](hipError_t err) {
        if (err != hipSuccess && rc == 0) set_error("HIP error %s while contig #%lld was loaded", hipGetErrorString(err), (long long)contig), rc = RMR_ERR_HIP;
        return rc == 0;
    };
    step(hipMemcpyAsync(g->first_bad, &none, 8, hipMemcpyHostToDevice, e->stream));
    for (int64_t i0 = 0; i0 < len && rc == 0;) {
        int64_t t_lo = 0, t_n = 0;
        const int64_t nb = ref_next_piece(i0, len, lb, W, S, piece_bytes, &t_lo, &t_n);
        if (t_n < 1 || (size_t)t_n > buf_bytes || t_lo + t_n > S) {  // (by the arithmetic above: never true)
            set_error("contig #%lld: a piece of %lld bytes at %lld does not fit", (long long)contig, (long long)t_n, (long long)t_lo), rc = RMR_ERR_INVALID;
            break;
        }
        if (!step(hipMemcpyAsync(buf, text + t_lo, (size_t)t_n, hipMemcpyHostToDevice, e->stream))) break;
        rc = launch_ref_pack(e, buf, t_lo, t_n, S, i0, i0 + nb, lb, W, g->data + g->h_off[(size_t)contig] + i0 / 2, g->first_bad);
        i0 += nb;
    }
    if (rc == 0) step(hipMemcpyAsync(&first, g->first_bad, 8, hipMemcpyDeviceToHost, e->stream));
    const hipError_t done = hipStreamSynchronize(e->stream);  // the piece buffer goes when nothing reads it any more
    (void)hipFree(buf);
    if (rc != 0) return rc;
    if (!step(done)) return rc;
    if (first != none) {
        if (bad_offset) *bad_offset = (int64_t)first;
        const int64_t col = (int64_t)first % W;
        RMR_FAIL(RMR_ERR_INVALID, "contig #%lld, sequence line %lld: %s at column %lld (byte %lld of the contig's text); lines of %lld bases were expected",
                 (long long)contig, (long long)(first / W) + 1, col < lb ? "not an IUPAC letter" : "not the line terminator", (long long)col + 1,
                 (long long)first, (long long)lb);
    }
    return 0;
}

int rmr_ref_genome_read(rmr_ref_genome *g, int64_t contig, int64_t lo, int64_t hi, uint8_t *codes) {
    if (!g || !g->eng) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (contig < 0 || contig >= g->n_contigs) RMR_FAIL(RMR_ERR_INVALID, "contig #%lld of %lld", (long long)contig, (long long)g->n_contigs);
    if (lo < 0 || hi < lo || hi > g->h_len[(size_t)contig])
        RMR_FAIL(RMR_ERR_INVALID, "bases [%lld, %lld) of a contig of %lld", (long long)lo, (long long)hi, (long long)g->h_len[(size_t)contig]);
    if (hi == lo) return 0;
    if (!codes) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    rmr_engine *e = g->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    Stage st;
    uint8_t *d_codes;
    st.add(&d_codes, (size_t)(hi - lo));
    RMR_TRY(st.commit(e));
    RMR_TRY(launch_ref_unpack(e, g, contig, lo, hi, d_codes));
    D2H(codes, d_codes, (size_t)(hi - lo));
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

void rmr_ref_genome_destroy(rmr_ref_genome *g) {
    if (!g) return;
    (void)hipSetDevice(g->eng->device);
    (void)hipStreamSynchronize(g->eng->stream);  // nothing may still read the table when it is freed
    if (g->mem) (void)hipFree(g->mem);
    delete g;
}

}  // extern "C"
