// api_pileup.hip — the host entry points of `analyze pileup_modbams`: the emit (one pair of entries, every mode an option), the
// strand pairs of a hemi run, the per-site table, the partition stamp and the coverage join.  Everything is checked here and
// refused before a launch; the kernels and their launchers are k_pileup.hip, k_ref_genome.hip and k_pileup_duplex.hip.  No
// device code in this file.
#include <algorithm>
#include <cstring>
#include <new>

#include "rmr_internal.h"
#include "rmr_stage.h"

using namespace rmr;

static int check_call_batch(const rmr_modbam_batch *b, int32_t region_ref, int64_t region_lo, int64_t region_hi) {
    if (b->n_records < 0 || b->n_records > (int64_t)1 << 30) RMR_FAIL(RMR_ERR_INVALID, "bad n_records");
    if (b->n_mods < 1 || b->n_mods > 7) RMR_FAIL(RMR_ERR_INVALID, "1..7 modified-base codes supported, got %d", b->n_mods);
    if (b->n_deltas < 0 || b->n_ml < 0) RMR_FAIL(RMR_ERR_INVALID, "bad sizes");
    if (b->n_refs < 1 || b->n_refs > RMR_PILEUP_MAX_CONTIGS)
        RMR_FAIL(RMR_ERR_INVALID, "a site word holds up to %lld contigs, got %lld", (long long)RMR_PILEUP_MAX_CONTIGS, (long long)b->n_refs);
    if (b->n_records > 0 && (!b->seq_off || !b->cigar_off || !b->flag || !b->ref_id || !b->pos || !b->tok_status || !b->ent_off))
        RMR_FAIL(RMR_ERR_INVALID, "NULL array in the batch");
    if (region_ref >= 0 && (region_ref >= b->n_refs || region_lo < 0 || region_hi < region_lo)) RMR_FAIL(RMR_ERR_INVALID, "bad region");
    return 0;
}

static int reverse4(int c) { return ((c & 1) << 3) | ((c & 2) << 1) | ((c & 4) >> 1) | ((c & 8) >> 3); }

// the reference part of an emit from the caller's struct, everything checked
static int fill_ref_part(rmr_engine *e, const rmr_modbam_batch *b, const rmr_pileup_ref *ref, PileupRef *pr) {
    const rmr_ref_genome *g = ref->genome;
    if (!g || !g->data) RMR_FAIL(RMR_ERR_INVALID, "rmr_pileup_ref without a genome");
    if (g->eng != e) RMR_FAIL(RMR_ERR_INVALID, "the reference genome belongs to another engine");
    if (g->n_contigs < b->n_refs)
        RMR_FAIL(RMR_ERR_INVALID, "the reference genome holds %lld contigs, the batch names %lld", (long long)g->n_contigs, (long long)b->n_refs);
    if (ref->n_motifs < 1 || ref->n_motifs > RMR_PILEUP_MAX_MOTIFS)
        RMR_FAIL(RMR_ERR_INVALID, "1 to %d motifs, got %d", RMR_PILEUP_MAX_MOTIFS, ref->n_motifs);
    for (int j = 0; j < ref->n_motifs; ++j) {
        const rmr_pileup_motif &m = ref->motifs[j];
        if (m.len < 1 || m.len > RMR_PILEUP_MAX_MOTIF_LEN || m.focus < 0 || m.focus >= m.len)
            RMR_FAIL(RMR_ERR_INVALID, "motif #%d: a length of 1 to %d and a focus inside it, got %d and %d", j, RMR_PILEUP_MAX_MOTIF_LEN, m.len, m.focus);
        for (int i = 0; i < RMR_PILEUP_MAX_MOTIF_LEN; ++i) {
            const int c = (int)(m.mask >> (4 * i)) & 15, rc = (int)(m.rc_mask >> (4 * i)) & 15;
            if (i >= m.len ? (c != 0 || rc != 0) : (c == 0 || rc != reverse4((int)(m.mask >> (4 * (m.len - 1 - i))) & 15)))
                RMR_FAIL(RMR_ERR_INVALID, "motif #%d: nibble %d of mask / rc_mask is not a motif of %d bases and its reverse complement", j, i, m.len);
        }
        if (ref->combine && m.mask != m.rc_mask)
            RMR_FAIL(RMR_ERR_INVALID, "motif #%d is not its own reverse complement: its strands cannot be combined", j);
        pr->motifs[j] = m;
    }
    pr->data = g->data, pr->off = g->d_off, pr->len = g->d_len;
    pr->n_motifs = ref->n_motifs, pr->combine = ref->combine ? 1 : 0;
    return 0;
}

// Both passes of the emit.  The count pass (out_off == NULL) writes counts and, when given, hist; the fill pass writes words at
// out_off and takes k_t.  The options pick one of the three launchers; hemi travels to the kernel as combine == 2.
static int pileup_emit(rmr_engine *e, const rmr_modbam_batch *b, const rmr_pileup_emit_opts *opt, int32_t k_t, int32_t *ords, int64_t *cig_q,
                       int64_t *cig_r, int64_t *counts, int32_t *status, uint64_t *hist, const int64_t *out_off, uint64_t *words) {
    RMR_TRY(check_call_batch(b, opt->region_ref, opt->region_lo, opt->region_hi));
    if ((b->n_deltas > 0 && !ords) || !cig_q || !cig_r) RMR_FAIL(RMR_ERR_INVALID, "NULL workspace");
    if (k_t < 0 || k_t > RMR_PILEUP_BINS) RMR_FAIL(RMR_ERR_INVALID, "the threshold is 0 .. %d in units of 1/512, got %d", RMR_PILEUP_BINS, k_t);
    const rmr_pileup_ref *ref = opt->ref;
    if (opt->hemi != 0) {
        if (opt->duplex == 0) RMR_FAIL(RMR_ERR_INVALID, "the hemi mode of the emit pairs the calls of both strands: duplex must be set");
        if (!ref) RMR_FAIL(RMR_ERR_INVALID, "the hemi mode of the emit needs a reference: ref is NULL");
        if (ref->combine == 0) RMR_FAIL(RMR_ERR_INVALID, "the hemi mode of the emit folds the strands: combine must be set");
        if (ref->n_motifs != 1) RMR_FAIL(RMR_ERR_INVALID, "the hemi mode of the emit takes exactly one motif, got %d", ref->n_motifs);
    }
    const PileupEmit pe{opt->region_ref, opt->region_lo, opt->region_hi, k_t, reinterpret_cast<unsigned long long *>(hist), words};
    PileupRef pr{};
    if (ref) RMR_TRY(fill_ref_part(e, b, ref, &pr));
    if (opt->hemi != 0) pr.combine = 2;
    if (b->n_records == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (opt->duplex != 0) return launch_modbam_calls_duplex(e, *b, pe, pr, ref != nullptr, ords, cig_q, cig_r, counts, status, out_off);
    if (ref) return launch_modbam_calls_ref(e, *b, pe, pr, ords, cig_q, cig_r, counts, status, out_off);
    return launch_modbam_calls(e, *b, pe, ords, cig_q, cig_r, counts, status, out_off);
}

extern "C" {

int rmr_pileup_emit_counts(rmr_engine *e, const rmr_modbam_batch *b, const rmr_pileup_emit_opts *opt, int32_t *ords, int64_t *cig_q, int64_t *cig_r,
                           int64_t *counts, int32_t *status, uint64_t *hist) {
    if (!e || !b || !opt || !counts || !status) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    return pileup_emit(e, b, opt, 0, ords, cig_q, cig_r, counts, status, hist, nullptr, nullptr);
}

int rmr_pileup_emit_fill(rmr_engine *e, const rmr_modbam_batch *b, const rmr_pileup_emit_opts *opt, int32_t k_t, const int32_t *ords,
                         const int64_t *cig_q, const int64_t *cig_r, const int32_t *status, const int64_t *out_off, uint64_t *words) {
    if (!e || !b || !opt || !status || !out_off || !words) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    return pileup_emit(e, b, opt, k_t, const_cast<int32_t *>(ords), const_cast<int64_t *>(cig_q), const_cast<int64_t *>(cig_r), nullptr,
                       const_cast<int32_t *>(status), nullptr, out_off, words);
}

int rmr_pileup_pair_counts(rmr_engine *e, int64_t n_records, const int64_t *out_off, const uint64_t *words, int64_t n_words, int64_t *pairs) {
    if (!e || !out_off || !words || !pairs) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_records < 0 || n_records > (int64_t)1 << 30 || n_words < 0) RMR_FAIL(RMR_ERR_INVALID, "bad n_records or n_words");
    if (n_records == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_pileup_pairs(e, n_records, out_off, words, n_words, 0, pairs, nullptr, nullptr);
}

int rmr_pileup_pair_fill(rmr_engine *e, int64_t n_records, const int64_t *out_off, const uint64_t *words, int64_t n_words, int n_codes,
                         const int64_t *pair_off, uint64_t *pair_words) {
    if (!e || !out_off || !words || !pair_off || !pair_words) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_records < 0 || n_records > (int64_t)1 << 30 || n_words < 0) RMR_FAIL(RMR_ERR_INVALID, "bad n_records or n_words");
    if (n_codes < 3 || n_codes > 4)
        RMR_FAIL(RMR_ERR_INVALID, "a pair word holds n_codes^2 <= 16 pattern codes: n_codes (the modified bases + 2) is 3 or 4, got %d", n_codes);
    if (n_records == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_pileup_pairs(e, n_records, out_off, words, n_words, n_codes, nullptr, pair_off, pair_words);
}

// n_alpha: rmr_pileup_create's argument (ncol = n_alpha + 1 then; its own bound and message), NULL from rmr_pileup_create_cols
static int pileup_create(rmr_engine *e, int64_t n_contigs, int64_t max_contig_len, int ncol, const int *n_alpha, int64_t buffer_calls,
                         rmr_pileup **out);

int rmr_pileup_create(rmr_engine *e, int64_t n_contigs, int64_t max_contig_len, int n_alpha, int64_t buffer_calls, rmr_pileup **out) {
    return pileup_create(e, n_contigs, max_contig_len, n_alpha >= 2 && n_alpha <= 8 ? n_alpha + 1 : 0, &n_alpha, buffer_calls, out);
}

int rmr_pileup_create_cols(rmr_engine *e, int64_t n_contigs, int64_t max_contig_len, int ncol, int64_t buffer_calls, rmr_pileup **out) {
    return pileup_create(e, n_contigs, max_contig_len, ncol, nullptr, buffer_calls, out);
}

static int pileup_create(rmr_engine *e, int64_t n_contigs, int64_t max_contig_len, int ncol, const int *n_alpha, int64_t buffer_calls,
                         rmr_pileup **out) {
    if (out) *out = nullptr;
    if (!e || !out) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_contigs < 1 || n_contigs > RMR_PILEUP_MAX_CONTIGS)
        RMR_FAIL(RMR_ERR_INVALID, "a pileup holds 1 to %lld contigs (24 bits of a site word), got %lld", (long long)RMR_PILEUP_MAX_CONTIGS,
                 (long long)n_contigs);
    if (max_contig_len < 0 || max_contig_len > RMR_PILEUP_MAX_POS)
        RMR_FAIL(RMR_ERR_INVALID, "a pileup holds positions below %lld (31 bits of a site word), the longest contig has %lld bases",
                 (long long)RMR_PILEUP_MAX_POS, (long long)max_contig_len);
    if (n_alpha && ncol == 0) RMR_FAIL(RMR_ERR_INVALID, "a pileup counts the canonical base and 1 to 7 modified bases, got %d classes", *n_alpha);
    if (ncol < 3 || ncol > 16) RMR_FAIL(RMR_ERR_INVALID, "a row of the pileup has 3 to 16 columns (the 4 bits of a word's code), got %d", ncol);
    if (buffer_calls < 1 || buffer_calls > (int64_t)INT32_MAX) RMR_FAIL(RMR_ERR_INVALID, "the call buffer holds 1 to 2^31 - 1 words, got %lld", (long long)buffer_calls);
    rmr_pileup *p = new (std::nothrow) rmr_pileup();
    if (!p) RMR_FAIL(RMR_ERR_NOMEM, "out of host memory");
    p->eng = e, p->ncol = ncol, p->cap = buffer_calls;
    p->end_bit = 36;
    while (p->end_bit < 60 && ((int64_t)1 << (p->end_bit - 36)) < n_contigs) p->end_bit += 1;
    std::lock_guard<std::mutex> lk(e->mu);
    int rc = hipSetDevice(e->device) == hipSuccess ? 0 : RMR_ERR_HIP;
    if (rc != 0) set_error("hipSetDevice(%d) failed", e->device);
    if (rc == 0) rc = pileup_alloc(p);
    if (rc != 0) {
        if (p->work) (void)hipFree(p->work);
        delete p;
        return rc;
    }
    *out = p;
    return 0;
}

int rmr_pileup_add(rmr_pileup *p, const uint64_t *words, int64_t n) {
    if (!p || !p->eng || n < 0 || (n > 0 && !words)) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    if (n == 0) return 0;
    rmr_engine *e = p->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return pileup_append(p, words, n);
}

int rmr_pileup_finish(rmr_pileup *p, int64_t *n_sites, int64_t *n_calls, int64_t *n_flushes, int64_t *peak_device_bytes) {
    if (!p || !p->eng) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    rmr_engine *e = p->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    RMR_TRY(pileup_flush(p));
    unsigned long long over = 0;
    D2H(&over, p->overflow, 8);
    RMR_HIP(hipStreamSynchronize(e->stream));
    if (over) {
        const uint64_t key = over - 1;
        RMR_FAIL(RMR_ERR_INVALID, "the count of a site would pass 2^32 - 1: contig #%lld, position %lld, strand %c", (long long)(key >> 32),
                 (long long)((key >> 1) & 0x7fffffffull), (key & 1) ? '-' : '+');
    }
    p->finished = true;
    if (n_sites) *n_sites = p->nt;
    if (n_calls) *n_calls = p->n_calls;
    if (n_flushes) *n_flushes = p->n_flushes;
    if (peak_device_bytes) *peak_device_bytes = (int64_t)p->peak_bytes;
    return 0;
}

int rmr_pileup_read(rmr_pileup *p, uint64_t *keys, uint32_t *counts) {
    if (!p || !p->eng) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    if (p->used != 0) RMR_FAIL(RMR_ERR_INVALID, "rmr_pileup_read before rmr_pileup_finish: %lld words are still in the buffer", (long long)p->used);
    if (p->nt == 0) return 0;
    if (!keys || !counts) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    rmr_engine *e = p->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    D2H(keys, p->t_keys, (size_t)p->nt * 8);
    D2H(counts, p->t_counts, (size_t)p->nt * p->ncol * 4);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

int rmr_pileup_stamp_partition(rmr_engine *e, int64_t n_records, const int64_t *out_off, const int32_t *part, int shift, uint64_t *words,
                               int64_t n_words) {
    if (!e || !out_off || !part || !words) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (n_records < 0 || n_records > (int64_t)1 << 30 || n_words < 0) RMR_FAIL(RMR_ERR_INVALID, "bad n_records or n_words");
    if (shift < 36 || shift > 59) RMR_FAIL(RMR_ERR_INVALID, "the partition field starts at bit 36 to 59 of a site word, got %d", shift);
    if (n_records == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    return launch_pileup_stamp(e, n_records, out_off, part, shift, words, n_words);
}

int rmr_pileup_set_canonical(rmr_pileup *p, int base) {
    if (!p || !p->eng) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    if (base == 'U') base = 'T';
    if (base != 'A' && base != 'C' && base != 'G' && base != 'T')
        RMR_FAIL(RMR_ERR_INVALID, "the canonical base of a pileup is A, C, G, T or U, got character %d", base);
    p->canonical = base;
    return 0;
}

int rmr_pileup_cover(rmr_pileup *p, const rmr_modbam_batch *b, const rmr_pileup_ref *ref, const int32_t *status, const int64_t *cig_q,
                     const int64_t *cig_r, const int64_t *out_off, const uint64_t *words, int64_t n_words, const int32_t *part, int shift) {
    if (!p || !p->eng || !b) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    rmr_engine *e = p->eng;
    if (!p->finished || p->used != 0) RMR_FAIL(RMR_ERR_INVALID, "rmr_pileup_cover before rmr_pileup_finish: the table is not complete");
    if (!p->canonical) RMR_FAIL(RMR_ERR_INVALID, "rmr_pileup_cover before rmr_pileup_set_canonical: the canonical base is not known");
    RMR_TRY(check_call_batch(b, -1, 0, 0));
    if (n_words < 0 || (n_words > 0 && !words)) RMR_FAIL(RMR_ERR_INVALID, "bad n_words or NULL words");
    if (b->n_records > 0 && (!status || !cig_q || !cig_r || !out_off || !b->seq || !b->cigar)) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    if (part && (shift < 36 || shift > 59)) RMR_FAIL(RMR_ERR_INVALID, "the partition field starts at bit 36 to 59 of a site word, got %d", shift);
    PileupRef pr{};
    const bool combine = ref && ref->combine != 0;
    int fold_window = 0;
    if (combine) {
        RMR_TRY(fill_ref_part(e, b, ref, &pr));
        for (int j = 0; j < pr.n_motifs; ++j) {  // a folded '-' word stands within max |len - 1 - 2 focus| of its own position
            const int sh = pr.motifs[j].len - 1 - 2 * pr.motifs[j].focus;
            fold_window = std::max(fold_window, 2 * (sh < 0 ? -sh : sh));
        }
        if (pr.n_motifs == 1) fold_window = 0;  // one motif: one shift, the folded words are strictly monotone
    }
    if (b->n_records == 0 || p->nt == 0) return 0;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (!p->cover) {
        const size_t bytes = (size_t)p->nt * 3 * sizeof(uint32_t);
        void *mem = nullptr;
        if (hipMalloc(&mem, bytes) != hipSuccess) {
            (void)hipGetLastError();
            RMR_FAIL(RMR_ERR_NOMEM, "the coverage counts of %lld sites need %zu bytes of device memory and they could not be allocated", (long long)p->nt,
                     bytes);
        }
        p->cover = static_cast<uint32_t *>(mem), p->cover_bytes = bytes;
        RMR_HIP(hipMemsetAsync(p->cover, 0, bytes, e->stream));
        if (p->work_bytes + p->t_bytes + bytes > p->peak_bytes) p->peak_bytes = p->work_bytes + p->t_bytes + bytes;
    }
    return launch_pileup_cover(p, *b, pr, combine, fold_window, status, cig_q, cig_r, out_off, words, n_words, part, shift);
}

int rmr_pileup_read_cover(rmr_pileup *p, uint32_t *cover) {
    if (!p || !p->eng) RMR_FAIL(RMR_ERR_INVALID, "bad argument");
    if (!p->finished || p->used != 0) RMR_FAIL(RMR_ERR_INVALID, "rmr_pileup_read_cover before rmr_pileup_finish: the table is not complete");
    if (p->nt == 0) return 0;
    if (!cover) RMR_FAIL(RMR_ERR_INVALID, "NULL argument");
    rmr_engine *e = p->eng;
    std::lock_guard<std::mutex> lk(e->mu);
    RMR_HIP(hipSetDevice(e->device));
    if (!p->cover) {  // no record was joined against this table
        std::memset(cover, 0, (size_t)p->nt * 3 * sizeof(uint32_t));
        return 0;
    }
    D2H(cover, p->cover, p->cover_bytes);
    RMR_HIP(hipStreamSynchronize(e->stream));
    return 0;
}

void rmr_pileup_destroy(rmr_pileup *p) {
    if (!p) return;
    (void)hipSetDevice(p->eng->device);
    (void)hipStreamSynchronize(p->eng->stream);  // nothing may still read the buffer or the table when they are freed
    if (p->cover) (void)hipFree(p->cover);
    if (p->work) (void)hipFree(p->work);
    if (p->t_mem) (void)hipFree(p->t_mem);
    delete p;
}

}  // extern "C"
