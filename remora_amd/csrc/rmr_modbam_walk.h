// rmr_modbam_walk.h — the walk of a batch of BAM records' modified-base calls (the tokenised MM / ML tags, mod_tags.cpp) along
// the reads' bases and through the CIGARs to reference positions, shared by the two kernels that end it differently:
//   k_modbam.hip  (PILEUP = false)  a call is kept where the ground-truth table of `validate from_modbams` holds its position
//                                   and goes to the host as a row of probabilities with its label;
//   k_pileup.hip  (PILEUP = true)   every aligned call is kept (inside the region, if one is given), classified in integers
//                                   and written as one 64-bit site word - or only counted into the histogram of its confidence.
//                                   With a reference genome (PileupRef) a call is kept only where the reference shows
//                                   one of up to four motifs around it, and a '-' call can be folded onto the '+' position of
//                                   its motif (motif_keep below): everything after the keep test sees the filtered, folded calls.
//                                   DUPLEX (k_pileup_duplex.hip): '-'-strand entries count too - their calls lie on the reference
//                                   strand opposite to the record's, and that effective strand is what the word, the motif
//                                   test and the fold see.
//
// One workgroup of four waves per record, the same walk twice (count, then fill into the caller's prefix-summed offsets):
//   count pass only
//     1. the entries' ranges are checked against the flat arrays (nothing below indexes outside them), and whether any
//        entry counts (strand '+' - DUPLEX: or '-' -, a code of the alphabet);
//     2. CIGAR: exclusive prefix sums of the query and the reference lengths of the ops -> cig_q / cig_r (block scan, 256
//        ops a round);
//     3. per entry: inclusive prefix sum of (delta + 1) -> ords[k] = d_0 + .. + d_k + k, the occurrence ordinal of call k
//        (block scan, 256 deltas a round; clamped to int32: an ordinal beyond a read's length is beyond its last occurrence);
//   both passes
//     4. the walk: 256 bases of the ORIGINAL sequence a round (a reverse record's from its stored end, complemented).  Four
//        ballots give every base its occurrence number among the A / C / G / T of the read so far (running totals in
//        registers, nothing sized by the read: 1 base or megabases alike); for every entry of its base (or N) the thread
//        searches its occurrence number in the entry's ordinals - found = call k - and takes (ML + 0.5) / 256 for the codes
//        that count, later entries overwriting earlier ones.  A called base finds its CIGAR op by binary search in cig_q, its
//        reference position from cig_r, and then (truth join) its label by binary search in the truth slice of (ref_id,
//        strand).  Kept calls are compacted by a block prefix count: ascending stored position, i.e. back to front for a
//        reverse record (the pileup's words: ascending walk position, they are sorted afterwards).
//   The count pass ends with the check that no entry's last ordinal lies beyond the occurrences of its base.
// Every probability is a multiple of 1/512 below 8: float arithmetic is exact in any order, and 512 p is an exact integer.
#pragma once
#include "rmr_internal.h"

namespace rmr {

constexpr int MB_THREADS = 256, MB_WAVES = MB_THREADS / 64;

// inclusive scan of two int64 over the block; ta / tb = the block's totals.  s: int64[MB_WAVES][2] of LDS.
__device__ inline void block_scan2(int64_t &a, int64_t &b, int64_t &ta, int64_t &tb, int64_t (*s)[2], int lane, int wave) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long oa = __shfl_up((long long)a, d), ob = __shfl_up((long long)b, d);
        if (lane >= d) a += oa, b += ob;
    }
    if (lane == 63) s[wave][0] = a, s[wave][1] = b;
    __syncthreads();
    int64_t pa = 0, pb = 0;
    ta = tb = 0;
#pragma unroll
    for (int w = 0; w < MB_WAVES; ++w) {
        if (w < wave) pa += s[w][0], pb += s[w][1];
        ta += s[w][0], tb += s[w][1];
    }
    a += pa, b += pb;
    __syncthreads();  // s is free again
}

__device__ inline int base_index(int c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }
__device__ inline int complement(int c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c; }

// ---- the reference part of the pileup's keep test (k_ref_genome.hip: the form and the codes) ----
// the code of base i of a contig whose nibbles start at data[off]; 0 outside [0, len)
__device__ inline int ref_code(const uint8_t *__restrict__ data, int64_t off, int64_t len, int64_t i) {
    if (i < 0 || i >= len) return 0;
    const int byte = data[off + (i >> 1)];
    return (i & 1) ? byte >> 4 : byte & 15;
}

// do the L bases from s on match the L nibble masks of `masks`?  A reference code r matches a mask m iff r != 0 and
// (r & ~m) == 0; a window that leaves the contig does not match.
__device__ inline bool motif_window(const uint8_t *__restrict__ data, int64_t off, int64_t len, int64_t s, int L, uint64_t masks) {
    if (s < 0 || s + L > len) return false;
    for (int i = 0; i < L; ++i) {
        const int r = ref_code(data, off, len, s + i), m = (int)(masks >> (4 * i)) & 15;
        if (r == 0 || (r & ~m) != 0) return false;
    }
    return true;
}

// A call at reference position rp of contig `rid`, on '-' when rev: is it on a motif, and where is it written?  The first
// motif that matches decides; *wp = rp, or with pr.combine for a '-' call rp - (L - 1 - 2 focus): the focus of the same
// window read on '+' (inside the contig, as the window is).
__device__ inline bool motif_keep(const PileupRef &pr, int64_t rid, bool rev, int64_t rp, int64_t *wp) {
    const int64_t off = pr.off[rid], len = pr.len[rid];
    for (int j = 0; j < pr.n_motifs; ++j) {
        const rmr_pileup_motif &mo = pr.motifs[j];
        const int64_t s = rp - (rev ? mo.len - 1 - mo.focus : mo.focus);
        if (motif_window(pr.data, off, len, s, mo.len, rev ? mo.rc_mask : mo.mask)) {
            *wp = (rev && pr.combine) ? s + mo.focus : rp;
            return true;
        }
    }
    return false;
}

// The body of both kernels; called by every thread of a block of MB_THREADS.  PILEUP: probs / label / qpos / rpos are not
// touched and the truth fields of `b` are not read; s_hist is PILEUP_BINS words of LDS (count pass with pe.hist) or unused.
// REF (PILEUP only): the motif test and the fold by `rf`; without it `rf` is not read and the pileup compiles the code it had
// before there was a reference.
// DUPLEX (PILEUP only): entries of strand '-' count like those of '+'.  A position keeps the strand of the last entry, in tag
// order, that lists it with a code of the alphabet; what entries of the other strand gave it before is dropped.  The call's
// effective strand is rev XOR (that entry's strand == '-').  rf.combine == 2 (the hemi mode of the fill): the fold writes the
// '+' position of the window and the word keeps the strand bit.  Without DUPLEX none of this is compiled.
template <bool FILL, bool PILEUP, bool REF = false, bool DUPLEX = false>
__device__ __forceinline__ void modbam_walk(const rmr_modbam_batch &b, int32_t *__restrict__ ords, int64_t *__restrict__ cig_q,
                                            int64_t *__restrict__ cig_r, int64_t *__restrict__ counts, int32_t *__restrict__ status,
                                            const int64_t *__restrict__ out_off, float *__restrict__ probs, uint8_t *__restrict__ label,
                                            int64_t *__restrict__ qpos, int64_t *__restrict__ rpos, const PileupEmit &pe,
                                            unsigned *__restrict__ s_hist, const PileupRef &rf = PileupRef{}) {
    __shared__ int64_t s_scan[MB_WAVES][2];
    __shared__ int s_base[MB_WAVES][4];
    __shared__ int s_emit[MB_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x;
    // ---- records skipped whole (every test below is uniform over the block) ----
    if (FILL) {
        if (status[r] != 0 || out_off[r + 1] <= out_off[r]) return;
    } else {
        int st = b.tok_status[r];
        if (PILEUP) {
            const int fl = b.flag[r];
            if (st == 0 && (b.ref_id[r] < 0 || (fl & 0x4))) st = 3;
            if (st == 0 && (fl & 0x900)) st = 6;                     // secondary / supplementary
            if (st == 0 && (int64_t)b.ref_id[r] >= b.n_refs) st = 2;  // a contig the header does not have
        } else {
            if (st == 0 && b.ref_id[r] < 0) st = 3;
            if (st == 0 && !(b.has[r] & 0x80)) st = 4;
        }
        if (st != 0) {
            if (tid == 0) status[r] = st, counts[r] = 0;
            return;
        }
    }
    const int64_t e0 = b.ent_off[r], e1 = b.ent_off[r + 1];
    const int64_t s0 = b.seq_off[r], L = b.seq_off[r + 1] - s0;
    const int64_t c0 = b.cigar_off[r], nc = b.cigar_off[r + 1] - c0;
    const bool rev = (b.flag[r] & 0x10) != 0;
    const int n_mods = b.n_mods, n_alpha = n_mods + 1;
    int malformed = 0;
    const bool want_hist = PILEUP && !FILL && pe.hist != nullptr;

    if (!FILL) {
        // ---- 1. entries inside the flat arrays; does any of them count? ----
        int bad = 0, kept = 0;
        for (int64_t e = e0 + tid; e < e1; e += MB_THREADS) {
            const rmr_mod_entry &en = b.entries[e];
            const int64_t nd = en.n_deltas, ncd = en.n_codes;
            if (nd < 0 || ncd < 1 || ncd > RMR_MOD_MAX_CODES || en.delta_off < 0 || en.delta_off + nd > b.n_deltas || en.ml_off < 0 ||
                en.ml_off + nd * ncd > b.n_ml)
                bad = 1;
            else if ((en.strand == '+' || (DUPLEX && en.strand == '-')) && en.chebi == 0)
                for (int ci = 0; ci < ncd; ++ci)
                    for (int j = 0; j < n_mods; ++j) kept |= en.codes[ci] == b.mod_codes[j];
        }
        bad = __syncthreads_or(bad || L > 0x7fffffff);
        kept = __syncthreads_or(kept);
        if (bad || !kept) {
            if (tid == 0) status[r] = bad ? 2 : 5, counts[r] = 0;
            return;
        }
        if (want_hist)  // (the barriers of the scans below stand between this and the first count)
            for (int i = tid; i < PILEUP_BINS; i += MB_THREADS) s_hist[i] = 0;
        // ---- 2. CIGAR prefix sums ----
        int64_t run_q = 0, run_r = 0;
        for (int64_t i0 = 0; i0 < nc; i0 += MB_THREADS) {
            const int64_t i = i0 + tid;
            int64_t ql = 0, rl = 0, len = 0;
            if (i < nc) {
                const uint32_t w = b.cigar[c0 + i];
                const int op = (int)(w & 15u);
                len = (int64_t)(w >> 4);
                ql = (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? len : 0;  // M I S = X
                rl = (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? len : 0;  // M D N = X
            }
            int64_t a = ql, c = rl, ta, tc;
            block_scan2(a, c, ta, tc, s_scan, lane, wave);
            if (i < nc) cig_q[c0 + i] = run_q + a - ql, cig_r[c0 + i] = run_r + c - rl;
            run_q += ta, run_r += tc;
        }
        if (run_q != L) malformed = 1;  // (an empty CIGAR included: no base of such a record is aligned)
        // ---- 3. occurrence ordinals of the calls ----
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t nd = b.entries[e].n_deltas, d0 = b.entries[e].delta_off;
            int64_t run = 0;
            for (int64_t k0 = 0; k0 < nd; k0 += MB_THREADS) {
                const int64_t k = k0 + tid;
                int64_t a = k < nd ? (int64_t)b.deltas[d0 + k] + 1 : 0, unused = 0, ta, tu;
                if (a < 1) a = 1;  // (the tokeniser writes no negative delta; an array from elsewhere must not run the ordinals backwards)
                block_scan2(a, unused, ta, tu, s_scan, lane, wave);
                if (k < nd) {
                    const int64_t o = run + a - 1;
                    ords[d0 + k] = o > 0x7fffffff ? 0x7fffffff : (int32_t)o;
                }
                run += ta;
            }
        }
        __syncthreads();  // the ordinals and the CIGAR sums of this record are read by all of its threads from here on
    }

    // ---- 4. the walk ----
    int64_t run_base[4] = {0, 0, 0, 0}, emitted = 0;
    const int64_t o_lo = FILL ? out_off[r] : 0, o_hi = FILL ? out_off[r + 1] : 0;
    int64_t t0 = 0, t1 = 0;
    if (!PILEUP) {
        const int64_t n_truth_slices = 2 * b.n_refs, slice = 2 * (int64_t)b.ref_id[r] + (rev ? 1 : 0);
        t0 = slice < n_truth_slices ? b.truth_off[slice] : 0, t1 = slice < n_truth_slices ? b.truth_off[slice + 1] : 0;
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t p0 = 0; p0 < L && !(FILL ? false : malformed); p0 += MB_THREADS) {
        const int64_t p = p0 + tid;
        const bool valid = p < L;
        const int64_t sp = rev ? L - 1 - p : p;
        int c = valid ? (int)b.seq[s0 + sp] : 0;
        if (rev) c = complement(c);
        const int bi = base_index(c);
        int excl = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const unsigned long long m = __ballot(bi == x);
            if (bi == x) excl = __popcll(m & lt);
            if (lane == 0) s_base[wave][x] = __popcll(m);
        }
        __syncthreads();
        int64_t occ_own = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            int before = 0, tot = 0;
#pragma unroll
            for (int w = 0; w < MB_WAVES; ++w) {
                if (w < wave) before += s_base[w][x];
                tot += s_base[w][x];
            }
            if (bi == x) occ_own = run_base[x] + before + excl;
            run_base[x] += tot;
        }
        // the calls on this base
        float pr[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool called = false;
        bool on_minus = false;  // DUPLEX: the strand of the entries the probabilities are from
        if (valid) {
            for (int64_t e = e0; e < e1; ++e) {
                const rmr_mod_entry &en = b.entries[e];
                const int nd = en.n_deltas;
                if (nd == 0) continue;
                const int eb = en.base == 'U' ? 'T' : en.base;
                int64_t occ;
                if (eb == 'N') occ = p;
                else if (bi >= 0 && eb == c) occ = occ_own;
                else continue;
                const int32_t *o = ords + en.delta_off;
                int lo = 0, hi = nd;
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if ((int64_t)o[mid] < occ) lo = mid + 1;
                    else hi = mid;
                }
                if (lo >= nd || (int64_t)o[lo] != occ) continue;
                if ((en.strand != '+' && !(DUPLEX && en.strand == '-')) || en.chebi != 0) continue;
                const int ncd = en.n_codes;
                const uint8_t *q = b.ml + en.ml_off + (int64_t)lo * ncd;
                if (DUPLEX) {
                    bool listed = false;  // an entry without a code of the alphabet decides nothing
                    for (int ci = 0; ci < ncd; ++ci)
                        for (int j = 0; j < n_mods; ++j) listed |= en.codes[ci] == b.mod_codes[j];
                    if (!listed) continue;
                    const bool em = en.strand == '-';
                    if (called && em != on_minus) {
#pragma unroll
                        for (int j = 0; j < 7; ++j) pr[j] = 0.f;
                    }
                    on_minus = em;
                }
                for (int ci = 0; ci < ncd; ++ci) {
                    const char code = en.codes[ci];
#pragma unroll
                    for (int j = 0; j < 7; ++j)
                        if (j < n_mods && code == b.mod_codes[j]) pr[j] = ((float)q[ci] + 0.5f) * (1.0f / 256.0f), called = true;
                }
            }
        }
        // stored position -> reference position -> truth label (or the region test)
        bool keep = false;
        int64_t rp = 0;
        int lab = 0;
        if (called && nc > 0) {
            int64_t lo = 0, hi = nc;  // the last op that starts at or before sp
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (cig_q[c0 + mid] <= sp) lo = mid + 1;
                else hi = mid;
            }
            if (lo > 0) {
                const int64_t i = lo - 1;
                const uint32_t w = b.cigar[c0 + i];
                const int op = (int)(w & 15u);
                const int64_t within = sp - cig_q[c0 + i];
                if ((op == 0 || op == 7 || op == 8) && within < (int64_t)(w >> 4)) {
                    rp = (int64_t)b.pos[r] + cig_r[c0 + i] + within;
                    if (PILEUP) {
                        // (a position outside the word's 31 bits cannot come from a BAM whose header passed the host's check)
                        // with a reference: only calls on a motif, and a '-' call folded onto '+'; the region is asked of the
                        // position that is written (rp from here on)
                        // (DUPLEX: the call lies on the effective strand, rev XOR the strand of its entries; written out at
                        // its two uses - a variable for it moved an instruction of the kernels without the flag)
                        if (REF) keep = rp >= 0 && rp < ((int64_t)1 << 31) && motif_keep(rf, b.ref_id[r], DUPLEX ? rev != on_minus : rev, rp,
                                                                                                &rp);
                        keep = (REF ? keep : rp >= 0 && rp < ((int64_t)1 << 31)) &&
                               (pe.region_ref < 0 || (b.ref_id[r] == pe.region_ref && rp >= pe.region_lo && rp < pe.region_hi));
                    } else {
                        int64_t a = t0, z = t1;
                        while (a < z) {
                            const int64_t mid = a + ((z - a) >> 1);
                            if (b.truth_pos[mid] < rp) a = mid + 1;
                            else z = mid;
                        }
                        if (a < t1 && b.truth_pos[a] == rp) keep = true, lab = b.truth_label[a];
                    }
                }
            }
        }
        const unsigned long long km = __ballot(keep);
        if (lane == 0) s_emit[wave] = __popcll(km);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < MB_WAVES; ++w) {
            if (w < wave) before += s_emit[w];
            tot += s_emit[w];
        }
        if (PILEUP) {
            if (keep && (FILL || want_hist)) {
                // the class: argmax over (512 - sum, k_1 .. k_n), ties to the lower column; k = 512 p, exact
                int sum = 0, best = 0, kmax;
                int kj[7];
#pragma unroll
                for (int j = 0; j < 7; ++j) kj[j] = j < n_mods ? (int)(pr[j] * 512.0f) : 0, sum += kj[j];
                kmax = 512 - sum;
#pragma unroll
                for (int j = 0; j < 7; ++j)
                    if (j < n_mods && kj[j] > kmax) kmax = kj[j], best = 1 + j;
                if (kmax < 0) kmax = 0;  // (never: a called position has a code with k >= 1)
                if (FILL) {
                    const int64_t o = o_lo + emitted + before + __popcll(km & lt);
                    if (o >= o_lo && o < o_hi) {  // (offsets that are not this batch's counts write nothing outside the record's slice)
                        const uint64_t code = kmax >= pe.k_t ? (uint64_t)best : (uint64_t)(n_mods + 1);
                        // (a folded call stands on '+' - in the hemi mode, combine == 2, it keeps its strand bit)
                        const bool minus = (DUPLEX ? rev != on_minus : rev) && !(REF && (DUPLEX ? rf.combine == 1 : rf.combine != 0));
                        pe.words[o] = ((uint64_t)b.ref_id[r] << 36) | ((uint64_t)rp << 5) | ((uint64_t)(minus ? 1 : 0) << 4) | code;
                    }
                } else {
                    atomicAdd(&s_hist[kmax], 1u);
                }
            }
        } else if (FILL && keep) {
            const int64_t rank = emitted + before + __popcll(km & lt);
            const int64_t o = rev ? o_hi - 1 - rank : o_lo + rank;
            if (o >= o_lo && o < o_hi) {  // (offsets that are not this batch's counts write nothing outside the record's slice)
                float sum = 0.f;
                for (int j = 0; j < n_mods; ++j) sum += pr[j];
                float *row = probs + o * n_alpha;
                row[0] = 1.0f - sum;
                for (int j = 0; j < n_mods; ++j) row[1 + j] = pr[j];
                label[o] = (uint8_t)lab;
                qpos[o] = sp;
                rpos[o] = rp;
            }
        }
        emitted += tot;
    }
    if (!FILL) {
        // a call beyond the last occurrence of its base: the whole record is malformed (uniform: every thread walks the entries)
        for (int64_t e = e0; e < e1 && !malformed; ++e) {
            const rmr_mod_entry &en = b.entries[e];
            if (en.n_deltas == 0) continue;
            const int eb = en.base == 'U' ? 'T' : en.base;
            const int x = base_index(eb);
            const int64_t have = eb == 'N' ? L : x >= 0 ? run_base[x] : 0;
            if ((int64_t)ords[en.delta_off + en.n_deltas - 1] >= have) malformed = 1;
        }
        if (tid == 0) status[r] = malformed ? 2 : 0, counts[r] = malformed ? 0 : emitted;
        if (want_hist) {  // the record's bins go out only now that it is known to count: one integer atomic per non-zero bin
            __syncthreads();
            if (!malformed)
                for (int i = tid; i < PILEUP_BINS; i += MB_THREADS)
                    if (s_hist[i]) atomicAdd(&pe.hist[i], (unsigned long long)s_hist[i]);
        }
    }
}

}  // namespace rmr
