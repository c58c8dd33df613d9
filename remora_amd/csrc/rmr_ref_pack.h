// rmr_ref_pack.h — the arithmetic of loading a contig of a FASTA file into the device's nibble table (k_ref_genome.hip,
// api_ref.hip), in plain C++ that the host, the kernel and a CPU harness share (tools/fuzz/ref_pack_asan.cpp runs every
// function here under AddressSanitizer against text and piece buffers of exact size).
//
// A contig's text is the bytes of its sequence lines as they stand in the file, from its first base to its last: lines of
// `lb` bases followed by W - lb terminator bytes ("\n" or "\r\n"), the last line possibly shorter and without terminator.
// Base i stands at (i / lb) * W + i % lb.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RMR_HD __host__ __device__
#else
#define RMR_HD
#endif

namespace rmr {

// the IUPAC set of a letter as a mask (A 1, C 2, G 4, T / U 8, an ambiguity letter the union of its bases, N 15; either
// case); 0: no IUPAC letter.  The table is 26 nibbles, 'A' + i in bits 4 i .. 4 i + 3 of lo (i < 16) or hi.
RMR_HD inline int iupac_code(int c) {
    const int i = (c | 0x20) - 'a';
    if (i < 0 || i >= 26 || c < 'A' || (c > 'Z' && c < 'a')) return 0;
    //                        P O N M L K J I H G F E D C B A                       Z Y X W V U T S R Q
    const uint64_t lo = 0x00F30C00B400D2E1ull, hi = 0x0A09788650ull;
    return (int)((i < 16 ? lo >> (4 * i) : hi >> (4 * (i - 16))) & 15);
}

// the bases that S bytes of text hold, as `samtools faidx` computes a contig's length
RMR_HD inline int64_t ref_bases_of_text(int64_t S, int64_t lb, int64_t W) { return (S / W) * lb + (S % W < lb ? S % W : lb); }

// where base i of a contig of `len` bases stands in its text of S bytes; i >= len: the text's end
RMR_HD inline int64_t ref_text_at(int64_t i, int64_t len, int64_t lb, int64_t W, int64_t S) { return i >= len ? S : (i / lb) * W + i % lb; }

// The piece that starts at base i0 (even, below len): the most bases - an even number, or all that are left - whose text,
// the terminators behind the last of them included, takes at most piece_bytes (>= 16: two bases and their terminators
// always fit).  -> the number of bases; *t_lo, *t_n: the piece's bytes in the text.
inline int64_t ref_next_piece(int64_t i0, int64_t len, int64_t lb, int64_t W, int64_t S, int64_t piece_bytes, int64_t *t_lo, int64_t *t_n) {
    int64_t nb = ref_bases_of_text(piece_bytes, lb, W) & ~(int64_t)1;
    if (nb < 2) nb = 2;
    if (nb > len - i0) nb = len - i0;
    *t_lo = ref_text_at(i0, len, lb, W, S);
    while (nb > 2 && ref_text_at(i0 + nb, len, lb, W, S) - *t_lo > piece_bytes) nb -= (nb & 1) ? 1 : 2;
    *t_n = ref_text_at(i0 + nb, len, lb, W, S) - *t_lo;
    return nb;
}

// What the thread of one output byte does.  text: the piece, text[0] = byte text_lo of the contig's text of span_bytes bytes,
// text_bytes of it; the piece holds bases [.., base_hi).  -> the packed byte of bases i0 (even) and i0 + 1 (low nibble first;
// a base at or beyond base_hi is nibble 0).  *bad: the smallest text offset among the bytes this thread checks - its bases,
// and behind a line's last base the terminator columns as far as the text goes - that is no IUPAC letter, or not the
// terminator; ~0 when all are fine.
RMR_HD inline int ref_pack_pair(const uint8_t *text, int64_t text_lo, int64_t text_bytes, int64_t span_bytes, int64_t i0, int64_t base_hi,
                                int64_t lb, int64_t W, unsigned long long *bad) {
    const int term = (int)(W - lb);
    int byte = 0;
    unsigned long long first = ~0ull;
    for (int h = 0; h < 2; ++h) {
        const int64_t i = i0 + h;
        if (i >= base_hi) break;
        const int64_t col = i % lb, at = (i / lb) * W + col, rel = at - text_lo;
        if (rel < 0 || rel >= text_bytes) continue;  // (the host cut the piece around these bases: never true)
        const int code = iupac_code(text[rel]);
        if (code == 0 && (unsigned long long)at < first) first = (unsigned long long)at;
        byte |= code << (4 * h);
        if (col == lb - 1)
            for (int k = 0; k < term; ++k) {
                const int64_t a = at + 1 + k, rl = a - text_lo;
                if (a >= span_bytes || rl >= text_bytes) break;
                const int want = (term == 2 && k == 0) ? '\r' : '\n';
                if ((int)text[rl] != want && (unsigned long long)a < first) first = (unsigned long long)a;
            }
    }
    *bad = first;
    return byte;
}

}  // namespace rmr
