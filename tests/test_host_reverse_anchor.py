"""rmr_ref_anchor_batch_dir (ref_to_signal.cpp: the reference-anchor composition of a BAM batch on native threads, for either
signal direction) against the per-read composition in numpy: io.parse_move_tag's arithmetic for reverse signal
(src/remora/io.py:394-407: the moves' positions times the stride, the signal length appended, the two checks, then
sig_len - query_to_signal[::-1]) followed by data_chunks.compute_ref_to_signal on the strand-ordered CIGAR, as
Read.add_alignment composes them.  io.parse_move_tag itself expands on the GPU, so its four lines are restated here; the
CIGAR side is the package's own numpy code.  No GPU."""
import ctypes
import os

import numpy as np

from conftest import ROOT

DATA = os.path.join(ROOT, "tests", "golden", "data")
MATCH, QUERY, REF = (0, 7, 8), (0, 1, 4, 7, 8), (0, 2, 3, 7, 8)
ERR_INVALID = -1  # RMR_ERR_INVALID of include/remora_hip.h


def _pp(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _anchor(L, entry, mv, mv_off, sig_len, seq_len, cigar, cigar_off, rev, ref_len, *tail):
    n = len(sig_len)
    r2s_off = np.zeros(n + 1, np.int64)
    np.cumsum(np.maximum(ref_len, -1) + 1, out=r2s_off[1:])
    r2s = np.full(int(r2s_off[-1]) + 1, -7, np.int64)
    status = np.full(n, 77, np.int32)
    L.check(getattr(L.lib(), entry)(n, _pp(mv), _pp(mv_off), _pp(sig_len), _pp(seq_len), _pp(cigar), _pp(cigar_off), _pp(rev), _pp(ref_len),
                                    _pp(r2s), _pp(r2s_off), _pp(status), *tail))
    assert r2s[-1] == -7, "a write behind the last record's slot"
    return status, r2s, r2s_off


def _expected(L, mv, sig_len, seq_len, cig, strand_rev, ref_len, reverse_signal):
    """(status, ref_to_signal or None) of one record, the per-read path's way."""
    from remora_amd import RemoraError
    from remora_amd.data_chunks import compute_ref_to_signal

    if mv.size < 1:
        return 8, None
    if mv[0] <= 0:
        return ERR_INVALID, None
    q2s = np.concatenate([np.nonzero(mv[1:])[0] * int(mv[0]), [sig_len]]).astype(np.int64)
    if q2s.size - 1 != seq_len:
        return L.ERR_DISCORDANT_SEQ, None
    if mv.size - 1 != sig_len // int(mv[0]):
        return L.ERR_DISCORDANT_SIG, None
    if reverse_signal:
        q2s = sig_len - q2s[::-1]
    if ref_len < 0:
        return 9, None
    ops, lens = (cig & 0xF).astype(np.int64), (cig >> 4).astype(np.int64)
    if strand_rev:
        ops, lens = ops[::-1], lens[::-1]
    try:
        r2s = compute_ref_to_signal(query_to_signal=q2s, cigar=(ops, lens))
    except RemoraError as e:
        return {"Invalid cigar op(s)": 2, "No match operations found in alignment cigar": 3}[str(e)], None
    if r2s.size != ref_len + 1:
        return 1, None
    return 0, r2s


def _random_records(rng, n):
    mv, mv_off, sig_len, seq_len, cigar, cigar_off, rev, ref_len, kind = [], [0], [], [], [], [0], [], [], []
    kinds = ["ok"] * 12 + ["one base short", "signal short", "bad stride", "no moves", "no reference", "reference short", "bad op", "no match"]
    for _ in range(n):
        k = kinds[rng.randint(len(kinds))]
        n_ops = rng.randint(1, 9)
        ops = rng.choice([0, 0, 0, 1, 2, 3, 4, 7, 8], n_ops)
        if k == "no match":
            ops = rng.choice([1, 2, 4], n_ops)
        elif not np.isin(ops, MATCH).any():
            ops[rng.randint(n_ops)] = 0
        if k == "bad op":
            ops[rng.randint(n_ops)] = 9 + rng.randint(7)
        lens = rng.randint(1, 30, n_ops)
        q = int(lens[np.isin(ops, QUERY)].sum())
        # the reference bases the strand-ordered walk covers: up to its last match run
        strand_rev = bool(rng.randint(2))
        o, ln = (ops[::-1], lens[::-1]) if strand_rev else (ops, lens)
        m = np.nonzero(np.isin(o, MATCH))[0]
        r = int(ln[: m[-1] + 1][np.isin(o[: m[-1] + 1], REF)].sum()) if m.size else 5
        nb = max(q, 1)
        stride = int(rng.randint(1, 7))
        moves = 2 * nb + int(rng.randint(5))
        tab = np.zeros(moves, np.int8)
        tab[np.sort(rng.choice(2 * nb, nb, replace=False))] = 1
        sl = moves * stride + int(rng.randint(stride))
        ql, rl = nb, r
        if k == "one base short":
            ql -= 1
        elif k == "signal short":
            sl -= stride + 3
        elif k == "bad stride":
            stride = -int(rng.randint(0, 3))
        elif k == "no reference":
            rl = -1
        elif k == "reference short":
            rl = max(r - 1 - int(rng.randint(3)), 0) if rng.randint(2) else r + 1 + int(rng.randint(3))
        if k != "no moves":
            mv.extend([stride] + tab.tolist())
        mv_off.append(len(mv))
        sig_len.append(sl)
        seq_len.append(ql)
        cigar.extend(((lens.astype(np.int64) << 4) | ops).tolist())
        cigar_off.append(len(cigar))
        rev.append(strand_rev)
        ref_len.append(rl)
        kind.append(k)
    return (np.asarray(mv, np.int8), np.asarray(mv_off, np.int64), np.asarray(sig_len, np.int64), np.asarray(seq_len, np.int64),
            np.asarray(cigar, np.uint32), np.asarray(cigar_off, np.int64), np.asarray(rev, np.uint8), np.asarray(ref_len, np.int64)), kind


def test_reverse_anchor_batch_equals_the_per_read_composition_on_random_records():
    from remora_amd import _lib as L

    rng = np.random.RandomState(17)
    args, kind = _random_records(rng, 400)
    mv, mv_off, sig_len, seq_len, cigar, cigar_off, rev, ref_len = args
    seen = {}
    for reverse_signal, threads in ((1, 1), (1, 5), (0, 3)):
        status, r2s, r2s_off = _anchor(L, "rmr_ref_anchor_batch_dir", *args, reverse_signal, threads)
        for i in range(len(kind)):
            want_st, want = _expected(L, mv[mv_off[i] : mv_off[i + 1]], int(sig_len[i]), int(seq_len[i]), cigar[cigar_off[i] : cigar_off[i + 1]],
                                      bool(rev[i]), int(ref_len[i]), reverse_signal)
            assert status[i] == want_st, (kind[i], i, reverse_signal, int(status[i]), want_st)
            if want_st == 0:
                assert np.array_equal(r2s[r2s_off[i] : r2s_off[i + 1]], want), (kind[i], i, reverse_signal)
            if reverse_signal:
                seen[(want_st, bool(rev[i]))] = seen.get((want_st, bool(rev[i])), 0) + 1
    # every status the per-read path can end in, on both strands, and enough anchored records for the comparison to mean something
    for st in (0, 1, 2, 3, 8, 9, ERR_INVALID, L.ERR_DISCORDANT_SEQ, L.ERR_DISCORDANT_SIG):
        assert seen.get((st, False), 0) and seen.get((st, True), 0), (st, seen)
    assert seen[(0, False)] + seen[(0, True)] >= 2 * 200
    # direction 0 is the old entry
    old = _anchor(L, "rmr_ref_anchor_batch", *args, 2)
    new = _anchor(L, "rmr_ref_anchor_batch_dir", *args, 0, 2)
    assert np.array_equal(old[0], new[0])
    for i in np.nonzero(old[0] == 0)[0]:
        assert np.array_equal(old[1][old[2][i] : old[2][i + 1]], new[1][new[2][i] : new[2][i + 1]])
    # reversed coordinates are another mapping, not the forward one again
    fwd, rvs = new, _anchor(L, "rmr_ref_anchor_batch_dir", *args, 1, 2)
    assert any(not np.array_equal(fwd[1][fwd[2][i] : fwd[2][i + 1]], rvs[1][rvs[2][i] : rvs[2][i + 1]]) for i in np.nonzero(fwd[0] == 0)[0])


def test_reverse_anchor_batch_on_the_reference_test_alignments():
    """The reference's own aligned reads (both test BAMs, both strands), signal lengths any the move tables allow."""
    from remora_amd import _lib as L
    from remora_amd import io as rio

    checked = 0
    for name in ("can_mappings.bam", "mod_mappings.bam"):
        rb = next(iter(rio.iter_bam_raw_batches(os.path.join(DATA, name), want_ref=True, batch=64)))[0]
        n = rb.n
        mv_len = np.diff(rb.mv_off)
        stride = np.array([int(rb.mv[rb.mv_off[i]]) if mv_len[i] else 1 for i in range(n)])
        sig_len = ((mv_len - 1) * stride + 3).astype(np.int64)
        seq_len = np.diff(rb.seq_off).astype(np.int64)
        rev = np.ascontiguousarray((rb.flag & 16) != 0, np.uint8)
        ref_len = np.where((rb.ref_ok != 0) & (rb.ref_id >= 0), np.diff(rb.refseq_off), -1).astype(np.int64)
        mv_off, cigar, cigar_off = (np.ascontiguousarray(rb.mv_off, np.int64), np.ascontiguousarray(rb.cigar, np.uint32),
                                    np.ascontiguousarray(rb.cigar_off, np.int64))
        status, r2s, r2s_off = _anchor(L, "rmr_ref_anchor_batch_dir", rb.mv, mv_off, sig_len, seq_len, cigar, cigar_off, rev, ref_len, 1, 4)
        for i in range(n):
            want_st, want = _expected(L, rb.mv[mv_off[i] : mv_off[i + 1]], int(sig_len[i]), int(seq_len[i]), cigar[cigar_off[i] : cigar_off[i + 1]],
                                      bool(rev[i]), int(ref_len[i]), True)
            assert status[i] == want_st, (name, i)
            if want_st == 0:
                assert np.array_equal(r2s[r2s_off[i] : r2s_off[i + 1]], want), (name, i)
                checked += 1
        assert rev.any() and not rev.all()
    assert checked >= 20
