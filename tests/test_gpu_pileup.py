"""`analyze pileup_modbams` on the GPU against a plain-Python restatement written here: modbam_restate.modified_bases, then
aligned_pairs, then dictionaries of integer counts.  Every comparison is exact - equal integers, equal file bytes; nothing
here has a tolerance.  The flush and merge kernels are also driven directly through the C ABI on hand-made word arrays."""
import ctypes
import logging
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import modbam_restate as mr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, "data")
REFS = [("ctgA", 2000), ("ctgB", 2000)]
ALPHABET = ["C", "h", "m"]
SKIP_TEXT = {1: "no MM tag", 2: "malformed modified-base tags", 3: "unmapped", 5: "no modified base of the alphabet",
             6: "secondary or supplementary"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def record_calls(rec, alphabet):
    """(status, [(ref_id, pos, strand, class, kmax)]) of one record by the rules of the pileup."""
    mods = list(alphabet[1:])
    reverse = bool(rec["flag"] & 0x10)
    if rec["mm"] is None:
        return 1, []
    try:
        mr.parse_mm_ml(rec["mm"], rec["ml"])
    except mr.Malformed:
        return 2, []
    if rec["ref_id"] < 0 or rec["flag"] & 0x4:
        return 3, []
    if rec["flag"] & 0x900:
        return 6, []
    try:
        mb = mr.modified_bases(rec["seq"], reverse, rec["mm"], rec["ml"])
        ok = True
    except mr.Malformed:
        mb, ok = None, False
    # does any entry count?  (asked of the entries, before their calls are looked at)
    entries = mr.parse_mm_ml(rec["mm"], rec["ml"])
    if not any(strand == "+" and any(c in mods for c in codes) for _, strand, codes, _, _, _ in entries):
        return 5, []
    if sum(n for op, n in rec["cigar"] if op in "MIS=X") != len(rec["seq"]) or not ok:
        return 2, []
    called = {}
    for (_, strand_key, code), items in mb.items():  # '+' entries carry the strand of the record
        if strand_key != int(reverse) or code not in mods:
            continue
        for p, q in items:
            called.setdefault(p, {})[code] = 2 * q + 1  # 512 p; the later entry wins
    q2r = {q: r for q, r, _ in mr.aligned_pairs(rec["cigar"], rec["pos"]) if q is not None and r is not None}
    out = []
    for p in sorted(called):
        r = q2r.get(p)
        if r is None:
            continue
        ks = [called[p].get(m, 0) for m in mods]
        cols = [512 - sum(ks)] + ks
        cls = int(np.argmax(cols))
        out.append((rec["ref_id"], r, int(reverse), cls, cols[cls]))
    return 0, out


def in_region(call, region):
    return region is None or (call[0] == region[0] and region[1] <= call[1] < region[2])


def restate(records, alphabet, k_t=None, pct=None, region=None):
    """-> (table {(ref_id, pos, strand): [counts]}, k_t, histogram, statuses)."""
    calls, statuses = [], []
    for rec in records:
        st, cs = record_calls(rec, alphabet)
        statuses.append(st)
        calls += [c for c in cs if in_region(c, region)]
    hist = np.bincount([c[4] for c in calls], minlength=513) if calls else np.zeros(513, np.int64)
    if k_t is None:
        allowed = (Fraction(len(calls)) * Fraction(str(pct)) / 100).__floor__()
        k_t = max(k for k in range(514) if int(hist[:k].sum()) <= allowed)
    ncol = len(alphabet) + 1
    table = {}
    for rid, pos, strand, cls, kmax in calls:
        table.setdefault((rid, pos, strand), [0] * ncol)[cls if kmax >= k_t else ncol - 1] += 1
    return table, k_t, hist, statuses


def bed_text(table, alphabet, refs, min_coverage=1):
    out = []
    for (rid, pos, strand), row in sorted(table.items()):
        nv = sum(row[:-1])
        if nv < max(min_coverage, 1):
            continue
        for j, code in enumerate(alphabet[1:]):
            out.append(f"{refs[rid][0]}\t{pos}\t{pos + 1}\t{code}\t{min(nv, 1000)}\t{'+-'[strand]}\t{pos}\t{pos + 1}\t255,0,0\t{nv}\t"
                       f"{100 * row[1 + j] / nv:.2f}\n")
    return "".join(out)


def tsv_text(table, alphabet, refs):
    head = "\t".join(["chrom", "start", "strand"] + [f"N_{a}" for a in alphabet] + ["N_fail"]) + "\n"
    return head + "".join(f"{refs[rid][0]}\t{pos}\t{'+-'[strand]}\t" + "\t".join(map(str, row)) + "\n"
                          for (rid, pos, strand), row in sorted(table.items()))


def files_of(table, tmp_path, tag, min_coverage=1):
    from remora_amd.pileup import write_bedmethyl, write_counts

    bed, tsv = tmp_path / f"{tag}.bed", tmp_path / f"{tag}.tsv"
    write_bedmethyl(table, bed, min_coverage=min_coverage)
    write_counts(table, tsv)
    return bed.read_text(), tsv.read_text()


def same_table(got, want, alphabet):
    keys = sorted(want)
    assert got.pos.size == len(keys)
    assert got.ref_id.dtype == np.int32 and got.pos.dtype == np.int64 and got.strand.dtype == np.uint8 and got.counts.dtype == np.int64
    assert list(zip(got.ref_id.tolist(), got.pos.tolist(), got.strand.tolist())) == keys
    assert got.counts.shape == (len(keys), len(alphabet) + 1) and got.counts.tolist() == [want[k] for k in keys]
    assert got.n_calls == sum(sum(r) for r in want.values())


# ---- goldens: BAM files read back into records for the restatement --------------------------------------------------------------
def records_of_bam(path):
    """The records of a BAM file as the restatement takes them, through the pure-Python reader."""
    from remora_amd.io import _iter_bam_records_py

    out = []
    for r in _iter_bam_records_py(path):
        tags = dict(r.tags)
        mm, ml = tags.get("MM", tags.get("Mm")), tags.get("ML", tags.get("Ml"))
        out.append(dict(seq=r.query_sequence, flag=int(r.flag), ref_id=int(r.reference_id), pos=int(r.reference_start),
                        cigar=[("MIDNSHP=X"[op], n) for op, n in r.cigartuples], mm=mm, ml=None if ml is None else [int(x) for x in ml],
                        has_md="MD" in tags))
    return out


@pytest.mark.parametrize("name,alphabet", [("mod_modbam.bam", ["C", "h", "m"]), ("can_modbam.bam", ["C", "m"])])
def test_goldens_equal_the_restatement(torch_cuda, tmp_path, name, alphabet):
    from remora_amd.pileup import bam_reference_dict, pileup_modbams

    path = os.path.join(DATA, name)
    recs, refs = records_of_bam(path), bam_reference_dict(path)
    assert len(recs) > 0 and any(r["mm"] for r in recs)
    for tag, kw in (("thr0", dict(filter_threshold=0, pct_filt=None)), ("pct10", dict(pct_filt=10))):
        want, k_t, hist, _ = restate(recs, alphabet, k_t=0 if tag == "thr0" else None, pct=10)
        assert len(want) > 0
        got = pileup_modbams(path, alphabet, **kw)
        assert got.threshold_k == k_t
        same_table(got, want, alphabet)
        bed, tsv = files_of(got, tmp_path, tag)
        assert bed == bed_text(want, alphabet, refs) and tsv == tsv_text(want, alphabet, refs)
        if tag == "pct10":
            assert np.array_equal(got.hist, hist)


# ---- synthetic depth ------------------------------------------------------------------------------------------------------------
def _rec(seq, cigar, mm, ml, flag=0, ref=0, pos=0, has_md=True):
    return dict(seq=seq, flag=flag, ref_id=ref, ref_name=REFS[ref][0] if ref >= 0 else None, pos=pos, cigar=cigar, mm=mm, ml=ml, has_md=has_md)


def _all_c(seq, reverse):
    """How many C the original sequence has."""
    return seq.count("G") if reverse else seq.count("C")


def _synthetic():
    """About 60 records over two contigs of 2 kb, both strands: reads cut from the contigs (so that calls of several reads
    meet on one reference position), every C called for h and m with seeded ML values, and one record per edge case."""
    rng = np.random.default_rng(17)
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    genome = [rand(2000), rand(2000)]
    ml = lambda n: rng.integers(0, 256, n).tolist()  # noqa: E731

    def confident(n):  # (h, m) pairs: mostly one clear class, some undecided
        out = []
        for kind in rng.integers(0, 4, n):
            lo, hi = int(rng.integers(0, 40)), int(rng.integers(150, 256))
            out += [[lo, hi], [hi, lo], [lo, lo // 2], [int(rng.integers(60, 110)), int(rng.integers(60, 110))]][kind]
        return out

    recs = []
    for i in range(44):
        ref, rev = i % 2, (i // 2) % 2 == 1
        n = int(rng.integers(700, 1300))
        pos = int(rng.integers(0, 2000 - n))
        seq = genome[ref][pos : pos + n]
        nc = _all_c(seq, rev)
        flag_char = "?" if i % 3 else "."
        recs.append(_rec(seq, [("M", n)], f"C+hm{flag_char}" + ",0" * nc + ";", confident(nc), flag=16 if rev else 0, ref=ref, pos=pos,
                         has_md=i % 5 != 0))
    g = genome[0]
    # exactly 256 bases: one round of the walk
    recs.append(_rec(g[100:356], [("M", 256)], "C+m?" + ",0" * g[100:356].count("C") + ";", ml(g[100:356].count("C")), pos=100))
    # more than 256 CIGAR operations
    s = rand(350)
    recs.append(_rec(s, [("M", 2), ("I", 1), ("M", 2), ("D", 1)] * 70, "C+m?" + ",0" * s.count("C") + ";", ml(s.count("C")), pos=900))
    # calls under a soft clip and inside an insertion: dropped
    recs.append(_rec("C" * 55, [("S", 5), ("M", 20), ("I", 6), ("M", 20), ("S", 4)], "C+m?" + ",0" * 55 + ";", ml(55), pos=300))
    # a deletion across reference positions that other reads list
    recs.append(_rec(g[500:530] + g[535:565], [("M", 30), ("D", 5), ("M", 30)], "C+m?" + ",0" * (g[500:530] + g[535:565]).count("C") + ";",
                     ml((g[500:530] + g[535:565]).count("C")), pos=500))
    # an N entry: positions counted over every base
    recs.append(_rec(g[600:800], [("M", 200)], "N+m?,0,5,2,189;", ml(4), pos=600))
    recs.append(_rec(g[600:800], [("S", 3), ("M", 197)], "N+h?,0,5,2,189;", ml(4), flag=16, ref=1, pos=650))
    # two entries give one code at one position (the later wins); h and m from two entries on one base
    recs.append(_rec("C" * 30, [("M", 30)], "C+h?,0,1;C+m?,0,1;C+m?,2;", [10, 20, 30, 40, 250], pos=1200))
    # a ChEBI entry and a '-'-strand entry: ignored, their ML consumed
    recs.append(_rec(g[700:900], [("M", 200)], "C+76792,4;G-m,3,1;C+m.,0,2;", ml(5), pos=700))
    # skipped whole: malformed MM, ML too short, unmapped, secondary, supplementary, no tags, nothing of the alphabet
    recs.append(_rec(g[0:100], [("M", 100)], "C+m?,x;", [1], pos=0))
    recs.append(_rec(g[0:100], [("M", 100)], "C+m?,1,1;", [5], pos=0))
    recs.append(_rec(g[0:100], [], "C+m?,0;", [200], flag=4, ref=-1, pos=-1))
    recs.append(_rec(g[0:100], [("M", 100)], "C+m?,0;", [200], flag=0x100, pos=0))
    recs.append(_rec(g[0:100], [("M", 100)], "C+m?,0;", [200], flag=0x800 | 16, pos=0))
    recs.append(_rec(g[0:100], [("M", 100)], None, None, pos=0))
    recs.append(_rec(g[0:100], [("M", 100)], "G-m,3,1;", ml(2), pos=0))
    recs.append(_rec(g[0:100], [("M", 99)], "C+m?,0;", [200], pos=0))  # CIGAR shorter than the read
    # the last base of a contig, reverse strand
    recs.append(_rec(genome[1][1900:2000], [("M", 100)], "C+m?" + ",0" * genome[1][1900:2000].count("G") + ";", ml(genome[1][1900:2000].count("G")),
                     flag=16, ref=1, pos=1900))
    return recs, genome


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    recs, genome = _synthetic()
    d = tmp_path_factory.mktemp("pileup")
    path = str(d / "synth.bam")
    mr.write_bam(path, REFS, recs)
    return path, recs, genome, d


def test_synthetic_input_is_not_vacuous(synth):
    """Asked of the restatement alone, before anything runs on the GPU."""
    _, recs, genome, _ = synth
    table, k_t, hist, statuses = restate(recs, ALPHABET, pct=10)
    assert 55 <= len(recs) <= 70
    assert sum(1 for row in table.values() if sum(row) >= 5) >= 50
    for rid in (0, 1):
        for strand in (0, 1):
            assert any(k[0] == rid and k[2] == strand for k in table), (rid, strand)
    assert sum(row[-1] for row in table.values()) >= 1
    assert sum(1 for row in table.values() if sum(1 for c in row[:-1] if c) > 1) >= 1  # a site whose class differs between reads
    assert any(len(r["seq"]) > 256 for r in recs) and any(len(r["seq"]) == 256 for r in recs) and any(len(r["cigar"]) > 256 for r in recs)
    clip = next(r for r in recs if r["cigar"][0] == ("S", 5))
    assert len(record_calls(clip, ALPHABET)[1]) == 40  # 55 calls listed, 9 under the clips and 6 in the insertion dropped
    dele = next(r for r in recs if ("D", 5) in r["cigar"])
    deleted = [k for k in table if k[0] == 0 and k[2] == 0 and 530 <= k[1] < 535]
    assert deleted and not any(530 <= c[1] < 535 for c in record_calls(dele, ALPHABET)[1])
    mms = [r["mm"] or "" for r in recs]
    assert any("?" in m for m in mms) and any("C+hm." in m for m in mms) and any(m.startswith("N+") for m in mms)
    assert any("76792" in m for m in mms) and any("G-m" in m for m in mms) and any(not r["has_md"] and record_calls(r, ALPHABET)[1] for r in recs)
    twice = next(r for r in recs if r["mm"] == "C+h?,0,1;C+m?,0,1;C+m?,2;")
    assert [c[3:] for c in record_calls(twice, ALPHABET)[1]] == [(0, 512 - 21 - 61), (2, 501)]  # m of the third C: 250, not 40
    assert statuses.count(2) == 3 and statuses.count(3) == 1 and statuses.count(6) == 2 and statuses.count(1) == 1 and statuses.count(5) == 1
    assert any(k[0] == 1 and k[2] == 1 and k[1] >= 1990 for k in table)  # near the contig's end
    assert 0 < k_t < 512 and hist.sum() == sum(sum(r) for r in table.values())


def test_synthetic_depth_equals_the_restatement(torch_cuda, synth, tmp_path, caplog):
    from remora_amd.pileup import pileup_modbams

    path, recs, _, _ = synth
    want, k_t, hist, statuses = restate(recs, ALPHABET, pct=10)
    with caplog.at_level(logging.INFO, logger="Remora"):
        got = pileup_modbams(path, ALPHABET, pct_filt=10)
    assert got.threshold_k == k_t and np.array_equal(got.hist, np.asarray(hist, np.int64))
    same_table(got, want, ALPHABET)
    bed, tsv = files_of(got, tmp_path, "synth")
    assert bed == bed_text(want, ALPHABET, REFS) and tsv == tsv_text(want, ALPHABET, REFS)
    bed3, _ = files_of(got, tmp_path, "synth3", min_coverage=3)
    assert bed3 == bed_text(want, ALPHABET, REFS, min_coverage=3) and 0 < len(bed3) < len(bed)
    text = [r.getMessage() for r in caplog.records]
    assert sum("Reverse strand (duplex) mods not supported" in t for t in text) == 1
    assert sum("Modified base found in BAM (76792)" in t for t in text) == 1
    for st in (1, 2, 3, 5, 6):
        line = f"{statuses.count(st)} of {len(recs)} records skipped: {SKIP_TEXT[st]} ({path})"
        assert text.count(line) == 1, line


# ---- threshold edges ------------------------------------------------------------------------------------------------------------
def test_threshold_edges(torch_cuda, synth, tmp_path):
    from remora_amd.pileup import pileup_modbams

    path, recs, _, _ = synth
    one = str(tmp_path / "one.bam")
    mr.write_bam(one, REFS, [_rec("ACGT", [("M", 4)], "C+m?,0;", [200], pos=10)])  # k_m = 401, column 0 = 111
    at = pileup_modbams(one, ["C", "m"], filter_threshold=Fraction(401, 512), pct_filt=None)
    assert at.threshold_k == 401 and at.counts.tolist() == [[0, 1, 0]] and (at.ref_id[0], at.pos[0], at.strand[0]) == (0, 11, 0)
    above = pileup_modbams(one, ["C", "m"], filter_threshold=Fraction(402, 512), pct_filt=None)
    assert above.threshold_k == 402 and above.counts.tolist() == [[0, 0, 1]]
    for pct in (0, 10, 50, 100):
        want, k_t, hist, _ = restate(recs, ALPHABET, pct=pct)
        got = pileup_modbams(path, ALPHABET, pct_filt=pct)
        assert got.threshold_k == k_t and np.array_equal(got.hist, hist)
        same_table(got, want, ALPHABET)
        n_fail = int(got.counts[:, -1].sum())
        assert n_fail <= got.n_calls * pct // 100 and n_fail == int(hist[:k_t].sum())
    assert pileup_modbams(path, ALPHABET, pct_filt=100).counts[:, :-1].sum() == 0
    # every call has one kmax: the tie filters nothing
    tie = str(tmp_path / "tie.bam")
    mr.write_bam(tie, REFS, [_rec("C" * 40, [("M", 40)], "C+m?" + ",0" * 40 + ";", [180] * 40, pos=5 * i) for i in range(6)])
    got = pileup_modbams(tie, ["C", "m"], pct_filt=10)
    assert got.threshold_k == 361 and got.counts[:, -1].sum() == 0 and got.counts[:, 1].sum() == 240 and got.counts[:, 1].max() == 6


# ---- budget and batch independence ----------------------------------------------------------------------------------------------
def test_buffer_batch_and_file_split_do_not_matter(torch_cuda, synth, tmp_path):
    from remora_amd.pileup import pileup_modbams

    path, recs, _, d = synth
    whole = pileup_modbams(path, ALPHABET, filter_threshold=0.6, pct_filt=None)
    assert whole.n_flushes == 1
    ref_files = files_of(whole, tmp_path, "whole")
    for batch in (1, 7, 512):
        got = pileup_modbams(path, ALPHABET, filter_threshold=0.6, pct_filt=None, batch=batch)
        assert files_of(got, tmp_path, f"b{batch}") == ref_files
    got = pileup_modbams(path, ALPHABET, filter_threshold=0.6, pct_filt=None, buffer_calls=64)
    assert got.n_flushes > 1 and got.n_flushes == -(-got.n_calls // 64) and files_of(got, tmp_path, "c64") == ref_files
    # a buffer of one call on a smaller input (a flush per call): deep sites straddle many flushes
    small = str(tmp_path / "small.bam")
    mr.write_bam(small, REFS, recs[:4] + recs[44:52])
    a = pileup_modbams(small, ALPHABET, filter_threshold=0.6, pct_filt=None)
    assert a.n_flushes == 1 and a.counts.sum(axis=1).max() >= 2
    small_files = files_of(a, tmp_path, "small")
    for cap in (64, 1):
        got = pileup_modbams(small, ALPHABET, filter_threshold=0.6, pct_filt=None, buffer_calls=cap)
        assert got.n_flushes == -(-got.n_calls // cap) > 1 and files_of(got, tmp_path, f"small{cap}") == small_files
        assert got.peak_device_bytes < a.peak_device_bytes
    # two files piled into one table: the bytes of their concatenation, in either order; the percentile is taken over both
    p1, p2 = str(tmp_path / "half1.bam"), str(tmp_path / "half2.bam")
    mr.write_bam(p1, REFS, recs[:25])
    mr.write_bam(p2, REFS, recs[25:])
    by_pct = files_of(pileup_modbams(path, ALPHABET, pct_filt=10), tmp_path, "pct")
    for tag, order in (("ab", [p1, p2]), ("ba", [p2, p1])):
        assert files_of(pileup_modbams(order, ALPHABET, filter_threshold=0.6, pct_filt=None), tmp_path, tag) == ref_files
        assert files_of(pileup_modbams(order, ALPHABET, pct_filt=10), tmp_path, tag + "pct") == by_pct


# ---- the flush and merge kernels through the C ABI ----------------------------------------------------------------------------
def word(ref_id, pos, strand, code):
    return (int(ref_id) << 36) | (int(pos) << 5) | (int(strand) << 4) | int(code)


class Pile:
    def __init__(self, n_contigs, n_alpha, cap, max_len=1 << 31):
        from remora_amd.engine import get_engine
        from remora_amd.pileup import DevicePileup

        self.eng = get_engine(None)
        self.p = DevicePileup(self.eng, n_contigs, max_len, n_alpha, cap)

    def add(self, words):
        import torch

        if len(words):
            t = torch.from_numpy(np.asarray(words, np.uint64).view(np.int64)).to(self.eng.torch_device)
            self.p.add(t, t.numel())
            self.eng.synchronize()

    def table(self):
        n_sites, n_calls, n_flushes, peak = self.p.finish()
        keys, counts = self.p.read(n_sites)
        return keys, counts, n_calls, n_flushes


def want_table(words, ncol):
    words = np.asarray(words, np.uint64)
    keys = np.unique(words >> np.uint64(4))
    counts = np.zeros((keys.size, ncol), np.uint32)
    np.add.at(counts, (np.searchsorted(keys, words >> np.uint64(4)), (words & np.uint64(15)).astype(np.int64)), 1)
    return keys, counts


def _words(kind, n, n_alpha, rng):
    ncol = n_alpha + 1
    code = rng.integers(0, ncol, n)
    if kind == "one_site":
        return [word(3, 77, 1, c) for c in code]
    if kind == "own_site":
        return [word(i % 5, 10 + i // 5, 0, c) for i, c in zip(rng.permutation(n), code)]
    site = rng.integers(0, max(n // 4, 1), n)
    return [word(s % 3, s // 3, s % 2, c) for s, c in zip(site, code)]


@pytest.mark.parametrize("n_alpha", [2, 8])
@pytest.mark.parametrize("kind", ["random", "one_site", "own_site"])
def test_flush_kernels_on_hand_made_words(torch_cuda, kind, n_alpha):
    rng = np.random.default_rng(11)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 70000):
        words = _words(kind, n, n_alpha, rng)
        for cap in ((max(n, 1),) if n < 70000 else (70000, 4096)):
            pile = Pile(5, n_alpha, cap)
            try:
                pile.add(words)
                keys, counts, n_calls, n_flushes = pile.table()
            finally:
                pile.p.close()
            wk, wc = want_table(words, n_alpha + 1) if n else (np.zeros(0, np.uint64), np.zeros((0, n_alpha + 1), np.uint32))
            assert n_calls == n and n_flushes == -(-n // cap), (n, cap)
            assert np.array_equal(keys, wk) and np.array_equal(counts, wc), (kind, n, cap)
            if kind == "one_site" and n:
                assert keys.size == 1 and counts.sum() == n
            if kind == "own_site":
                assert keys.size == n


def test_flush_holds_the_largest_ref_id_and_position(torch_cuda):
    top_ref, top_pos = (1 << 24) - 1, (1 << 31) - 1
    words = [word(top_ref, top_pos, 1, 8), word(top_ref, top_pos, 0, 0), word(0, 0, 0, 1), word(top_ref, top_pos, 1, 8), word(top_ref, 0, 1, 2),
             word(0, top_pos, 1, 3)]
    pile = Pile(1 << 24, 8, 16)
    try:
        pile.add(words)
        keys, counts, _, _ = pile.table()
    finally:
        pile.p.close()
    wk, wc = want_table(words, 9)
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc) and int(keys[-1]) == (top_ref << 32) | (top_pos << 1) | 1 and counts[-1, 8] == 2


@pytest.mark.parametrize("case", ["all_hits", "all_misses_interleaved", "all_before", "all_after", "mixed"])
def test_merge_into_the_resident_table(torch_cuda, case):
    rng = np.random.default_rng(23)
    first = [word(1, p, p % 2, c) for p in range(1000, 1600, 2) for c in rng.integers(0, 4, 3)]
    pos = {"all_hits": range(1000, 1600, 2), "all_misses_interleaved": range(1001, 1601, 2), "all_before": range(0, 700),
           "all_after": range(1600, 2300), "mixed": range(900, 1700)}[case]
    second = [word(1, p, p % 2, c) for p in pos for c in rng.integers(0, 4, 2)]
    if case == "all_before":
        second += [word(0, 5000, 1, 3)]
    if case == "all_after":
        second += [word(2, 0, 0, 0)]
    pile = Pile(3, 3, 4096)
    try:
        pile.add(first)
        k1, c1, _, f1 = pile.table()  # the first flush: the table is resident from here on
        assert f1 == 1 and np.array_equal(k1, want_table(first, 4)[0])
        pile.add(second)
        keys, counts, n_calls, n_flushes = pile.table()
        third = [word(1, 1000, 0, 3)] * 5  # and once more into the merged table
        pile.add(third)
        keys3, counts3, _, _ = pile.table()
    finally:
        pile.p.close()
    wk, wc = want_table(first + second, 4)
    assert n_flushes == 2 and n_calls == len(first) + len(second)
    assert np.array_equal(keys, wk) and np.array_equal(counts, wc)
    if case == "all_hits":
        assert keys.size == k1.size
    if case == "all_misses_interleaved":
        assert keys.size == 2 * k1.size
    wk3, wc3 = want_table(first + second + third, 4)
    assert np.array_equal(keys3, wk3) and np.array_equal(counts3, wc3)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(torch_cuda, synth, tmp_path):
    from remora_amd import RemoraError
    from remora_amd import _lib as L
    from remora_amd.engine import get_engine
    from remora_amd.pileup import pileup_modbams, write_bedmethyl

    path, recs, _, _ = synth
    other = str(tmp_path / "other.bam")
    mr.write_bam(other, [("ctgA", 2000), ("ctgB", 2001)], recs[:2])
    eng = get_engine(None)
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        with pytest.raises(RemoraError, match="either --filter-threshold or --pct-filt"):
            pileup_modbams(path, ALPHABET, filter_threshold=0.5, pct_filt=10)
        with pytest.raises(RemoraError, match="1 to 7 distinct single-letter modified bases"):
            pileup_modbams(path, ["C"] + list("abdefghm"), pct_filt=10)
        with pytest.raises(RemoraError, match=r"differ at contig #1: ctgB \(2000 bases\) against ctgB \(2001 bases\)"):
            pileup_modbams([path, other], ALPHABET, pct_filt=10)
        with pytest.raises(RemoraError, match="does not have"):
            pileup_modbams(path, ALPHABET, pct_filt=10, region="ctgZ:1-5")
        h = ctypes.c_void_p()
        lib = L.lib()
        assert lib.rmr_pileup_create(eng.handle, (1 << 24) + 1, 1000, 3, 64, ctypes.byref(h)) != 0 and not h
        assert b"24 bits" in lib.rmr_last_error()
        assert lib.rmr_pileup_create(eng.handle, 3, (1 << 31) + 1, 3, 64, ctypes.byref(h)) != 0 and not h
        assert b"31 bits" in lib.rmr_last_error()
        assert lib.rmr_pileup_create(eng.handle, 3, 1000, 9, 64, ctypes.byref(h)) != 0 and not h
        assert not any(k.startswith(("pileup_", "modbam_")) for k in eng.profile()), eng.profile()
        # no call is kept: known only after the emit has counted - a message, no flush, no file
        none = str(tmp_path / "none.bam")
        mr.write_bam(none, REFS, [_rec("C" * 30, [("S", 30)], "C+m?,0;", [1], pos=5), _rec("C" * 30, [("M", 30)], "C+a?,0;", [1], pos=5)])
        bed = tmp_path / "none.bed"
        for kw in (dict(pct_filt=10), dict(filter_threshold=0, pct_filt=None), dict(pct_filt=10, region="ctgB")):
            with pytest.raises(RemoraError, match="No modified-base call"):
                write_bedmethyl(pileup_modbams(none, ["C", "m"], **kw), bed)
        assert not bed.exists() and "pileup_flush" not in eng.profile()
    finally:
        eng.profile_enable(False)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_api_bytes(torch_cuda, synth, tmp_path):
    from remora_amd.pileup import pileup_modbams

    path, recs, _, _ = synth
    base = [sys.executable, "-m", "remora_amd", "analyze", "pileup_modbams", "--bam", path, "--canonical-base", "C", "--mod-bases", "h", "m"]
    runs = {"a": [], "b": [], "r": ["--region", "ctgB:400-1500", "--min-coverage", "2", "--reads-per-batch", "7"]}
    procs = {t: subprocess.Popen(base + ["--out-bed", str(tmp_path / f"{t}.bed"), "--counts-filename", str(tmp_path / f"{t}.tsv")] + extra,
                                 cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for t, extra in runs.items()}
    for t, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err
    read = lambda t: ((tmp_path / f"{t}.bed").read_text(), (tmp_path / f"{t}.tsv").read_text())  # noqa: E731
    assert read("a") == files_of(pileup_modbams(path, ALPHABET), tmp_path, "api")  # the default: --pct-filt 10
    assert read("b") == read("a")
    want, k_t, _, _ = restate(recs, ALPHABET, pct=10, region=(1, 400, 1500))
    assert 0 < len(want) and all(k[0] == 1 and 400 <= k[1] < 1500 for k in want)
    assert read("r") == (bed_text(want, ALPHABET, REFS, min_coverage=2), tsv_text(want, ALPHABET, REFS))


def test_command_line_refuses_both_thresholds(torch_cuda, synth, tmp_path, capsys):
    from remora_amd.__main__ import main

    rc = main(["analyze", "pileup_modbams", "--bam", synth[0], "--canonical-base", "C", "--mod-bases", "h", "m", "--out-bed", str(tmp_path / "x.bed"),
               "--filter-threshold", "0.5", "--pct-filt", "10"])
    assert rc == 1 and "either --filter-threshold or --pct-filt" in capsys.readouterr().err and not (tmp_path / "x.bed").exists()
