"""`analyze pileup_modbams --duplex / --hemi` on the GPU against the plain-Python restatement of test_host_pileup_duplex.py, on
its synthetic input: the '-'-strand entries on the effective strand (without a reference, with motifs, folded), the strand
pairs per motif site, the pair kernels and the 16-column table driven directly through the C ABI on hand-made word arrays, and
the command line.  Every comparison is exact - equal integers, equal file bytes."""
import ctypes
import logging
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import modbam_restate as mr
import test_gpu_pileup as tp
import test_gpu_pileup_ref as tgr
import test_host_pileup_duplex as hd
from conftest import ROOT

pytestmark = pytest.mark.gpu

REFS, ALPHABET = tp.REFS, ["C", "h", "m"]
K307 = Fraction(307, 512)
HEMI_CASES = {"CG_m": (hd.CG, ["C", "m"]), "CG_hm": (hd.CG, ["C", "h", "m"]), "GC_m": (hd.GC, ["C", "m"]), "GATC_a": (hd.GATC, ["A", "a"])}
THRESHOLDS = {"k307": (dict(filter_threshold=K307, pct_filt=None), dict(k_t=307)), "pct10": (dict(pct_filt=10), dict(pct=10))}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def duplex_input(tmp_path_factory):
    recs, genome, planted = hd.synth()
    d = tmp_path_factory.mktemp("pileup_duplex")
    bam, fa = str(d / "duplex.bam"), str(d / "genome.fa")
    mr.write_bam(bam, REFS, recs)
    with open(fa, "w") as fh:
        fh.write(tgr.fasta_text([(name, seq) for (name, _), seq in zip(REFS, genome)], 60))
    return bam, fa, recs, genome, planted


@pytest.fixture(scope="module")
def device_genome(torch_cuda, duplex_input):
    from remora_amd.pileup import RefGenome

    with RefGenome.from_fasta(duplex_input[1], [n for n, _ in REFS], [ln for _, ln in REFS]) as g:
        yield g


# ---- 1. --duplex without a reference ------------------------------------------------------------------------------------------
def test_duplex_entries_lie_on_the_effective_strand(torch_cuda, duplex_input, tmp_path, caplog):
    from remora_amd.pileup import pileup_modbams

    bam, _, recs, _, _ = duplex_input
    for tag, (kw, rkw) in THRESHOLDS.items():
        want, k_t, hist, statuses = hd.restate(recs, ALPHABET, **rkw)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="Remora"):
            got = pileup_modbams(bam, ALPHABET, duplex=True, **kw)
        assert got.threshold_k == k_t and not got.hemi and got.n_unpaired is None and not got.combined
        tp.same_table(got, want, ALPHABET)
        assert tp.files_of(got, tmp_path, "d" + tag) == (tp.bed_text(want, ALPHABET, REFS), tp.tsv_text(want, ALPHABET, REFS))
        text = [r.getMessage() for r in caplog.records]
        assert not any("Reverse strand (duplex) mods not supported" in t for t in text)
        assert sum("Modified base found in BAM" in t for t in text) == 1  # (the ChEBI warning looks at the '+' entries, as before)
        if tag == "pct10":
            assert np.array_equal(got.hist, hist)
            for st in (2, 5):
                assert text.count(f"{statuses.count(st)} of {len(recs)} records skipped: {tp.SKIP_TEXT[st]} ({bam})") == 1, st
    # the same call without the flag is the parent's: '+' entries on the record's strand, the warning, three records of status 5
    want, k_t, hist, statuses = tp.restate(recs, ALPHABET, pct=10)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="Remora"):
        got = pileup_modbams(bam, ALPHABET, pct_filt=10, duplex=False)
    assert got.threshold_k == k_t and np.array_equal(got.hist, hist)
    tp.same_table(got, want, ALPHABET)
    assert tp.files_of(got, tmp_path, "plain") == (tp.bed_text(want, ALPHABET, REFS), tp.tsv_text(want, ALPHABET, REFS))
    text = [r.getMessage() for r in caplog.records]
    assert sum("Reverse strand (duplex) mods not supported" in t for t in text) == 1
    assert text.count(f"3 of {len(recs)} records skipped: {tp.SKIP_TEXT[5]} ({bam})") == 1 and statuses.count(5) == 3


# ---- 2. --duplex --ref -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["CG", "CHH_CHG", "CG_comb"])
def test_duplex_with_motifs_equals_the_restatement(torch_cuda, duplex_input, device_genome, tmp_path, tag):
    from remora_amd.pileup import pileup_modbams

    bam, _, recs, genome, _ = duplex_input
    motifs, combine = tgr.MOTIF_SETS[tag]
    for name, (kw, rkw) in THRESHOLDS.items():
        want, k_t, hist, _ = hd.restate(recs, ALPHABET, genome=genome, motifs=motifs, combine=combine, **rkw)
        assert len(want) > 50 and (combine or any(k[2] for k in want))
        got = pileup_modbams(bam, ALPHABET, ref=device_genome, motifs=motifs, combine_strands=combine, duplex=True, **kw)
        assert got.threshold_k == k_t and got.combined == combine and (name == "k307" or np.array_equal(got.hist, hist))
        tp.same_table(got, want, ALPHABET)
        assert tp.files_of(got, tmp_path, tag + name) == (tgr.bed_text(want, combine), tgr.tsv_text(want, combine))
    # placed on the record's own strand, the '-' entries would stand on other motif sites: the plain restatement differs
    assert tp.restate(recs, ALPHABET, pct=10)[0] != hd.restate(recs, ALPHABET, pct=10)[0]


# ---- 3. --hemi -------------------------------------------------------------------------------------------------------------------
def hemi_files(table, tmp_path, tag, min_coverage=1):
    return tp.files_of(table, tmp_path, tag, min_coverage)


@pytest.mark.parametrize("threshold", list(THRESHOLDS))
@pytest.mark.parametrize("case", list(HEMI_CASES))
def test_hemi_equals_the_restatement(torch_cuda, duplex_input, device_genome, tmp_path, case, threshold):
    from remora_amd.pileup import pileup_modbams

    bam, _, recs, genome, _ = duplex_input
    motif, alphabet = HEMI_CASES[case]
    kw, rkw = THRESHOLDS[threshold]
    want, k_t, hist, n_unpaired, _ = hd.restate_hemi(recs, alphabet, genome, motif, **rkw)
    assert len(want) >= 20 and n_unpaired > 0
    got = pileup_modbams(bam, alphabet, ref=device_genome, motifs=[motif], hemi=True, **kw)
    assert got.threshold_k == k_t and got.n_unpaired == n_unpaired
    hd.same_hemi_table(got, want, alphabet)
    if threshold == "pct10":  # the histogram of all kept single calls: that of the --duplex --ref --combine-strands run
        assert np.array_equal(got.hist, hist) and int(hist.sum()) == n_unpaired + 2 * got.n_calls
        single = pileup_modbams(bam, alphabet, ref=device_genome, motifs=[motif], combine_strands=True, duplex=True, **kw)
        assert np.array_equal(single.hist, hist) and single.threshold_k == k_t and single.n_calls == int(hist.sum())
    assert hemi_files(got, tmp_path, case) == (hd.hemi_bed_text(want, alphabet, REFS), hd.hemi_tsv_text(want, alphabet, REFS))
    assert hemi_files(got, tmp_path, case + "c3", 3)[0] == hd.hemi_bed_text(want, alphabet, REFS, 3)


def test_hemi_never_pairs_across_records_and_asks_the_region_of_the_c(torch_cuda, duplex_input, device_genome, tmp_path):
    from remora_amd.pileup import pileup_modbams

    bam, _, recs, genome, planted = duplex_input
    alphabet, m = ["C", "m"], planted["meet"]
    a, b = hd.by_name(recs, "ends_on_c"), hd.by_name(recs, "starts_on_g")
    two = str(tmp_path / "two.bam")
    third = next(r for r in recs[:40] if r["ref_id"] == 1)  # (a full duplex record on the other contig, so that the run keeps a pair at all)
    mr.write_bam(two, REFS, [a, b, third])
    want, _, _, n_unpaired, per_record = hd.restate_hemi([a, b, third], alphabet, genome, hd.CG, k_t=0)
    assert (0, m) not in want and any(c[1] == m for c in per_record[0][2]) and any(c[1] == m + 1 for c in per_record[1][2])
    for batch in (512, 2, 1):  # neighbours in one fill, and a batch each
        got = pileup_modbams(two, alphabet, ref=device_genome, motifs=[hd.CG], hemi=True, filter_threshold=0, pct_filt=None, batch=batch)
        hd.same_hemi_table(got, want, alphabet)
        assert got.n_unpaired == n_unpaired and not ((got.ref_id == 0) & (got.pos == m)).any()
    # a region whose edge falls between the C and the G of a CpG that full duplex records cover
    full, _, _, _, _ = hd.restate_hemi(recs, alphabet, genome, hd.CG, k_t=307)
    x = next(rp for rid, rp in sorted(full) if rid == 0 and rp > 500 and sum(full[(rid, rp)]) >= 3)
    for region, inside in (((0, 400, x + 1), True), ((0, x + 1, 1500), False)):
        want, k_t, _, n_unpaired, _ = hd.restate_hemi(recs, alphabet, genome, hd.CG, k_t=307, region=region)
        assert ((0, x) in want) == inside and len(want) > 5
        got = pileup_modbams(bam, alphabet, ref=device_genome, motifs=[hd.CG], hemi=True, filter_threshold=K307, pct_filt=None,
                             region=f"ctgA:{region[1]}-{region[2]}")
        hd.same_hemi_table(got, want, alphabet)
        assert got.n_unpaired == n_unpaired and (want.get((0, x)) == full[(0, x)] if inside else True)


def test_hemi_does_not_depend_on_batch_buffer_or_file_order(torch_cuda, duplex_input, tmp_path):
    from remora_amd.pileup import pileup_modbams

    bam, fa, recs, genome, _ = duplex_input
    run = lambda paths=bam, **kw: pileup_modbams(paths, ALPHABET, ref=fa, motifs=[hd.CG], hemi=True, **kw)  # noqa: E731
    whole = run(filter_threshold=K307, pct_filt=None)
    ref_files, by_pct = hemi_files(whole, tmp_path, "whole"), hemi_files(run(pct_filt=10), tmp_path, "pct")
    assert whole.n_flushes == 1
    for batch in (1, 7, 512):
        for cap in (64, None):
            got = run(filter_threshold=K307, pct_filt=None, batch=batch, buffer_calls=cap)
            assert hemi_files(got, tmp_path, f"b{batch}c{cap}") == ref_files and got.n_unpaired == whole.n_unpaired
            assert got.n_flushes == (-(-got.n_calls // 64) if cap else 1)
    p1, p2 = str(tmp_path / "half1.bam"), str(tmp_path / "half2.bam")
    mr.write_bam(p1, REFS, recs[:23])
    mr.write_bam(p2, REFS, recs[23:])
    for tag, order in (("ab", [p1, p2]), ("ba", [p2, p1])):
        assert hemi_files(run(order, filter_threshold=K307, pct_filt=None), tmp_path, tag) == ref_files
        assert hemi_files(run(order, pct_filt=10), tmp_path, tag + "pct") == by_pct


# ---- 4. the pair kernels through the C ABI ------------------------------------------------------------------------------------
word = tp.word


def pair_in_python(words, off, n_codes):
    """The pairs per record and the pair words: the first word with the '+' word's site and strand 1 among the 15 before and
    the 15 behind it, inside the record's slice."""
    counts, out = [], []
    for lo, hi in zip(off[:-1], off[1:]):
        k = 0
        for i in range(lo, hi):
            w = words[i]
            if (w >> 4) & 1:
                continue
            for j in range(max(lo, i - 15), min(hi, i + 16)):
                x = words[j]
                if x >> 5 == w >> 5 and (x >> 4) & 1:
                    out.append((w & ~31) | (min(w & 15, n_codes - 1) * n_codes + min(x & 15, n_codes - 1)))
                    k += 1
                    break
        counts.append(k)
    return counts, out


def run_pairs(words, off, n_codes, n_records=None, n_words=None):
    """rmr_pileup_pair_counts, the prefix sum, rmr_pileup_pair_fill -> (pairs per record, pair words); the fill's output has a
    guard word behind it that must stay."""
    import torch

    from remora_amd import _lib as L
    from remora_amd.engine import get_engine

    eng, lib = get_engine(None), L.lib()
    dev = eng.torch_device
    n = len(off) - 1 if n_records is None else n_records
    nw = len(words) if n_words is None else n_words
    d_words = torch.from_numpy(np.asarray(list(words) + [0], np.uint64).view(np.int64)).to(dev)
    d_off = torch.from_numpy(np.asarray(off, np.int64)).to(dev)
    d_pairs = torch.full((max(n, 1),), -7, dtype=torch.int64, device=dev)
    L.check(lib.rmr_pileup_pair_counts(eng.handle, n, d_off.data_ptr(), d_words.data_ptr(), nw, d_pairs.data_ptr()))
    eng.synchronize()
    pairs = d_pairs[:n].cpu().numpy()
    pair_off = np.zeros(n + 1, np.int64)
    np.cumsum(pairs, out=pair_off[1:])
    guard = 0x7EAD_BEEF_0BAD_F00D
    d_out = torch.full((int(pair_off[-1]) + 1,), guard, dtype=torch.int64, device=dev)
    L.check(lib.rmr_pileup_pair_fill(eng.handle, n, d_off.data_ptr(), d_words.data_ptr(), nw, n_codes, torch.from_numpy(pair_off).to(dev).data_ptr(),
                                     d_out.data_ptr()))
    eng.synchronize()
    out = d_out.cpu().numpy()
    assert int(out[-1]) == guard
    return pairs.tolist(), out[:-1].view(np.uint64).tolist()


def slice_words(n, rng, n_codes, ref_id, start):
    """n words of one record in walk order: single '+' and '-' words, pairs with the partner behind and before the '+' word, at
    distance 1, 15 and 16 (other sites between them)."""
    out, pos = [], start
    code = lambda: int(rng.integers(0, n_codes))  # noqa: E731
    while len(out) < n:
        kind, pos = int(rng.integers(0, 7)), pos + int(rng.integers(2, 40))
        first, second = (0, 1) if rng.integers(0, 2) else (1, 0)
        if kind == 0:
            out.append(word(ref_id, pos, 0, code()))
        elif kind == 1:
            out.append(word(ref_id, pos, 1, code()))
        else:
            gap = {2: 0, 3: 0, 4: 14, 5: 15, 6: int(rng.integers(1, 14))}[kind]  # words between the two: distance gap + 1
            out.append(word(ref_id, pos, first, code()))
            out += [word(ref_id, pos + 1 + g, int(rng.integers(0, 2)), code()) for g in range(gap)]
            out.append(word(ref_id, pos, second, code()))
            pos += gap + 1
    return out[:n]


@pytest.mark.parametrize("n_codes", [3, 4])
def test_pair_kernels_on_hand_made_words(torch_cuda, n_codes):
    rng = np.random.default_rng(31 + n_codes)
    words, off = [], [0]
    for r, n in enumerate((0, 1, 2, 63, 64, 65, 300, 0, 300, 7)):
        words += slice_words(n, rng, n_codes, r % 3, 100)
        off.append(len(words))
    # equal sites in neighbouring slices: a '+' word ends one, its '-' word begins the next - and the other way round
    for first in (0, 1):
        words += [word(1, 5000, 0, 1), word(1, 5001, first, 2)]
        off.append(len(words))
        words += [word(1, 5001, 1 - first, 0), word(1, 5002, 1, 1)]
        off.append(len(words))
    # a slice of 300 whose pairs straddle the waves of the block and its rounds: (1, 2), (3, 4), .. (63, 64) .. (255, 256) ..
    words += [word(2, 9, 0, 0)] + [word(2, 10 + i // 2, i % 2, (i * 7) % n_codes) for i in range(298)] + [word(2, 400, 1, 0)]
    off.append(len(words))
    # distance 15 pairs, distance 16 does not (the emit never produces it); two '-' words of one site: the first in index order
    far = lambda dist: [word(0, 70, 0, 1)] + [word(0, 71 + g, 0, 0) for g in range(dist - 1)] + [word(0, 70, 1, 2)]  # noqa: E731
    for ws in (far(15), far(16), far(15)[::-1], far(16)[::-1], [word(0, 8, 1, 1), word(0, 8, 0, 2), word(0, 8, 1, 0)]):
        words += ws
        off.append(len(words))
    want_counts, want_words = pair_in_python(words, off, n_codes)
    k = len(off) - 1
    assert want_counts[k - 5 : k] == [1, 0, 1, 0, 1] and want_counts[k - 6] == 149 and want_counts[k - 10 : k - 6] == [0, 0, 0, 0]
    assert want_words[-1] == word(0, 8, 0, 2 * n_codes + 1)
    got_counts, got_words = run_pairs(words, off, n_codes)
    assert got_counts == want_counts and got_words == want_words and sum(want_counts) > 200
    # n_words bounds the loads: cut behind the first 70 words, the later records pair nothing
    cut_off = [min(o, 70) for o in off]
    assert run_pairs(words, off, n_codes, n_words=70) == pair_in_python(words[:70], cut_off, n_codes)


def test_pair_refusals_launch_nothing(torch_cuda):
    import torch

    from remora_amd import _lib as L
    from remora_amd.engine import get_engine

    eng, lib = get_engine(None), L.lib()
    t = torch.zeros(8, dtype=torch.int64, device=eng.torch_device)
    p = t.data_ptr()
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        assert lib.rmr_pileup_pair_counts(eng.handle, 0, p, p, 0, p) == 0 and lib.rmr_pileup_pair_fill(eng.handle, 0, p, p, 0, 3, p, p) == 0
        for n_codes in (2, 5, 0, -1):
            assert lib.rmr_pileup_pair_fill(eng.handle, 1, p, p, 2, n_codes, p, p) != 0 and b"3 or 4" in lib.rmr_last_error()
        for n_records, n_words in ((-1, 2), (1, -1)):
            assert lib.rmr_pileup_pair_counts(eng.handle, n_records, p, p, n_words, p) != 0
            assert lib.rmr_pileup_pair_fill(eng.handle, n_records, p, p, n_words, 3, p, p) != 0
        for k in range(4):
            a = [eng.handle, p, p, p]
            a[k] = None
            assert lib.rmr_pileup_pair_counts(a[0], 1, a[1], a[2], 2, a[3]) != 0 and b"NULL" in lib.rmr_last_error()
        for k in range(5):
            a = [eng.handle, p, p, p, p]
            a[k] = None
            assert lib.rmr_pileup_pair_fill(a[0], 1, a[1], a[2], 2, 3, a[3], a[4]) != 0 and b"NULL" in lib.rmr_last_error()
        assert "pileup_pair" not in eng.profile(), eng.profile()
        assert lib.rmr_pileup_pair_counts(eng.handle, 1, p, p, 0, p) == 0  # (one record without words: launched, pairs nothing)
        eng.synchronize()
        assert eng.profile()["pileup_pair"][1] == 1 and int(t[0]) == 0
    finally:
        eng.profile_enable(False)


def test_hemi_emit_refusals_launch_nothing(torch_cuda, duplex_input, device_genome):
    """The C entries: hemi without a reference, without the fold, with two motifs, without duplex."""
    import torch

    from remora_amd import _lib as L
    from remora_amd.engine import get_engine
    from remora_amd.pileup import _pileup_ref_struct, check_pileup_motifs

    eng, lib = get_engine(None), L.lib()
    b = L.ModbamBatch()
    b.n_records, b.n_mods, b.n_refs = 0, 1, 2
    b.mod_codes = b"m"
    t = torch.zeros(8, dtype=torch.int64, device=eng.torch_device)
    p = t.data_ptr()
    one, two = check_pileup_motifs([hd.CG], "C", True), check_pileup_motifs([hd.CG, hd.GC], "C", True)
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    def opts(pref, duplex, hemi):
        return ctypes.byref(L.PileupEmitOpts(region_ref=-1, ref=None if pref is None else ctypes.pointer(pref), duplex=duplex, hemi=hemi))

    ok = _pileup_ref_struct(device_genome, one, True)
    try:
        for pref, duplex, message in ((None, 1, b"needs a reference"), (_pileup_ref_struct(device_genome, one, False), 1, b"combine must be set"),
                                      (_pileup_ref_struct(device_genome, two, True), 1, b"exactly one motif"), (ok, 0, b"duplex must be set")):
            assert lib.rmr_pileup_emit_counts(eng.handle, ctypes.byref(b), opts(pref, duplex, 1), p, p, p, p, p, None) != 0
            assert message in lib.rmr_last_error()
            assert lib.rmr_pileup_emit_fill(eng.handle, ctypes.byref(b), opts(pref, duplex, 1), 0, p, p, p, p, p, p) != 0
            assert message in lib.rmr_last_error()
        assert lib.rmr_pileup_emit_counts(eng.handle, ctypes.byref(b), opts(ok, 1, 1), p, p, p, p, p, None) == 0
        assert lib.rmr_pileup_emit_counts(eng.handle, ctypes.byref(b), opts(None, 1, 0), p, p, p, p, p, None) == 0
        assert not any(k.startswith("pileup_") for k in eng.profile()), eng.profile()
    finally:
        eng.profile_enable(False)


# ---- 5. rows of up to 16 columns -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", [9, 16])
def test_table_of_up_to_16_columns(torch_cuda, ncol):
    from remora_amd import _lib as L
    from remora_amd.engine import get_engine
    from remora_amd.pileup import DevicePileup

    eng = get_engine(None)
    rng = np.random.default_rng(ncol)
    n = 5000
    site = rng.integers(0, 600, n)
    words = [word(s % 3, s // 3, 0, c) for s, c in zip(site, rng.integers(0, ncol, n))] + [word(2, 999, 0, ncol - 1)] * 3
    wk, wc = tp.want_table(words, ncol)
    assert wc.shape[1] == ncol and (wc.sum(axis=0) > 0).all() and wc[-1, ncol - 1] == 3  # every code, the last one included, is counted
    for cap in (len(words), 257):  # one flush; many, merged into the resident table
        pile = tp.Pile.__new__(tp.Pile)
        pile.eng, pile.p = eng, DevicePileup(eng, 3, 1 << 31, None, cap, ncol=ncol)
        try:
            pile.add(words)
            keys, counts, n_calls, n_flushes = pile.table()
        finally:
            pile.p.close()
        assert n_calls == len(words) and n_flushes == -(-len(words) // cap)
        assert counts.shape == wc.shape and np.array_equal(keys, wk) and np.array_equal(counts, wc)
    h, lib = ctypes.c_void_p(), L.lib()
    for bad in (2, 17, 0, -1):
        assert lib.rmr_pileup_create_cols(eng.handle, 3, 1000, bad, 64, ctypes.byref(h)) != 0 and not h and b"3 to 16 columns" in lib.rmr_last_error()
    assert lib.rmr_pileup_create(eng.handle, 3, 1000, 9, 64, ctypes.byref(h)) != 0 and not h and b"1 to 7 modified bases" in lib.rmr_last_error()


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_api_bytes(torch_cuda, duplex_input, tmp_path):
    from remora_amd.pileup import pileup_modbams

    bam, fa, recs, genome, _ = duplex_input
    base = [sys.executable, "-m", "remora_amd", "analyze", "pileup_modbams", "--bam", bam, "--canonical-base", "C"]
    runs = {"duplex": ["--mod-bases", "h", "m", "--duplex"],
            "hemi": ["--mod-bases", "m", "--ref", fa, "--cpg", "--hemi", "--min-coverage", "2", "--reads-per-batch", "7"]}
    procs = {t: subprocess.Popen(base + ["--out-bed", str(tmp_path / f"{t}.bed"), "--counts-filename", str(tmp_path / f"{t}.tsv")] + extra,
                                 cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for t, extra in runs.items()}
    for t, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err
    read = lambda t: ((tmp_path / f"{t}.bed").read_text(), (tmp_path / f"{t}.tsv").read_text())  # noqa: E731
    assert read("duplex") == tp.files_of(pileup_modbams(bam, ALPHABET, duplex=True), tmp_path, "api_duplex")  # the default: --pct-filt 10
    want, _, _, _ = hd.restate(recs, ALPHABET, pct=10)
    assert read("duplex") == (tp.bed_text(want, ALPHABET, REFS), tp.tsv_text(want, ALPHABET, REFS))
    api = pileup_modbams(bam, ["C", "m"], ref=fa, motifs=[("CG", 0)], hemi=True)
    assert read("hemi") == hemi_files(api, tmp_path, "api_hemi", 2)
    want, _, _, _, _ = hd.restate_hemi(recs, ["C", "m"], genome, hd.CG, pct=10)
    assert read("hemi") == (hd.hemi_bed_text(want, ["C", "m"], REFS, 2), hd.hemi_tsv_text(want, ["C", "m"], REFS)) and len(read("hemi")[0]) > 0
