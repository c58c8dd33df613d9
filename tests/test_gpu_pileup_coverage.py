"""`analyze pileup_modbams --coverage-columns` on the GPU against the plain-Python restatement of pileup_coverage_restate.py:
per record aligned_pairs and the four rules.  Every comparison is exact - equal integers, equal file bytes.  The coverage
kernel is also driven through the C ABI against a site table made by hand."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

import modbam_restate as mr
import pileup_coverage_restate as pc
import test_gpu_pileup as tp
import test_gpu_pileup_partition as tpp
import test_gpu_pileup_ref as tr
import test_host_pileup_duplex as hpd
from conftest import ROOT

pytestmark = pytest.mark.gpu

ALPHABET = pc.ALPHABET
REFS = pc.REFS
K_08 = 410  # ceil(512 x 0.8)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def run(bams, alphabet=ALPHABET, coverage=True, **kw):
    from remora_amd.pileup import pileup_modbams

    if "pct_filt" not in kw and "filter_threshold" not in kw:
        kw.update(filter_threshold=0.8, pct_filt=None)
    return pileup_modbams(bams, alphabet, coverage=coverage, **kw)


def cover_of(table):
    return {k: row for k, row in zip(zip(table.ref_id.tolist(), table.pos.tolist(), table.strand.tolist()), table.coverage.tolist())}


def same_cover(got, want):
    assert got.coverage is not None and got.coverage.dtype == np.int64 and got.coverage.shape == (got.pos.size, 3)
    have = cover_of(got)
    assert sorted(have) == sorted(want)
    bad = [(k, have[k], want[k]) for k in sorted(want) if have[k] != want[k]]
    assert not bad, (len(bad), bad[:10])


@pytest.fixture(scope="module")
def cov(tmp_path_factory, torch_cuda):
    """The input (test_gpu_pileup._synthetic() and one record per edge case), its BAM, and the run at 0.8 the tests share."""
    recs, genome, expect = pc.coverage_input()
    d = tmp_path_factory.mktemp("pileup_coverage")
    path = str(d / "cov.bam")
    mr.write_bam(path, REFS, recs)
    return dict(recs=recs, genome=genome, expect=expect, dir=d, path=path, table=run(path))


# ---- 1. the table against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["thr08", "pct10"])
def test_table_equals_the_restatement(cov, tmp_path, mode):
    from remora_amd.pileup import write_bedmethyl, write_counts

    kw, rk = (dict(filter_threshold=0.8, pct_filt=None), dict(k_t=K_08)) if mode == "thr08" else (dict(pct_filt=10), dict(pct=10))
    want, k_t, hist, _ = tp.restate(cov["recs"], ALPHABET, **rk)
    want_cover = pc.cover_restate(cov["recs"], ALPHABET, list(want))
    got = cov["table"] if mode == "thr08" else run(cov["path"], **kw)
    plain = run(cov["path"], coverage=False, **kw)
    assert got.threshold_k == k_t == plain.threshold_k and plain.coverage is None
    tp.same_table(got, want, ALPHABET)
    for f in ("ref_id", "pos", "strand", "counts"):  # the table is that of the run without the flag
        assert getattr(got, f).tobytes() == getattr(plain, f).tobytes(), f
    assert got.n_calls == plain.n_calls and (got.hist is None) == (plain.hist is None) and (got.hist is None or np.array_equal(got.hist, plain.hist))
    assert got.peak_device_bytes >= plain.peak_device_bytes
    same_cover(got, want_cover)
    bed, tsv = tmp_path / "t.bed", tmp_path / "t.tsv"
    write_bedmethyl(got, bed, min_coverage=2), write_counts(got, tsv)
    assert bed.read_text() == pc.bed18_text(want, want_cover, ALPHABET, REFS, min_coverage=2)
    assert tsv.read_text() == pc.tsv_text(want, want_cover, ALPHABET, REFS)
    assert tp.files_of(plain, tmp_path, "plain") == (tp.bed_text(want, ALPHABET, REFS), tp.tsv_text(want, ALPHABET, REFS))


def test_every_edge_case_by_name(cov):
    """Case by case: at the site of each named record the device's counts are the restatement's, the record alone adds there
    what its case says (a column, or nothing), and that column is not empty on the device."""
    got = cover_of(cov["table"])
    recs, expect = cov["recs"], cov["expect"]
    want = pc.cover_restate(recs, ALPHABET, list(got))
    for case, (site, col) in expect.items():
        assert got[site] == want[site], (case, site)
        rec = next(r for r in recs if r.get("case") == case)
        alone = pc.record_cover(rec, ALPHABET, [s for s in got if s[0] == site[0]])
        assert alone.get(site) == col, case
        if col is not None:
            assert got[site][col] >= 1, case


# ---- 2. conservation ------------------------------------------------------------------------------------------------------------
def test_conservation(cov):
    got = cov["table"]
    reach = {}
    for rec in cov["recs"]:
        if tp.record_calls(rec, ALPHABET)[0] == 0:
            for _, r, marker in mr.aligned_pairs(rec["cigar"], rec["pos"]):
                if r is not None and marker is not None:  # (an N skip has no marker)
                    key = (rec["ref_id"], r, (rec["flag"] >> 4) & 1)
                    reach[key] = reach.get(key, 0) + 1
    total = got.counts.sum(axis=1) + got.coverage.sum(axis=1)
    keys = list(zip(got.ref_id.tolist(), got.pos.tolist(), got.strand.tolist()))
    assert total.tolist() == [reach[k] for k in keys] and len(keys) > 1000


# ---- 3. independence ------------------------------------------------------------------------------------------------------------
def test_batch_buffer_and_file_order_do_not_matter(cov, tmp_path):
    whole, recs = cov["table"], cov["recs"]
    for batch in (1, 7, 512):
        got = run(cov["path"], batch=batch)
        assert np.array_equal(got.coverage, whole.coverage) and np.array_equal(got.counts, whole.counts), batch
    got = run(cov["path"], buffer_calls=64)
    assert got.n_flushes > 1 and np.array_equal(got.coverage, whole.coverage) and np.array_equal(got.counts, whole.counts)
    p1, p2 = str(tmp_path / "half1.bam"), str(tmp_path / "half2.bam")
    mr.write_bam(p1, REFS, recs[:40])
    mr.write_bam(p2, REFS, recs[40:])
    for order in ([p1, p2], [p2, p1]):
        got = run(order)
        assert np.array_equal(got.pos, whole.pos) and np.array_equal(got.coverage, whole.coverage)


# ---- 4. --region ----------------------------------------------------------------------------------------------------------------
def test_region_is_the_rows_of_the_whole_table_inside_it(cov):
    whole = cov["table"]
    got = run(cov["path"], region="ctgA:1100-1650")
    rows = np.nonzero((whole.ref_id == 0) & (whole.pos >= 1100) & (whole.pos < 1650))[0]
    assert rows.size > 100 and np.array_equal(got.pos, whole.pos[rows]) and np.array_equal(got.strand, whole.strand[rows])
    assert np.array_equal(got.counts, whole.counts[rows]) and np.array_equal(got.coverage, whole.coverage[rows])
    assert got.coverage.sum(axis=0).min() > 0
    want, _, _, _ = tp.restate(cov["recs"], ALPHABET, k_t=K_08, region=(0, 1100, 1650))
    same_cover(got, pc.cover_restate(cov["recs"], ALPHABET, list(want), region=(0, 1100, 1650)))


# ---- 5. with a reference ------------------------------------------------------------------------------------------------------
def restate_ref(recs, alphabet, genome, motifs, combine, k_t):
    calls = [c for c in (tr.place(c, genome, motifs, combine) for rec in recs for c in tp.record_calls(rec, alphabet)[1]) if c is not None]
    ncol = len(alphabet) + 1
    table = {}
    for rid, pos, strand, cls, kmax in calls:
        table.setdefault((rid, pos, strand), [0] * ncol)[cls if kmax >= k_t else ncol - 1] += 1
    return table


def write_fasta(path, genome):
    with open(path, "w") as fh:
        fh.write(tr.fasta_text(list(zip([r[0] for r in REFS], genome)), 60))


@pytest.mark.parametrize("combine", [False, True])
def test_cpg_sites_plain_and_combined(torch_cuda, tmp_path, combine):
    genome, recs = tr._genome_and_records()
    g = genome[0].upper()
    motifs = [("CG", 0)]
    folded, apart = (restate_ref(recs, ALPHABET, genome, motifs, c, K_08) for c in (True, False))
    s = next(p for p in range(1150, 1250) if g[p : p + 2] == "CG" and (0, p, 0) in folded and (0, p, 0) in apart and (0, p + 1, 1) in apart)
    # a '-' record that starts on the G of the CpG at s (it is asked at s + 1: it counts at s), one that ends on its C (its
    # span ends before s + 1: it does not), and a '+' record over both
    recs = recs + [dict(pc.over(s + 1, g[s + 1 : s + 51], [("M", 50)], s + 1, flag=16), case="minus_starts_on_the_g"),
                   dict(pc.over(s - 49, g[s - 49 : s + 1], [("M", 50)], s, flag=16), case="minus_ends_on_the_c"),
                   dict(pc.over(s - 25, g[s - 25 : s + 25], [("M", 50)], s), case="plus_over_the_site")]
    bam, fa = str(tmp_path / "r.bam"), str(tmp_path / "g.fa")
    mr.write_bam(bam, REFS, recs)
    write_fasta(fa, genome)
    want = restate_ref(recs, ALPHABET, genome, motifs, combine, K_08)
    want_cover = pc.cover_restate(recs, ALPHABET, list(want), genome=genome, motifs=motifs, combine=combine)
    named = {r["case"]: r for r in recs if r.get("case")}
    sites = [k for k in want if k[0] == 0]
    kw = dict(genome=genome, motifs=motifs, combine=combine)
    if combine:
        assert pc.record_cover(named["minus_starts_on_the_g"], ALPHABET, sites, **kw).get((0, s, 0)) == 2
        assert (0, s, 0) not in pc.record_cover(named["minus_ends_on_the_c"], ALPHABET, sites, **kw)
        assert pc.record_cover(named["plus_over_the_site"], ALPHABET, sites, **kw).get((0, s, 0)) == 2
    else:
        assert pc.record_cover(named["minus_starts_on_the_g"], ALPHABET, sites, **kw).get((0, s + 1, 1)) == 2
        assert not any(k[1] in (s, s + 1) for k in pc.record_cover(named["minus_ends_on_the_c"], ALPHABET, sites, **kw))
    got = run(bam, ref=fa, motifs=motifs, combine_strands=combine)
    plain = run(bam, coverage=False, ref=fa, motifs=motifs, combine_strands=combine)
    tp.same_table(got, want, ALPHABET)
    assert got.combined == combine and np.array_equal(got.counts, plain.counts) and np.array_equal(got.pos, plain.pos)
    same_cover(got, want_cover)
    assert all(sum(v[c] for v in want_cover.values()) > 0 for c in (1, 2))
    bed, tsv = tmp_path / "t.bed", tmp_path / "t.tsv"
    from remora_amd.pileup import write_bedmethyl, write_counts

    write_bedmethyl(got, bed), write_counts(got, tsv)
    assert bed.read_text() == pc.bed18_text(want, want_cover, ALPHABET, REFS, combine=combine)
    assert tsv.read_text() == pc.tsv_text(want, want_cover, ALPHABET, REFS, combine=combine)


@pytest.mark.parametrize("motif,alphabet,shift", [(("GATC", 1), ["A", "a"], 1), (("GC", 1), ["C", "h", "m"], -1)])
def test_combined_motifs_with_either_shift(torch_cuda, tmp_path, motif, alphabet, shift):
    recs, genome, _ = hpd.synth()
    assert len(motif[0]) - 1 - 2 * motif[1] == shift
    # one site of the motif, and records of both strands beside, on and over the position they are asked at
    g, base, code = genome[0], alphabet[0], alphabet[-1]
    site = next(k[1] for k in sorted(restate_ref(recs, alphabet, genome, [motif], True, K_08)) if k[0] == 0 and k[1] > 600)
    a = site + shift  # where a '-' record is asked
    other = "T" if g[a] != "T" else "A"
    ov = lambda *args, **kw: pc.over(*args, base=base, code=code, **kw)  # noqa: E731
    edges = {"plus_over": (ov(site - 25, g[site - 25 : site + 25], [("M", 50)], site), 2),
             "minus_over": (ov(a - 25, g[a - 25 : a + 25], [("M", 50)], a, flag=16), 2),
             "minus_starts_where_it_is_asked": (ov(a, g[a : a + 50], [("M", 50)], a, flag=16), 2),
             "minus_ends_one_before": (ov(a - 50, g[a - 50 : a], [("M", 50)], a, flag=16), None),
             "minus_starts_one_behind": (ov(a + 1, g[a + 1 : a + 51], [("M", 50)], a, flag=16), None),
             "plus_deleted": (ov(site - 30, g[site - 30 : site - 1] + g[site + 2 : site + 32], [("M", 29), ("D", 3), ("M", 30)], site), 0),
             "minus_substituted": (ov(a - 25, g[a - 25 : a] + other + g[a + 1 : a + 25], [("M", 50)], a, flag=16), 1)}
    for case, (rec, col) in edges.items():
        got = pc.record_cover(rec, alphabet, [(0, site, 0)], genome=genome, motifs=[motif], combine=True)
        assert got.get((0, site, 0)) == col, (case, got)
    recs = recs + [dict(rec, name=case) for case, (rec, _) in edges.items()]
    bam, fa = str(tmp_path / "r.bam"), str(tmp_path / "g.fa")
    mr.write_bam(bam, REFS, recs)
    write_fasta(fa, genome)
    want = restate_ref(recs, alphabet, genome, [motif], True, K_08)
    want_cover = pc.cover_restate(recs, alphabet, list(want), genome=genome, motifs=[motif], combine=True)
    assert len(want) > 20 and sum(v[2] for v in want_cover.values()) > 0 and sum(v[0] + v[1] for v in want_cover.values()) > 0
    got = run(bam, alphabet, ref=fa, motifs=[motif], combine_strands=True)
    tp.same_table(got, want, alphabet)
    same_cover(got, want_cover)
    # several motifs with different shifts in one run: the folded words of a '-' record are no longer strictly monotone
    motifs = [("GATC", 1), ("AT", 0), ("TA", 1)] if alphabet[0] == "A" else [("GC", 1), ("CG", 0), ("CCGG", 1)]
    want = restate_ref(recs, alphabet, genome, motifs, True, K_08)
    got = run(bam, alphabet, ref=fa, motifs=motifs, combine_strands=True)
    tp.same_table(got, want, alphabet)
    same_cover(got, pc.cover_restate(recs, alphabet, list(want), genome=genome, motifs=motifs, combine=True))


# ---- 6. --partition-tag ---------------------------------------------------------------------------------------------------------
def test_each_partition_equals_the_run_on_its_records(torch_cuda, tmp_path):
    from remora_amd.pileup import partition_tables, write_partitioned

    recs, _ = tpp.tagged_records()
    path = str(tmp_path / "tagged.bam")
    tpp.write_bam(path, REFS, recs)
    table = run(path, partition_tag="HP")
    plain = run(path, coverage=False, partition_tag="HP")
    assert table.partition_labels == ["1", "2", "ungrouped"] and np.array_equal(table.counts, plain.counts)
    assert table.coverage.shape == (table.pos.size, 3) and plain.coverage is None
    subs = partition_tables(table)
    write_partitioned(table, tmp_path / "p.bed", tmp_path / "p.tsv")
    whole = tp.restate(recs, ALPHABET, k_t=K_08)[0]
    for label, name in (("1", "HP_1"), ("2", "HP_2"), ("ungrouped", "ungrouped")):
        own = [r for r in recs if r["label"] == label]
        only = str(tmp_path / f"only_{name}.bam")
        tpp.write_bam(only, REFS, own)
        alone = run(only)
        sub = subs[label]
        assert np.array_equal(sub.pos, alone.pos) and np.array_equal(sub.counts, alone.counts) and np.array_equal(sub.coverage, alone.coverage), label
        want = tp.restate(own, ALPHABET, k_t=K_08)[0]
        want_cover = pc.cover_restate(own, ALPHABET, list(want))
        same_cover(sub, want_cover)
        assert sum(map(sum, want_cover.values())) > 0 and len(want) < len(whole)
        assert (tmp_path / f"p.{name}.bed").read_text() == pc.bed18_text(want, want_cover, ALPHABET, REFS)
        assert (tmp_path / f"p.{name}.tsv").read_text() == pc.tsv_text(want, want_cover, ALPHABET, REFS)


# ---- 7. the kernel through the C ABI, on a site table made by hand --------------------------------------------------------------
BIG_REFS = [("ctgA", 10000), ("ctgB", 10000)]


def hand_records():
    """No record calls a site: the only call of each lies under its soft clip."""
    rng = np.random.default_rng(5)
    rand = lambda n: "".join(rng.choice(list("ACGTN"), n, p=[0.22, 0.3, 0.22, 0.22, 0.04]))  # noqa: E731
    rec = lambda seq, cigar, pos, flag=0, ref=0: tp._rec("C" + seq, [("S", 1)] + cigar, "C+m?,0;", [250], flag=flag, ref=ref, pos=pos)  # noqa: E731
    recs = [rec(rand(3000), [("M", 3000)], 100),                                        # more sites than a workgroup has lanes
            rec(rand(750), [("M", 2), ("D", 1), ("M", 2), ("I", 1)] * 150, 500),         # more operations than lanes
            rec(rand(50), [("M", 50)], 4000),                                             # overlaps no site
            rec(rand(50), [("M", 50)], 700, ref=1)]                                       # another contig
    rev = tp._rec(rand(2999) + "G", [("M", 2999), ("S", 1)], "C+m?,0;", [250], flag=16, pos=100)  # the other strand: nothing
    return recs + [rev]


def device_batches(eng, path, mods, n_refs):
    from remora_amd.io import iter_bam_raw_batches
    from remora_amd.validate import modbam_device_batch, tokenise_mod_tags

    for rb, _ in iter_bam_raw_batches(path, want_ref=False, batch=512):
        tok = tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off)
        buf, b = modbam_device_batch(eng.torch_device, mods, rb.seq, rb.seq_off, rb.cigar, rb.cigar_off, rb.flag, rb.ref_id, rb.pos, rb.has, tok)
        b.n_refs = n_refs
        yield buf, b, int(np.asarray(rb.cigar).size), int(tok[5].size)


def test_cover_kernel_on_a_hand_made_site_table(torch_cuda, tmp_path):
    from remora_amd import _lib as L
    from remora_amd.engine import get_engine
    from remora_amd.pileup import DevicePileup, _emit_batch

    torch = torch_cuda
    recs = hand_records()
    assert [tp.record_calls(r, ["C", "m"]) for r in recs] == [(0, [])] * len(recs) and len(recs[1]["cigar"]) == 601
    path = str(tmp_path / "hand.bam")
    mr.write_bam(path, BIG_REFS, recs)
    eng, lib = get_engine(None), L.lib()
    tables = {"3000 sites": [(0, p, 0) for p in range(100, 3100)], "one site": [(0, 700, 0)]}
    eng.synchronize()
    eng.profile_enable(True)
    try:
        for name, sites in tables.items():
            want = pc.cover_restate(recs, ["C", "m"], sites)
            assert sum(v[0] for v in want.values()) > 0 or name == "one site"
            words = torch.from_numpy(np.array([tp.word(*s, 0) for s in sites], np.uint64).view(np.int64)).to(eng.torch_device)
            with DevicePileup(eng, 2, 10000, 2, 4096) as pile:
                pile.add(words, words.numel())
                eng.synchronize()
                batches = list(device_batches(eng, path, ["m"], 2))
                assert len(batches) == 1
                buf, b, n_cig, n_deltas = batches[0]
                pile.set_canonical("C")
                eng.profile_reset()
                # before rmr_pileup_finish: refused, nothing launched
                dummy = torch.zeros(8, dtype=torch.int64, device=eng.torch_device)
                rc = lib.rmr_pileup_cover(pile.h, ctypes.byref(b), None, dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), None, 0,
                                          None, 0)
                assert rc != 0 and b"rmr_pileup_finish" in lib.rmr_last_error() and "pileup_cover" not in eng.profile()
                n_sites = pile.finish()[0]
                assert n_sites == len(sites)
                # no record: nothing launched, nothing stored
                n_records, b.n_records = b.n_records, 0
                rc = lib.rmr_pileup_cover(pile.h, ctypes.byref(b), None, dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), None, 0,
                                          None, 0)
                b.n_records = n_records
                assert rc == 0 and "pileup_cover" not in eng.profile() and not pile.read_cover(n_sites).any()
                peak = pile.finish()[3]
                _emit_batch(eng, b, L.PileupEmitOpts(region_ref=-1), K_08, None, n_cig, n_deltas, cover=pile)
                eng.synchronize()
                assert eng.profile()["pileup_cover"][1] == 1  # one launch, under its own name
                keys, counts = pile.read(n_sites)
                got = pile.read_cover(n_sites)
                assert pile.finish()[3] >= peak and pile.finish()[3] >= 12 * n_sites
                assert got.dtype == np.uint32 and got.shape == (n_sites, 3) and counts.sum() == n_sites
                have = {(int(k >> 32), int((k >> 1) & 0x7FFFFFFF), int(k & 1)): row for k, row in zip(keys.tolist(), got.tolist())}
                bad = [(k, have[k], want[k]) for k in sites if have[k] != want[k]]
                assert not bad, (name, len(bad), bad[:10])
                # words added afterwards drop the counts: the next join starts from zero
                pile.add(words[:1], 1)
                eng.synchronize()
                assert pile.finish()[0] == n_sites and not pile.read_cover(n_sites).any()
                del buf
        # without a canonical base the join is refused
        with DevicePileup(eng, 2, 10000, 2, 64) as pile:
            pile.finish()
            rc = lib.rmr_pileup_cover(pile.h, ctypes.byref(b), None, dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), None, 0, None, 0)
            assert rc != 0 and b"canonical" in lib.rmr_last_error()
            assert lib.rmr_pileup_set_canonical(pile.h, ord("N")) != 0
    finally:
        eng.profile_enable(False)


# ---- 8. the command line --------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_restatement_bytes(cov, tmp_path):
    base = [sys.executable, "-m", "remora_amd", "analyze", "pileup_modbams", "--bam", cov["path"], "--canonical-base", "C", "--mod-bases", "h", "m",
            "--filter-threshold", "0.8"]
    runs = {"cov": ["--coverage-columns"], "plain": []}
    procs = {t: subprocess.Popen(base + ["--out-bed", str(tmp_path / f"{t}.bed"), "--counts-filename", str(tmp_path / f"{t}.tsv")] + extra, cwd=ROOT,
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for t, extra in runs.items()}
    errs = {}
    for t, p in procs.items():
        _, errs[t] = p.communicate(timeout=300)
        assert p.returncode == 0, errs[t]
    want, _, _, _ = tp.restate(cov["recs"], ALPHABET, k_t=K_08)
    want_cover = pc.cover_restate(cov["recs"], ALPHABET, list(want))
    assert (tmp_path / "cov.bed").read_text() == pc.bed18_text(want, want_cover, ALPHABET, REFS)
    assert (tmp_path / "cov.tsv").read_text() == pc.tsv_text(want, want_cover, ALPHABET, REFS)
    assert (tmp_path / "plain.bed").read_text() == tp.bed_text(want, ALPHABET, REFS)
    assert (tmp_path / "plain.tsv").read_text() == tp.tsv_text(want, ALPHABET, REFS)
    totals = [sum(v[c] for v in want_cover.values()) for c in range(3)]
    assert f"N_delete {totals[0]}, N_diff {totals[1]}, N_nocall {totals[2]}" in errs["cov"] and "N_delete" not in errs["plain"]
