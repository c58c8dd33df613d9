"""`analyze pileup_modbams --ref`: the reference genome packed on the GPU (rmr_ref_genome_*), and the motif test and the strand
fold inside the emit, against plain Python written here: the IUPAC codes of a string, and the restatement of
test_gpu_pileup.py extended with the genome - string matching on Python strings, then the fold.  Every comparison is exact."""
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import modbam_restate as mr
import test_gpu_pileup as tp
from conftest import ROOT

REFS, ALPHABET = tp.REFS, tp.ALPHABET
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT",
         "H": "ACT", "V": "ACG", "N": "ACGT"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K", "B": "V", "V": "B", "D": "H", "H": "D",
        "N": "N"}
LETTERS = "ACGTURYSWKMBDHVN"

MOTIF_SETS = {
    "C": ([("C", 0)], False),
    "CG": ([("CG", 0)], False),
    "CHH_CHG": ([("CHH", 0), ("CHG", 0)], False),
    "GC": ([("GC", 1)], False),
    "CN": ([("CN", 0)], False),
    "CG_comb": ([("CG", 0)], True),
    "GC_comb": ([("GC", 1)], True),
    "CG_GC_comb": ([("CG", 0), ("GC", 1)], True),
    "GC_CG_comb": ([("GC", 1), ("CG", 0)], True),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---- 1. the pack kernel -------------------------------------------------------------------------------------------------------
def codes_of(seq):
    """A 1, C 2, G 4, T / U 8, an ambiguity letter the union; either case."""
    return np.array([sum({"A": 1, "C": 2, "G": 4, "T": 8}[b] for b in IUPAC[c.upper()]) for c in seq], np.uint8)


def fasta_text(contigs, width, eol="\n"):
    return "".join(f">{name} test contig{eol}" + "".join(seq[i : i + width] + eol for i in range(0, len(seq), width)) for name, seq in contigs)


def pack_contigs():
    rng = np.random.default_rng(5)
    both = LETTERS + LETTERS.lower()
    out = [(f"len{n}", "".join(rng.choice(list(both), n))) for n in (1, 2, 3, 59, 60, 61, 120, 121)]
    return out + [("letters", both)]


@pytest.mark.gpu
@pytest.mark.parametrize("width,eol", [(60, "\n"), (1, "\n"), (7, "\n"), (60, "\r\n"), (7, "\r\n")])
def test_pack_kernel_equals_python_codes(torch_cuda, tmp_path, width, eol):
    from remora_amd.pileup import RefGenome

    contigs = pack_contigs()
    path = tmp_path / "g.fa"
    path.write_bytes(fasta_text(contigs, width, eol).encode())
    names, lens, n_open = [c[0] for c in contigs], [len(c[1]) for c in contigs], RefGenome.n_open
    with RefGenome.from_fasta(path, names, lens, piece_bytes=64) as g:  # pieces end inside contigs and inside lines
        assert g.device_bytes >= sum((n + 1) // 2 for n in lens) and RefGenome.n_open == n_open + 1
        for name, seq in contigs:
            want = codes_of(seq)
            assert np.array_equal(g.read(name), want), name
            n = len(seq)
            for lo, hi in ((0, n), (1, n), (0, n - 1), (1, n - 1), (n // 2, n // 2 + 1), (n // 2 | 1, n), (2, 2), (n, n)):
                if 0 <= lo <= hi <= n:
                    assert np.array_equal(g.read(name, lo, hi), want[lo:hi]), (name, lo, hi)
        assert set(g.read("letters").tolist()) == set(range(1, 16))
    assert RefGenome.n_open == n_open
    # only some contigs asked for, in another order than the file's, at the default piece size
    with RefGenome.from_fasta(path, names[::-1], lens[::-1], contigs=["len121", "len1"]) as g:
        assert np.array_equal(g.read("len121"), codes_of(dict(contigs)["len121"])) and np.array_equal(g.read("len1"), codes_of(dict(contigs)["len1"]))
        with pytest.raises(Exception, match="len60 was not loaded"):
            g.read("len60")


@pytest.mark.gpu
@pytest.mark.parametrize("case,line,what", [("short_line", 8, "the line has 5 bases"), ("digit", 9, "not an IUPAC letter"),
                                            ("cr_in_lf", 7, "does not end after 8 bases")])
def test_pack_kernel_refuses_what_the_host_did_not_look_at(torch_cuda, tmp_path, case, line, what):
    """The violation sits in the second contig, far enough in for several pieces (piece_bytes 16) to come before it."""
    from remora_amd import RemoraError
    from remora_amd.pileup import RefGenome, fasta_spans

    good = ["ACGTACGT"] * 6
    lines = {"short_line": good[:2] + ["ACGTA"] + good[3:], "digit": good[:3] + ["ACG7ACGT"] + good[4:], "cr_in_lf": good[:1] + ["ACGTACGT\r"] + good[2:]}[case]
    text = ">ok\nACGTACGT\nACGT\n\n>bad one\n" + "\n".join(lines) + "\n"
    path = tmp_path / f"{case}.fa"
    path.write_bytes(text.encode())
    assert text.split("\n")[line - 1] == {"short_line": "ACGTA", "digit": "ACG7ACGT", "cr_in_lf": "ACGTACGT\r"}[case]  # 1-based line of the file
    spans = fasta_spans(path.read_bytes())
    names, lens = [s.name for s in spans], [s.n_bases for s in spans]
    assert names == ["ok", "bad"]
    n_open = RefGenome.n_open
    with pytest.raises(RemoraError, match=rf"contig bad, line {line} \(line {line - 5} of its sequence\): .*{what}") as ei:
        RefGenome.from_fasta(path, names, lens, piece_bytes=16)
    assert ("re-wrap" in str(ei.value)) == (case != "digit") and str(path) in str(ei.value)
    assert RefGenome.n_open == n_open  # nothing is left allocated
    with RefGenome.from_fasta(path, names, lens, contigs=["ok"], piece_bytes=16) as g:  # the contig that is not asked for is not read
        assert np.array_equal(g.read("ok"), codes_of("ACGTACGTACGT"))


# ---- 2. the restatement with the genome -----------------------------------------------------------------------------------------
def matches(ref_letter, motif_letter):
    """Everything the reference allows, the motif allows."""
    return set(IUPAC[ref_letter.upper()]) <= set(IUPAC[motif_letter])


def place(call, genome, motifs, combine):
    """The call where it is written, or None when no motif matches: string matching on the contig's text."""
    rid, pos, strand, cls, kmax = call
    g = genome[rid]
    for motif, f in motifs:
        n = len(motif)
        pattern = motif if strand == 0 else "".join(COMP[c] for c in reversed(motif))
        s = pos - (f if strand == 0 else n - 1 - f)
        if s < 0 or s + n > len(g) or not all(matches(g[s + i], pattern[i]) for i in range(n)):
            continue
        if combine and strand == 1:
            return rid, pos - (n - 1 - 2 * f), 0, cls, kmax
        return rid, pos, 0 if combine else strand, cls, kmax
    return None


def restate_ref(records, genome, motifs, combine, k_t=None, pct=None, region=None):
    """tp.restate with the motif test and the fold in front of the region test -> (table, k_t, histogram, calls before the
    motif test, calls kept)."""
    raw = [c for rec in records for c in tp.record_calls(rec, ALPHABET)[1]]
    placed = [place(c, genome, motifs, combine) for c in raw]
    calls = [c for c in placed if c is not None and tp.in_region(c, region)]
    hist = np.bincount([c[4] for c in calls], minlength=513) if calls else np.zeros(513, np.int64)
    if k_t is None:
        allowed = (Fraction(len(calls)) * Fraction(str(pct)) / 100).__floor__()
        k_t = max(k for k in range(514) if int(hist[:k].sum()) <= allowed)
    ncol = len(ALPHABET) + 1
    table = {}
    for rid, pos, strand, cls, kmax in calls:
        table.setdefault((rid, pos, strand), [0] * ncol)[cls if kmax >= k_t else ncol - 1] += 1
    return table, k_t, hist, raw, calls


def bed_text(table, combine, min_coverage=1):
    text = tp.bed_text(table, ALPHABET, REFS, min_coverage)
    return text.replace("\t+\t", "\t.\t") if combine else text


def tsv_text(table, combine):
    text = tp.tsv_text(table, ALPHABET, REFS)
    return text.replace("\t+\t", "\t.\t") if combine else text


def _genome_and_records():
    """Two contigs of 2 kb with planted edges, and reads cut from them on both strands as tp._synthetic() cuts its own: every C
    of the read called for h and m.  The reads are cut from a sample whose N are bases; a third of them carry substitutions."""
    rng = np.random.default_rng(29)
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    a, b = list(rand(2000)), list(rand(2000))
    a[0], a[1999] = "G", "C"                      # the CG windows of these two calls run off the contig
    b[0:2], b[1998:2000] = "CG", "CG"             # these four are inside
    a[700:704], a[900:903], a[1100:1103] = "ACNA", "GCG", "CGC"
    b[800:804], b[1000:1003], b[1300:1303] = "TNGT", "GCG", "CGC"
    a[1400:1406] = "crCGyn".replace("r", "R").replace("y", "Y").replace("n", "g")  # soft-masked and ambiguous reference letters
    genome = ["".join(a), "".join(b)]
    sample = [g.upper().replace("N", "C").replace("R", "A").replace("Y", "C") for g in genome]
    sample[1] = sample[1][:801] + "A" + sample[1][802:]  # (the N before the G of contig 1: any base)

    def read(ref, rev, pos, n, substitute):
        seq = list(sample[ref][pos : pos + n])
        if substitute:
            for i in rng.choice(n, max(n // 25, 1), replace=False):
                seq[i] = rng.choice([x for x in "ACGT" if x != seq[i]])
        seq = "".join(seq)
        nc = tp._all_c(seq, rev)
        ml = []
        for _ in range(nc):
            h = int(rng.integers(0, 256))
            ml += [h, int(rng.integers(0, 256 - h))]
        return tp._rec(seq, [("M", n)], "C+hm?" + ",0" * nc + ";", ml, flag=16 if rev else 0, ref=ref, pos=pos)

    recs = []
    for i in range(28):
        n = int(rng.integers(500, 900))
        recs.append(read(i % 2, (i // 2) % 2 == 1, int(rng.integers(0, 2000 - n)), n, i % 3 == 0))
    for ref in (0, 1):  # both ends of both contigs on both strands, and the planted stretches
        for rev in (False, True):
            recs += [read(ref, rev, 0, 300, False), read(ref, rev, 1700, 300, False), read(ref, rev, 650, 800, False)]
    syn, _ = tp._synthetic()  # its soft-clip / insertion, deletion and N+m? records: calls wherever they fall on this genome
    recs.append(next(r for r in syn if r["cigar"][0] == ("S", 5)))
    recs.append(next(r for r in syn if ("D", 5) in r["cigar"]))
    recs += [r for r in syn if (r["mm"] or "").startswith("N+")]
    return genome, recs


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    genome, recs = _genome_and_records()
    d = tmp_path_factory.mktemp("pileup_ref")
    bam, fa = str(d / "reads.bam"), str(d / "genome.fa")
    mr.write_bam(bam, REFS, recs)
    with open(fa, "w") as fh:
        fh.write(fasta_text(list(zip([r[0] for r in REFS], genome)), 60))
    return bam, fa, genome, recs


def test_planted_input_is_not_vacuous():
    """Asked of the restatement alone, before anything runs on the GPU."""
    genome, recs = _genome_and_records()
    assert [len(g) for g in genome] == [2000, 2000] and len(recs) == 28 + 12 + 4
    tables = {}
    for tag, (motifs, combine) in MOTIF_SETS.items():
        table, k_t, hist, raw, calls = restate_ref(recs, genome, motifs, combine, pct=10)
        tables[tag] = table
        assert 0 < len(calls) < len(raw), tag  # every set both keeps and drops
        assert 0 < k_t < 512 and hist.sum() == len(calls)
    raw = set(c[:3] for c in restate_ref(recs, genome, [("C", 0)], False, pct=10)[3])
    cg = tables["CG"]
    # the windows that leave contig 0: called, and dropped; those of contig 1 lie inside: kept
    assert {(0, 0, 1), (0, 1999, 0)} <= raw and (0, 0, 1) not in cg and (0, 1999, 0) not in cg
    assert {(1, 0, 0), (1, 1, 1), (1, 1998, 0), (1, 1999, 1)} <= set(cg)
    # [C 0] keeps the last C of contig 0 and drops only calls on a reference non-C (substituted reads, the added records)
    assert (0, 1999, 0) in tables["C"] and any(genome[k[0]][k[1]].upper() not in "CY" for k in raw if k[2] == 0)
    # a reference N matches only a motif N, on both strands
    assert (0, 701, 0) in raw and (0, 701, 0) in tables["CN"] and (0, 701, 0) not in cg and (0, 701, 0) not in tables["CHH_CHG"]
    assert (1, 802, 1) in raw and (1, 802, 1) in tables["CN"] and (1, 802, 1) not in cg
    assert (0, 1999, 0) not in tables["CN"]  # the N of the motif is a base of the window: it leaves the contig
    # soft-masked and ambiguous reference letters: c is C; R Y are not inside CG
    assert (0, 1402, 0) in cg and (0, 1400, 0) in tables["C"]
    # combining: site pairs with calls on both strands become one row
    both = [k for k in cg if k[2] == 0 and (k[0], k[1] + 1, 1) in cg]
    assert len(both) >= 20
    comb = tables["CG_comb"]
    assert all(k[2] == 0 for k in comb) and len(comb) == len({(k[0], k[1] - k[2]) for k in cg})
    assert all(sum(comb[k]) == sum(cg[k]) + sum(cg[(k[0], k[1] + 1, 1)]) for k in both)
    # a site that matches two motifs with different shifts: the order decides where the '-' call on the G of CGC goes
    assert (0, 1101, 1) in raw and (1, 1301, 1) in raw
    one, two = tables["CG_GC_comb"], tables["GC_CG_comb"]
    assert one != two and sum(map(sum, one.values())) == sum(map(sum, two.values()))
    minus = [c for c in restate_ref(recs, genome, [("C", 0)], False, pct=10)[3] if c[:3] == (0, 1101, 1)]
    assert place(minus[0], genome, *MOTIF_SETS["CG_GC_comb"])[1] == 1100 and place(minus[0], genome, *MOTIF_SETS["GC_CG_comb"])[1] == 1102


@pytest.fixture(scope="module")
def device_genome(torch_cuda, planted):
    from remora_amd.pileup import RefGenome

    bam, fa, genome, recs = planted
    g = RefGenome.from_fasta(fa, [r[0] for r in REFS], [r[1] for r in REFS])
    yield g
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(MOTIF_SETS))
def test_motif_sets_equal_the_restatement(torch_cuda, planted, device_genome, tmp_path, tag):
    from remora_amd.pileup import pileup_modbams

    bam, fa, genome, recs = planted
    motifs, combine = MOTIF_SETS[tag]
    for kw, rk in ((dict(filter_threshold=0.6, pct_filt=None), dict(k_t=308)), (dict(pct_filt=10), dict(pct=10))):
        want, k_t, hist, _, calls = restate_ref(recs, genome, motifs, combine, **rk)
        got = pileup_modbams(bam, ALPHABET, ref=device_genome, motifs=motifs, combine_strands=combine, **kw)
        assert got.threshold_k == k_t and got.combined == combine and got.n_calls == len(calls)
        tp.same_table(got, want, ALPHABET)
        if "pct_filt" in kw and kw["pct_filt"] is not None:
            assert np.array_equal(got.hist, hist)
        else:
            assert got.hist is None
        bed, tsv = tp.files_of(got, tmp_path, tag)
        assert bed == bed_text(want, combine) and tsv == tsv_text(want, combine)
        assert got.peak_device_bytes > device_genome.device_bytes
    assert device_genome.h  # a RefGenome given by the caller stays open


# ---- 3. invariance --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_folded_table_does_not_depend_on_buffer_batch_or_file_order(torch_cuda, planted, tmp_path):
    from remora_amd.pileup import RefGenome, pileup_modbams

    bam, fa, genome, recs = planted
    kw = dict(filter_threshold=0.6, pct_filt=None, ref=fa, motifs=[("CG", 0)], combine_strands=True)
    n_open = RefGenome.n_open
    whole = pileup_modbams(bam, ALPHABET, **kw)
    ref_files = tp.files_of(whole, tmp_path, "whole")
    assert whole.n_flushes == 1 and RefGenome.n_open == n_open  # a genome loaded from a path is closed with the run
    want = restate_ref(recs, genome, [("CG", 0)], True, k_t=308)[0]
    assert ref_files == (bed_text(want, True), tsv_text(want, True))
    one = pileup_modbams(bam, ALPHABET, buffer_calls=1, **kw)
    assert one.n_flushes == one.n_calls > 100 and tp.files_of(one, tmp_path, "cap1") == ref_files
    assert tp.files_of(pileup_modbams(bam, ALPHABET, batch=1, **kw), tmp_path, "batch1") == ref_files
    p1, p2 = str(tmp_path / "half1.bam"), str(tmp_path / "half2.bam")
    mr.write_bam(p1, REFS, recs[:19])
    mr.write_bam(p2, REFS, recs[19:])
    by_pct = tp.files_of(pileup_modbams(bam, ALPHABET, ref=fa, motifs=[("CG", 0)], combine_strands=True, pct_filt=10), tmp_path, "pct")
    for tag, order in (("ab", [p1, p2]), ("ba", [p2, p1])):
        assert tp.files_of(pileup_modbams(order, ALPHABET, **kw), tmp_path, tag) == ref_files
        assert tp.files_of(pileup_modbams(order, ALPHABET, ref=fa, motifs=[("CG", 0)], combine_strands=True, pct_filt=10), tmp_path, tag + "p") == by_pct


# ---- 4. the region is asked of the position that is written ---------------------------------------------------------------------
@pytest.mark.gpu
def test_region_after_the_fold(torch_cuda, planted, tmp_path):
    from remora_amd.pileup import pileup_modbams

    bam, fa, genome, recs = planted
    kw = dict(filter_threshold=0.6, pct_filt=None, ref=fa, motifs=[("CG", 0)], combine_strands=True)
    cg = restate_ref(recs, genome, [("CG", 0)], False, k_t=308)[0]
    both = sorted(k[1] for k in cg if k[0] == 1 and k[2] == 0 and (1, k[1] + 1, 1) in cg)
    p1, p2 = both[2], both[-3]
    # from the G of one covered CpG to the C of another: the '-' calls on the first G are written outside, those on the G
    # behind the last C inside
    region = ("ctgB", p1 + 1, p2 + 1)
    whole = pileup_modbams(bam, ALPHABET, **kw)
    got = pileup_modbams(bam, ALPHABET, region=f"ctgB:{p1 + 1}-{p2 + 1}", **kw)
    inside = (whole.ref_id == 1) & (whole.pos >= p1 + 1) & (whole.pos < p2 + 1)
    assert 0 < inside.sum() < whole.pos.size and got.pos.tolist() == whole.pos[inside].tolist()
    assert got.counts.tolist() == whole.counts[inside].tolist() and set(got.ref_id.tolist()) == {1} and not got.strand.any()
    assert got.pos[-1] == p2 and p1 not in got.pos.tolist()
    want = restate_ref(recs, genome, [("CG", 0)], True, k_t=308, region=(1, region[1], region[2]))[0]
    tp.same_table(got, want, ALPHABET)
    assert sum(want[(1, p2, 0)]) == sum(cg[(1, p2, 0)]) + sum(cg[(1, p2 + 1, 1)])  # both strands of the last CpG
    # the percentile of a region is taken over the region's calls
    want, k_t, hist, _, _ = restate_ref(recs, genome, [("CG", 0)], True, pct=10, region=(1, region[1], region[2]))
    got = pileup_modbams(bam, ALPHABET, region=region, pct_filt=10, ref=fa, motifs=[("CG", 0)], combine_strands=True)
    assert got.threshold_k == k_t and np.array_equal(got.hist, hist)
    tp.same_table(got, want, ALPHABET)


# ---- 5. refusals before any pileup launch, and the command line -------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_launch_no_pileup_kernel(torch_cuda, planted, tmp_path):
    from remora_amd import RemoraError
    from remora_amd.engine import get_engine
    from remora_amd.pileup import RefGenome, pileup_modbams

    bam, fa, genome, recs = planted
    short = tmp_path / "short.fa"
    short.write_text(fasta_text([("ctgA", genome[0]), ("ctgB", genome[1][:1999])], 60))
    only_a = tmp_path / "only_a.fa"
    only_a.write_text(fasta_text([("ctgA", genome[0])], 60))
    digit = tmp_path / "digit.fa"
    digit.write_text(fasta_text([("ctgA", genome[0]), ("ctgB", genome[1][:500] + "5" + genome[1][501:])], 60))
    eng = get_engine(None)
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    n_open = RefGenome.n_open
    try:
        for kw, msg in ((dict(ref=str(short), motifs=[("CG", 0)]), r"contig ctgB has 1999 bases .* says 2000"),
                        (dict(ref=str(only_a), motifs=[("CG", 0)]), "no contig ctgB"),
                        (dict(ref=str(digit), motifs=[("CG", 0)]), r"contig ctgB, line \d+ .*not an IUPAC letter"),
                        (dict(ref=fa, motifs=[("CHH", 0)], combine_strands=True), "--combine-strands: the motif CHH is not its own reverse"),
                        (dict(ref=fa, motifs=[("GC", 0)]), "--motif GC 0: the focus base is G"),
                        (dict(ref=fa), "--ref needs a motif"), (dict(motifs=[("CG", 0)]), "--motif needs --ref"),
                        (dict(combine_strands=True), "--combine-strands needs --ref")):
            with pytest.raises(RemoraError, match=msg):
                pileup_modbams(bam, ALPHABET, pct_filt=10, **kw)
        assert not any(k.startswith(("pileup_", "modbam_")) for k in eng.profile()), eng.profile()
        assert RefGenome.n_open == n_open
        # with a region only the region's contig is loaded: the FASTA without ctgB serves ctgA
        got = pileup_modbams(bam, ALPHABET, pct_filt=10, region="ctgA", ref=str(only_a), motifs=[("CG", 0)])
        want = restate_ref(recs, genome, [("CG", 0)], False, pct=10, region=(0, 0, 2000))[0]
        tp.same_table(got, want, ALPHABET)
    finally:
        eng.profile_enable(False)


@pytest.mark.gpu
def test_command_line_writes_the_api_bytes(torch_cuda, planted, tmp_path):
    from remora_amd.pileup import pileup_modbams

    bam, fa, genome, recs = planted
    base = [sys.executable, "-m", "remora_amd", "analyze", "pileup_modbams", "--bam", bam, "--canonical-base", "C", "--mod-bases", "h", "m", "--ref", fa]
    runs = {"comb": ["--cpg", "--combine-strands"], "cpg": ["--cpg"], "two": ["--motif", "CHH", "0", "--motif", "CHG", "0", "--filter-threshold", "0.6"]}
    procs = {t: subprocess.Popen(base + ["--out-bed", str(tmp_path / f"{t}.bed"), "--counts-filename", str(tmp_path / f"{t}.tsv")] + extra,
                                 cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for t, extra in runs.items()}
    for t, p in procs.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, err
    read = lambda t: ((tmp_path / f"{t}.bed").read_text(), (tmp_path / f"{t}.tsv").read_text())  # noqa: E731
    assert read("comb") == tp.files_of(pileup_modbams(bam, ALPHABET, ref=fa, motifs=[("CG", 0)], combine_strands=True), tmp_path, "api_comb")
    assert read("cpg") == tp.files_of(pileup_modbams(bam, ALPHABET, ref=fa, motifs=[("CG", 0)]), tmp_path, "api_cpg")
    want = restate_ref(recs, genome, [("CHH", 0), ("CHG", 0)], False, k_t=308)[0]
    assert read("two") == (bed_text(want, False), tsv_text(want, False))
    strands = lambda text, col: {ln.split("\t")[col] for ln in text.splitlines()}  # noqa: E731
    assert strands(read("comb")[0], 5) == {"."} and strands(read("comb")[1], 2) == {"strand", "."}
    assert strands(read("cpg")[0], 5) == {"+", "-"} and strands(read("cpg")[1], 2) == {"strand", "+", "-"}
