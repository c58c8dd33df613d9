"""`analyze pileup_modbams --duplex / --hemi`, the host side: the plain-Python restatement of the rules (written here from
mr.parse_mm_ml, mr.entry_positions and mr.aligned_pairs: the entries in tag order with the both-strands rule, then the pairing by
reference position per record), the synthetic input the GPU tests run and what it must contain, the refusals of --hemi, the
writers on a hand-made hemi table and the new symbols of the C ABI.  No GPU."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import modbam_restate as mr
import test_gpu_pileup as tp
import test_gpu_pileup_ref as tgr
from conftest import ROOT

REFS = tp.REFS
NEW_SYMBOLS = ("rmr_pileup_emit_counts", "rmr_pileup_emit_fill", "rmr_pileup_pair_counts", "rmr_pileup_pair_fill",
               "rmr_pileup_create_cols")


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def record_calls(rec, alphabet):
    """(status, [(ref_id, pos, effective strand, class, kmax)]) of one record by the rules of a --duplex run."""
    mods = list(alphabet[1:])
    reverse = bool(rec["flag"] & 0x10)
    if rec["mm"] is None:
        return 1, []
    try:
        entries = mr.parse_mm_ml(rec["mm"], rec["ml"])
    except mr.Malformed:
        return 2, []
    if rec["ref_id"] < 0 or rec["flag"] & 0x4:
        return 3, []
    if rec["flag"] & 0x900:
        return 6, []
    # an entry counts: strand + or -, letter codes (no ChEBI number), one of them in the alphabet; the base letter is not asked
    counting = [any(c in mods for c in codes) for _, _, codes, _, _, _ in entries]
    if not any(counting):
        return 5, []
    if sum(n for op, n in rec["cigar"] if op in "MIS=X") != len(rec["seq"]):
        return 2, []
    try:  # a call beyond the last occurrence of its base, in any entry
        positions = [mr.entry_positions(rec["seq"], reverse, base, deltas) for base, _, _, _, deltas, _ in entries]
    except mr.Malformed:
        return 2, []
    called = {}  # stored position -> [entry strand, {code: 512 p}]
    for (_, strand, codes, _, _, rows), pos, counts in zip(entries, positions, counting):  # tag order
        if not counts:
            continue
        for p, row in zip(pos, rows):
            if p not in called or called[p][0] != strand:  # the last entry's strand decides; the other strand's values are dropped
                called[p] = [strand, {}]
            for c, code in enumerate(codes):
                if code in mods:
                    called[p][1][code] = 2 * row[c] + 1  # the later entry wins
    q2r = {q: r for q, r, _ in mr.aligned_pairs(rec["cigar"], rec["pos"]) if q is not None and r is not None}
    out = []
    for p in sorted(called):
        r = q2r.get(p)
        if r is None:
            continue
        strand, ks = called[p]
        cols = [512 - sum(ks.get(m, 0) for m in mods)] + [ks.get(m, 0) for m in mods]
        cls = int(np.argmax(cols))
        out.append((rec["ref_id"], r, int(reverse) ^ int(strand == "-"), cls, cols[cls]))
    return 0, out


def _threshold(calls, k_t, pct):
    hist = np.bincount([c[4] for c in calls], minlength=513) if calls else np.zeros(513, np.int64)
    if k_t is None:
        allowed = (Fraction(len(calls)) * Fraction(str(pct)) / 100).__floor__()
        k_t = max(k for k in range(514) if int(hist[:k].sum()) <= allowed)
    return k_t, hist


def restate(records, alphabet, k_t=None, pct=None, region=None, genome=None, motifs=None, combine=False):
    """A --duplex run, with a genome the motif test (and the fold) on the effective strand -> (table {(ref_id, pos, strand):
    [counts]}, k_t, histogram, statuses)."""
    calls, statuses = [], []
    for rec in records:
        st, cs = record_calls(rec, alphabet)
        statuses.append(st)
        if genome is not None:
            cs = [p for p in (tgr.place(c, genome, motifs, combine) for c in cs) if p is not None]
        calls += [c for c in cs if tp.in_region(c, region)]
    k_t, hist = _threshold(calls, k_t, pct)
    ncol = len(alphabet) + 1
    table = {}
    for rid, pos, strand, cls, kmax in calls:
        table.setdefault((rid, pos, strand), [0] * ncol)[cls if kmax >= k_t else ncol - 1] += 1
    return table, k_t, hist, statuses


def hemi_record(rec, alphabet, genome, motif, region=None):
    """One record -> (kept single calls, [(ref_id, rp, '+' call, '-' call)] pairs, unpaired calls).  A call is kept where the motif
    stands around it on its effective strand and the '+' position of its window lies in the region; the '+' call at rp and the
    '-' call at rp + d are a pair."""
    d = len(motif[0]) - 1 - 2 * motif[1]
    kept = []
    for c in record_calls(rec, alphabet)[1]:
        if tgr.place(c, genome, [motif], False) is not None and tp.in_region((c[0], c[1] - d if c[2] else c[1]), region):
            kept.append(c)
    plus = {c[1]: c for c in kept if c[2] == 0}
    minus = {c[1]: c for c in kept if c[2] == 1}
    pairs = [(c[0], rp, c, minus[rp + d]) for rp, c in sorted(plus.items()) if rp + d in minus]
    paired = {id(x) for _, _, a, b in pairs for x in (a, b)}
    return kept, pairs, [c for c in kept if id(c) not in paired]


def restate_hemi(records, alphabet, genome, motif, k_t=None, pct=None, region=None):
    """-> (table {(ref_id, rp): [(n_mods + 2)^2 counts]}, k_t, histogram of all kept single calls, n_unpaired, per-record
    (kept, pairs, unpaired))."""
    per_record = [hemi_record(rec, alphabet, genome, motif, region) for rec in records]
    k_t, hist = _threshold([c for kept, _, _ in per_record for c in kept], k_t, pct)
    nc = len(alphabet) + 1
    table = {}
    for _, pairs, _ in per_record:
        for rid, rp, a, b in pairs:
            ca, cb = (a[3] if a[4] >= k_t else nc - 1), (b[3] if b[4] >= k_t else nc - 1)
            table.setdefault((rid, rp), [0] * (nc * nc))[ca * nc + cb] += 1
    return table, k_t, hist, sum(len(u) for _, _, u in per_record), per_record


def same_hemi_table(got, want, alphabet):
    keys, nc = sorted(want), len(alphabet) + 1
    assert got.hemi and got.combined and got.counts.dtype == np.int64 and got.counts.shape == (len(keys), nc * nc)
    assert list(zip(got.ref_id.tolist(), got.pos.tolist())) == keys and not got.strand.any()
    assert got.counts.tolist() == [want[k] for k in keys]
    assert got.n_calls == sum(sum(r) for r in want.values())


def hemi_bed_text(table, alphabet, refs, min_coverage=1):
    na, nc, out = len(alphabet), len(alphabet) + 1, []
    names = ["-"] + list(alphabet[1:])
    for (rid, pos), row in sorted(table.items()):
        nv = sum(row[a * nc + b] for a in range(na) for b in range(na))
        if nv < max(min_coverage, 1):
            continue
        for a in range(na):
            for b in range(na):
                out.append(f"{refs[rid][0]}\t{pos}\t{pos + 1}\t{names[a]},{names[b]},{alphabet[0]}\t{min(nv, 1000)}\t.\t{pos}\t{pos + 1}\t255,0,0\t{nv}\t"
                           f"{100 * row[a * nc + b] / nv:.2f}\n")
    return "".join(out)


def hemi_tsv_text(table, alphabet, refs):
    cls = list(alphabet) + ["fail"]
    head = "\t".join(["chrom", "start", "strand"] + [f"N_{a}_{b}" for a in cls for b in cls]) + "\n"
    return head + "".join(f"{refs[rid][0]}\t{pos}\t.\t" + "\t".join(map(str, row)) + "\n" for (rid, pos), row in sorted(table.items()))


# ---- the synthetic input --------------------------------------------------------------------------------------------------------
SEED = 41
CG, GC, GATC = ("CG", 0), ("GC", 1), ("GATC", 1)
CAUSES = ("g_deleted", "g_clipped", "g_inserted", "g_unlisted", "simplex")


def _occurrences(seq, reverse, base):
    """How often the ORIGINAL sequence has `base`."""
    return seq.count(mr.COMP[base]) if reverse else seq.count(base)


def synthetic():
    """-> (records, genome, planted): duplex-style records cut from two contigs of 2 kb on both record strands - every C carries
    C+hm?, every G G-hm?, every A A+a? and every T T-a? - then one named record per way a call loses its partner, the two
    records that meet between the C and the G of one CpG, and the edge records of the walk.  planted: the positions used."""
    rng = np.random.default_rng(SEED)
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    genome = [list(rand(2000)), list(rand(2000))]
    for g in genome:  # GATC is rare in random text
        for at in range(40, 1960, 60):
            g[at : at + 4] = "GATC"
    genome[0][300:306], genome[0][1000:1004] = "AACGTT", "TCGA"  # the CpG at 302 of the unpaired causes, the one at 1001 of the meeting records
    genome[0][1998:2000], genome[1][1998:2000] = "CG", "GC"  # the last base of a contig: a G, a C
    genome = ["".join(g) for g in genome]

    def two(n):  # (h, m) of n calls: a clear h, a clear m, a clear canonical base, undecided
        out = []
        for kind in rng.integers(0, 4, n):
            lo, hi = int(rng.integers(0, 25)), int(rng.integers(190, 230))
            mid = int(rng.integers(70, 110))
            out += [[hi, lo], [lo, hi], [lo, lo // 2], [mid, 180 - mid]][kind]
        return out

    def one(n):
        return [int(x) for x in rng.choice([3, 20, 128, 235, 250], n)]

    def duplex(seq, cigar, rev, ref, pos, name=None, g_entry=True, g_every=1):
        occ = lambda b: _occurrences(seq, rev, b)  # noqa: E731
        mm = "C+hm?" + ",0" * occ("C") + ";"
        ml = two(occ("C"))
        if g_entry:
            n_g = occ("G") // g_every  # (g_every 2: the second, the fourth, ... G)
            mm += "G-hm?" + f",{g_every - 1}" * n_g + ";"
            ml += two(n_g)
        mm += "A+a?" + ",0" * occ("A") + ";T-a?" + ",0" * occ("T") + ";"
        ml += one(occ("A")) + one(occ("T"))
        rec = tp._rec(seq, cigar, mm, ml, flag=16 if rev else 0, ref=ref, pos=pos)
        if name:
            rec["name"] = name
        return rec

    recs, g = [], genome[0]
    for i in range(40):
        ref, rev = i % 2, (i // 2) % 2 == 1
        n = int(rng.integers(600, 1100))
        pos = int(rng.integers(0, 2000 - n))
        recs.append(duplex(genome[ref][pos : pos + n], [("M", n)], rev, ref, pos))
    # the C of the CpG at 302 is called on '+', its G is ...
    recs.append(duplex(g[272:303] + g[304:334], [("M", 31), ("D", 1), ("M", 30)], False, 0, 272, "g_deleted"))
    recs.append(duplex(g[272:303] + g[303:308], [("M", 31), ("S", 5)], False, 0, 272, "g_clipped"))
    recs.append(duplex(g[272:303] + "GA" + g[304:334], [("M", 31), ("I", 2), ("D", 1), ("M", 30)], True, 0, 272, "g_inserted"))
    s = next(s for s in range(200, 260) if g[s:303].count("G") % 2 == 0)  # the G at 303 is an odd one of its read: not listed
    recs.append(duplex(g[s:400], [("M", 400 - s)], False, 0, s, "g_unlisted", g_every=2))
    recs.append(duplex(g[200:400], [("M", 200)], True, 0, 200, "simplex", g_entry=False))
    # two records meet between the C and the G of the CpG at 1001: neighbours in the file, so neighbours in the fill
    recs.append(duplex(g[960:1002], [("M", 42)], False, 0, 960, "ends_on_c"))
    recs.append(duplex(g[1002:1040], [("M", 38)], False, 0, 1002, "starts_on_g"))
    # the edges of the walk
    recs.append(duplex(g[100:356], [("M", 256)], False, 0, 100, "len256"))
    recs.append(duplex(g[100:357], [("M", 257)], True, 0, 100, "len257"))
    s = rand(350)
    recs.append(duplex(s, [("M", 2), ("I", 1), ("M", 2), ("D", 1)] * 70, False, 1, 900, "many_ops"))
    recs.append(duplex(genome[0][1900:2000], [("M", 100)], False, 0, 1900, "end_fwd"))
    recs.append(duplex(genome[1][1900:2000], [("M", 100)], True, 1, 1900, "end_rev"))
    # N+m / N-m on one position, in both orders; C+m then C-m on one base; a '-'-only record; a ChEBI '-' entry
    recs.append(dict(tp._rec(g[600:700], [("M", 100)], "N+m?,3,5;N-m?,3,2;", [200, 210, 220, 30], pos=600), name="n_plus_minus"))
    recs.append(dict(tp._rec(g[600:700], [("M", 100)], "N-m?,3,5;N+m?,3,2;", [200, 210, 220, 30], flag=16, ref=1, pos=600), name="n_minus_plus"))
    recs.append(dict(tp._rec("C" * 30, [("M", 30)], "C+hm?,0,1;C-m?,0,4;C+h?,9;", [10, 20, 30, 40, 250, 240, 99], pos=1200), name="c_plus_minus"))
    recs.append(dict(tp._rec(g[0:100], [("M", 100)], "G-m,3,1;", [77, 201], pos=0), name="minus_only"))
    recs.append(dict(tp._rec(g[700:900], [("M", 200)], "G-76792,4;C+m.,0,2;G-m?,1;", [9, 100, 150, 222], pos=700), name="chebi_minus"))
    # skipped whole also with --duplex
    recs.append(dict(tp._rec(g[0:100], [("M", 100)], "G-m?,99;", [5], pos=0), name="beyond_the_last_g"))
    recs.append(dict(tp._rec(g[0:100], [("M", 100)], "G-a?,0;", [5], pos=0), name="not_of_the_alphabet"))
    return recs, genome, dict(cpg=302, meet=1001)


SYNTH = None


def synth():
    """synthetic(), computed once for this file and for test_gpu_pileup_duplex.py and left unchanged."""
    global SYNTH
    if SYNTH is None:
        SYNTH = synthetic()
    return SYNTH


def by_name(recs, name):
    return next(r for r in recs if r.get("name") == name)


# ---- what the input must contain, asked of the restatement alone -----------------------------------------------------------------
@pytest.mark.parametrize("alphabet,n_codes", [(["C", "m"], 9), (["C", "h", "m"], 16)])
@pytest.mark.parametrize("kw", [dict(k_t=307), dict(pct=10)], ids=["k307", "pct10"])
def test_synthetic_input_holds_every_pattern(alphabet, n_codes, kw):
    recs, genome, _ = synth()
    table, k_t, hist, n_unpaired, per_record = restate_hemi(recs, alphabet, genome, CG, **kw)
    total = np.sum(list(table.values()), axis=0)
    assert total.size == n_codes and (total > 0).all(), total  # every pattern code occurs
    assert sum(1 for (rid, rp) in table if sum(1 for _, pairs, _ in per_record if any(p[:2] == (rid, rp) for p in pairs)) >= 3) >= 20
    n_kept = int(hist.sum())
    assert 0 < n_unpaired < n_kept / 2 and n_kept == n_unpaired + 2 * int(total.sum())
    assert 0 < k_t < 512


def test_synthetic_input_holds_every_way_to_lose_a_partner():
    recs, genome, planted = synth()
    alphabet = ["C", "h", "m"]
    x = planted["cpg"]
    assert genome[0][x : x + 2] == "CG" and any(r["flag"] & 16 for r in recs) and any(not r["flag"] & 16 for r in recs)
    for name in CAUSES:
        kept, pairs, unpaired = hemi_record(by_name(recs, name), alphabet, genome, CG)
        # the call that is left: the C's on '+' - in the simplex record, a reverse one with C+hm? alone, the G's on '-'
        at, on = (x + 1, 1) if name == "simplex" else (x, 0)
        assert any(c[1] == at and c[2] == on for c in unpaired), name
        assert not any(rp == x for _, rp, _, _ in pairs) and not any(c[1] == 2 * x + 1 - at for c in kept), name
    assert by_name(recs, "g_inserted")["flag"] & 16 and by_name(recs, "simplex")["flag"] & 16 and not by_name(recs, "g_deleted")["flag"] & 16
    # a full duplex record over the same CpG does pair it
    assert any(any(rp == x and rid == 0 for rid, rp, _, _ in hemi_record(r, alphabet, genome, CG)[1]) for r in recs[:40])
    # the two records that meet inside a CpG: one call each, no pair
    m = planted["meet"]
    a, b = by_name(recs, "ends_on_c"), by_name(recs, "starts_on_g")
    assert recs.index(b) == recs.index(a) + 1 and genome[0][m : m + 2] == "CG"
    assert any(c[1] == m and c[2] == 0 for c in hemi_record(a, alphabet, genome, CG)[2])
    assert any(c[1] == m + 1 and c[2] == 1 for c in hemi_record(b, alphabet, genome, CG)[2])
    # the other motifs have pairs too: GC 1 (d = -1) on the same entries, GATC 1 on the A / T entries
    for motif, alpha in ((GC, ["C", "m"]), (GATC, ["A", "a"])):
        table, _, _, n_unpaired, _ = restate_hemi(recs, alpha, genome, motif, k_t=307)
        assert len(table) >= 20 and n_unpaired > 0 and np.sum(list(table.values()), axis=0).min() > 0, motif


def test_synthetic_input_holds_the_edges_of_the_duplex_walk():
    recs, genome, _ = synth()
    alphabet = ["C", "h", "m"]
    table, k_t, hist, statuses = restate(recs, alphabet, pct=10)
    plain = tp.restate(recs, alphabet, pct=10)
    assert 50 <= len(recs) <= 70 and statuses.count(0) == len(recs) - 2 and statuses.count(2) == 1 and statuses.count(5) == 1
    assert plain[3].count(5) == 3  # without the flag the '-'-only records have nothing of the alphabet
    for rid in (0, 1):
        for strand in (0, 1):
            assert any(k[0] == rid and k[2] == strand for k in table)
    assert hist.sum() > 1.8 * plain[2].sum()  # the '-' entries about double the calls
    calls = lambda name: record_calls(by_name(recs, name), alphabet)[1]  # noqa: E731
    # N+m then N-m on position 603: the '-' entry is the last, the call lies on '-' with its value; 609 is '+' only, 606 '-' only
    assert [(c[1], c[2], c[4]) for c in calls("n_plus_minus")] == [(603, 1, 441), (606, 1, 451), (609, 0, 421)]
    # the reverse record, the other order: stored positions 96 / 93 / 90 -> 696 / 693 / 690; the last entry is '+' : the record's strand
    assert [(c[1], c[2], c[4]) for c in calls("n_minus_plus")] == [(690, 0, 421), (693, 1, 451), (696, 1, 441)]
    # C+hm? (bases 0, 2), C-m? (bases 0, 5), C+h? (base 9): base 0 is '-' with m = 250 alone; h of the '+' entry is dropped
    assert [(c[1], c[2], c[3], c[4]) for c in calls("c_plus_minus")] == [(1200, 1, 2, 501), (1202, 0, 0, 512 - 61 - 81), (1205, 1, 2, 481),
                                                                            (1209, 0, 0, 512 - 199)]
    assert len(calls("minus_only")) == 2 and all(c[2] == 1 for c in calls("minus_only")) and tp.record_calls(by_name(recs, "minus_only"), alphabet)[0] == 5
    assert len(calls("chebi_minus")) == 3 and sorted(c[2] for c in calls("chebi_minus")) == [0, 0, 1]
    assert len(by_name(recs, "len256")["seq"]) == 256 and len(by_name(recs, "len257")["seq"]) == 257 and len(by_name(recs, "many_ops")["cigar"]) > 256
    assert any(k == (0, 1999, 1) for k in table) and any(k == (1, 1999, 0) for k in table)  # G-hm? of a forward, of a reverse record
    assert any(k == (0, 1998, 0) for k in table) and any(k == (1, 1998, 1) for k in table)


# ---- the refusals of --hemi -----------------------------------------------------------------------------------------------------
REFUSALS = [
    (dict(ref=None), "--hemi needs --ref"),
    (dict(motifs=[("CG", 0), ("GC", 1)]), r"--hemi takes exactly one motif.*got 2"),
    (dict(motifs=None), r"--hemi takes exactly one motif.*got 0"),
    (dict(motifs=[("CHG", 0)]), "--hemi: the motif CHG is not its own reverse complement"),
    (dict(alphabet=["C", "h", "m", "f"]), r"at most two --mod-bases, got 3 \(h m f\)"),
    (dict(combine_strands=True), "--hemi implies the fold of --combine-strands"),
    (dict(partition_tag="HP"), "--hemi with --partition-tag is not built"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[m[:24] for _, m in REFUSALS])
def test_hemi_refusals_name_the_argument_and_touch_no_gpu(monkeypatch, tmp_path, change, message):
    from remora_amd import RemoraError, engine, pileup

    def no_gpu(*a, **k):
        raise AssertionError("the engine was asked for")

    monkeypatch.setattr(engine, "get_engine", no_gpu)
    monkeypatch.setattr(pileup, "bam_reference_dict", no_gpu)  # (and no file is opened)
    args = dict(ref="genome.fa", motifs=[("CG", 0)], combine_strands=False, partition_tag=None, alphabet=["C", "m"])
    args.update(change)
    with pytest.raises(RemoraError, match=message):
        pileup.check_hemi_arguments(args["ref"], args["motifs"], args["combine_strands"], args["partition_tag"], args["alphabet"])
    with pytest.raises(RemoraError, match=message):
        pileup.pileup_modbams("reads.bam", args["alphabet"], filter_threshold=0.6, pct_filt=None, ref=args["ref"], motifs=args["motifs"],
                              combine_strands=args["combine_strands"], partition_tag=args["partition_tag"], hemi=True)
    d = pileup.check_hemi_arguments("genome.fa", [("GATC", 1)], False, None, ["A", "a"])
    assert (d.motif, d.shift) == ("GATC", 1) and pileup.check_hemi_arguments("g.fa", [("GC", 1)], False, None, ["C", "h", "m"]).shift == -1


def test_command_line_takes_and_refuses_the_flags(monkeypatch, tmp_path, capsys):
    from remora_amd import engine
    from remora_amd.__main__ import build_parser, main

    base = ["analyze", "pileup_modbams", "--bam", "a.bam", "--out-bed", str(tmp_path / "s.bed"), "--canonical-base", "C", "--mod-bases", "m"]
    a = build_parser().parse_args(base)
    assert a.duplex is False and a.hemi is False
    a = build_parser().parse_args(base + ["--duplex", "--hemi"])
    assert a.duplex is True and a.hemi is True
    monkeypatch.setattr(engine, "get_engine", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the engine was asked for")))
    for extra, message in ((["--hemi"], "--hemi needs --ref"), (["--hemi", "--ref", "g.fa"], "--ref needs a motif"),
                           (["--hemi", "--ref", "g.fa", "--cpg", "--combine-strands"], "--hemi implies the fold"),
                           (["--hemi", "--ref", "g.fa", "--motif", "CG", "0", "--motif", "GC", "1"], "exactly one motif"),
                           (["--hemi", "--ref", "g.fa", "--cpg", "--partition-tag", "HP"], "--partition-tag is not built"),
                           (["--hemi", "--ref", "g.fa", "--cpg", "--mod-bases", "h", "m", "f"], "at most two --mod-bases")):
        assert main(base + extra) == 1 and message in capsys.readouterr().err, extra
    assert not (tmp_path / "s.bed").exists()


# ---- the writers ----------------------------------------------------------------------------------------------------------------
def test_writers_on_a_hand_made_hemi_table(tmp_path):
    from remora_amd.pileup import PileupTable, write_bedmethyl, write_counts

    # codes a * 3 + b for ["C", "m"]: C_C C_m C_fail m_C m_m m_fail fail_C fail_m fail_fail
    counts = np.array([[1, 2, 0, 3, 4, 5, 0, 0, 6], [0, 0, 1, 0, 0, 0, 2, 0, 3], [0, 0, 0, 0, 1200, 0, 0, 0, 0]], np.int64)
    table = PileupTable(ref_names=["ctgA", "ctgB"], ref_id=np.array([0, 0, 1], np.int32), pos=np.array([5, 9, 0], np.int64),
                        strand=np.zeros(3, np.uint8), counts=counts, alphabet=["C", "m"], threshold_k=300, n_calls=int(counts.sum()), n_flushes=1,
                        peak_device_bytes=0, hist=None, combined=True, hemi=True, n_unpaired=7)
    assert table.hemi and table.n_unpaired == 7 and not PileupTable(*table).hemi
    bed, tsv = tmp_path / "h.bed", tmp_path / "h.tsv"
    assert write_bedmethyl(table, bed) == 8 and write_counts(table, tsv) == 3
    row = lambda c, p, name, nv, pct: f"{c}\t{p}\t{p + 1}\t{name}\t{min(nv, 1000)}\t.\t{p}\t{p + 1}\t255,0,0\t{nv}\t{pct}\n"  # noqa: E731
    assert bed.read_text() == (row("ctgA", 5, "-,-,C", 10, "10.00") + row("ctgA", 5, "-,m,C", 10, "20.00") + row("ctgA", 5, "m,-,C", 10, "30.00") +
                               row("ctgA", 5, "m,m,C", 10, "40.00") + row("ctgB", 0, "-,-,C", 1200, "0.00") + row("ctgB", 0, "-,m,C", 1200, "0.00") +
                               row("ctgB", 0, "m,-,C", 1200, "0.00") + row("ctgB", 0, "m,m,C", 1200, "100.00"))
    assert tsv.read_text() == ("chrom\tstart\tstrand\tN_C_C\tN_C_m\tN_C_fail\tN_m_C\tN_m_m\tN_m_fail\tN_fail_C\tN_fail_m\tN_fail_fail\n"
                               "ctgA\t5\t.\t1\t2\t0\t3\t4\t5\t0\t0\t6\nctgA\t9\t.\t0\t0\t1\t0\t0\t0\t2\t0\t3\nctgB\t0\t.\t0\t0\t0\t0\t1200\t0\t0\t0\t0\n")
    # the site whose pairs all hold a failing call (N_valid 0) is in the counts file only; --min-coverage asks N_valid
    assert write_bedmethyl(table, bed, min_coverage=11) == 4 and bed.read_text().startswith("ctgB\t0\t1\t-,-,C\t1000\t.")
    assert write_bedmethyl(table, bed, min_coverage=1201) == 0 and bed.read_text() == ""
    want = {(0, 5): counts[0].tolist(), (0, 9): counts[1].tolist(), (1, 0): counts[2].tolist()}
    write_bedmethyl(table, bed)
    assert bed.read_text() == hemi_bed_text(want, ["C", "m"], REFS) and tsv.read_text() == hemi_tsv_text(want, ["C", "m"], REFS)
    # three classes: (n_mods + 1)^2 = 9 rows a site, ordered by the '+' class, then the '-' class
    t3 = PileupTable(ref_names=["ctgA"], ref_id=np.zeros(1, np.int32), pos=np.array([7], np.int64), strand=np.zeros(1, np.uint8),
                     counts=np.arange(16, dtype=np.int64)[None, :], alphabet=["C", "h", "m"], threshold_k=0, n_calls=120, n_flushes=1,
                     peak_device_bytes=0, hist=None, combined=True, hemi=True, n_unpaired=0)
    assert write_bedmethyl(t3, bed) == 9
    names = [line.split("\t")[3] for line in bed.read_text().splitlines()]
    assert names == ["-,-,C", "-,h,C", "-,m,C", "h,-,C", "h,h,C", "h,m,C", "m,-,C", "m,h,C", "m,m,C"]
    nv = sum(a * 4 + b for a in range(3) for b in range(3))
    assert bed.read_text().splitlines()[5] == f"ctgA\t7\t8\th,m,C\t{nv}\t.\t7\t8\t255,0,0\t{nv}\t{100 * 6 / nv:.2f}"
    write_counts(t3, tsv)
    assert tsv.read_text().splitlines()[0].split("\t")[3:] == [f"N_{a}_{b}" for a in ("C", "h", "m", "fail") for b in ("C", "h", "m", "fail")]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from remora_amd import _lib
    from remora_amd.pileup import bytes_per_buffered_call

    hdr = open(os.path.join(ROOT, "include", "remora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
        assert any(name in c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S)), name
    assert "k_pileup_duplex.hip" in open(os.path.join(ROOT, "remora_amd", "csrc", "Makefile")).read()
    # the emit pair, duplex and hemi in its options struct; the pair passes
    assert len(_lib.SIGNATURES["rmr_pileup_emit_counts"][1]) == 9 and len(_lib.SIGNATURES["rmr_pileup_emit_fill"][1]) == 10
    assert [n for n, _ in _lib.PileupEmitOpts._fields_][-2:] == ["duplex", "hemi"]
    assert len(_lib.SIGNATURES["rmr_pileup_pair_counts"][1]) == 6 and len(_lib.SIGNATURES["rmr_pileup_pair_fill"][1]) == 8
    assert bytes_per_buffered_call(15) == 52 + 4 * 16  # a hemi table of 16 columns
