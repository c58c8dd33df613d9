"""`validate from_modbams` on the GPU: parse_mod_bam / validate_modbams on the tagged fixture BAMs against the reference's
arrays and lines (tests/golden/modbams.npz), and hand-built records - every edge of the walk along the bases, of the CIGAR
walk and of the truth lookup - against the plain-Python restatement of the rules (tests/modbam_restate.py).  Every comparison
is exact: the values are integers and multiples of 1/512."""
import os
import subprocess
import sys

import numpy as np
import pytest

import modbam_restate as mr
from conftest import GOLDEN, ROOT, golden

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, "data")
PAIRS = [(os.path.join(DATA, f"{p}_modbam.bam"), os.path.join(DATA, f"{p}_gt.bed")) for p in ("can", "mod")]
REFS = [("chrA", 200000), ("chrB", 200000), ("chrNoTruth", 100000)]
ALPHABET = ["C", "h", "m"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fx():
    return golden("modbams.npz")


def _truth():
    """Sites with gaps (so that the lookup has something to miss) and all three labels, another pattern per strand."""
    return {("chrA", "+"): {p: "Chm"[p % 3] for p in range(900, 120000) if p % 5 != 3},
            ("chrA", "-"): {p: "mhC"[p % 3] for p in range(900, 120000) if p % 7 != 2},
            ("chrB", "+"): {p: "m" for p in range(0, 5000, 2)}}


def _mm(base, strand, codes, ordinals, flag="?"):
    """One MM entry calling the given occurrence ordinals of `base`."""
    deltas = [o - (ordinals[k - 1] + 1 if k else 0) for k, o in enumerate(ordinals)]
    return f"{base}{strand}{codes}{flag}" + "".join(f",{d}" for d in deltas) + ";"


def _rec(seq, cigar, mm, ml, flag=0, ref=0, pos=1000, has_md=True, **kw):
    return dict(seq=seq, flag=flag, ref_id=ref, ref_name=REFS[ref][0] if ref >= 0 else None, pos=pos, cigar=cigar, mm=mm, ml=ml,
                has_md=has_md, **kw)


def _edge_records():
    rng = np.random.default_rng(5)
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    ml = lambda n: rng.integers(0, 256, n).tolist()  # noqa: E731
    recs = []
    recs.append(_rec("C", [("M", 1)], "C+m?,0;", [200], pos=1001))  # a 1-base read
    s = rand(300)
    recs.append(_rec(s, [("M", 300)], _mm("C", "+", "m", [0, s.count("C") - 1]), ml(2)))  # first and last occurrence
    recs.append(_rec("AC" * 600, [("M", 1200)], _mm("C", "+", "m", [63, 64, 65, 255, 256, 300, 599]), ml(7)))  # wave and block edges
    recs.append(_rec("AC" * 10, [("M", 20)], _mm("C", "+", "m", [1]), [9], pos=1001))
    recs.append(_rec("AC" * 10, [("M", 20)], _mm("C", "+", "m", [3, 10]), ml(2), pos=1001))  # one past the last occurrence: malformed
    recs.append(_rec("AC" * 10, [("M", 20)], _mm("C", "+", "m", [9]), [8], pos=1001))
    recs.append(_rec("AC" * 10, [("M", 20)], "C+m?,0;A+a,11;", [1, 2], pos=1001))  # ... in an entry that does not count, too
    s = rand(112)
    recs.append(_rec(s, [("S", 7), ("M", 100), ("S", 5)], _mm("C", "+", "m", list(range(s.count("G")))), ml(s.count("G")), flag=16))
    recs.append(_rec(s, [("S", 7), ("M", 100), ("S", 5)], _mm("C", "+", "hm", [0, 2, s.count("G") - 1]), ml(6), flag=16, pos=2002))
    recs.append(_rec("C" * 55, [("S", 5), ("M", 20), ("I", 6), ("M", 20), ("S", 4)], _mm("C", "+", "m", list(range(55))), ml(55)))  # in I, in S
    recs.append(_rec("C" * 90, [("M", 30), ("D", 5), ("M", 30), ("N", 50), ("M", 30)], _mm("C", "+", "m", list(range(90))), ml(90)))  # D, N
    recs.append(_rec("G" * 90, [("M", 30), ("D", 5), ("M", 30), ("N", 50), ("M", 30)], _mm("C", "+", "m", list(range(90))), ml(90), flag=16))
    recs.append(_rec("C" * 43, [("H", 10), ("=", 20), ("X", 3), ("P", 2), ("=", 20), ("H", 3)], _mm("C", "+", "m", list(range(43))), ml(43)))
    # truth at the alignment's first and last reference position (1000 and 1029 are sites of chrA +; 1003 is a gap)
    recs.append(_rec("C" * 30, [("M", 30)], _mm("C", "+", "m", [0, 3, 29]), ml(3), pos=1000))
    recs.append(_rec("C" * 30, [("M", 30)], _mm("C", "+", "m", [0, 29]), ml(2), pos=899))  # first base in front of every site
    recs.append(_rec("C" * 30, [("M", 30)], _mm("C", "+", "m", [0, 29]), ml(2), pos=119999 - 29))  # last base on the last site
    recs.append(_rec("C" * 30, [("M", 30)], _mm("C", "+", "m", [0, 29]), ml(2), ref=2))  # a contig without truth
    recs.append(_rec("G" * 30, [("M", 30)], _mm("C", "+", "m", [0, 29]), ml(2), ref=1, pos=10, flag=16))  # truth on the other strand only
    recs.append(_rec("C" * 30, [("M", 30)], _mm("C", "+", "m", [0, 29]), ml(2), ref=1, pos=10))
    recs.append(_rec("C" * 30, [], _mm("C", "+", "m", [0, 29]), ml(2), ref=-1, pos=-1, flag=4))  # unmapped
    recs.append(_rec("C" * 30, [("M", 30)], _mm("C", "+", "m", [0, 29]), ml(2), has_md=False))  # no MD
    recs.append(_rec("C" * 30, [("M", 30)], "C+h?,0,1;C+m?,0,1;C+m?,1;", [10, 20, 30, 40, 250]))  # h and m on one base; m twice: later wins
    s = rand(200)
    recs.append(_rec(s, [("M", 200)], "N+m?,0,5,2,189;", ml(4)))  # N counts every base
    recs.append(_rec(s, [("S", 3), ("M", 197)], "N+m?,0,5,2,189;C+h?,1;", ml(5), flag=16))
    recs.append(_rec(s, [("M", 200)], "U+m?,0,1;", ml(2)))  # U counts T
    recs.append(_rec(s, [("M", 200)], "A+a,0,1;C+76792,4;C+m?,0,0;", ml(5)))  # the kept entry's ML lies behind the others'
    recs.append(_rec(s, [("M", 200)], "G-m,3,1;C+m.,0;", ml(3)))  # an ignored entry consumes its ML; flag '.'
    recs.append(_rec(s, [("M", 200)], "G-m,3,1;", ml(2)))  # nothing that counts
    recs.append(_rec(s, [("M", 200)], "C+a,3,1;", ml(2)))
    recs.append(_rec(s, [("M", 200)], "C+m,1,1;", ml(2), tags_lower=True))  # Mm / Ml, no flag
    recs.append(_rec(s, [("M", 200)], None, None))  # no tags
    recs.append(_rec(s, [("M", 200)], "C+m?,1,1;", [5]))  # ML too short
    recs.append(_rec(s, [("M", 199)], "C+m?,1,1;", ml(2)))  # CIGAR shorter than the read
    recs.append(_rec(s, [("M", 200)], "C+m?;", []))  # an entry without calls
    recs.append(_rec("C", [("M", 1)], "C+m?,0;", [255], flag=16, pos=1001))  # (the stored base is C: its original is G - malformed)
    recs.append(_rec("G", [("M", 1)], "C+m?,0;", [255], flag=16, pos=1001))
    return recs


def _big_records():
    rng = np.random.default_rng(6)
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    ml = lambda n: rng.integers(0, 256, n).tolist()  # noqa: E731
    recs = []
    s = rand(70000)  # longer than any tile
    ords = list(range(0, s.count("C"), 7))
    recs.append(_rec(s, [("S", 100), ("M", 30000), ("D", 10), ("M", 20000), ("I", 50), ("M", 19850)], _mm("C", "+", "hm", ords), ml(2 * len(ords)),
                     pos=5000))
    cig = [("M", 3), ("I", 1), ("M", 3), ("D", 2)] * 1250  # 5000 CIGAR ops
    s = rand(8750)
    ords = list(range(s.count("G")))
    recs.append(_rec(s, cig, _mm("C", "+", "m", ords), ml(len(ords)), flag=16, pos=2000))
    recs.append(_rec("C" * 3000, [("M", 3000)], _mm("C", "+", "m", list(range(3000))), ml(3000), pos=40000))  # more calls than threads
    return recs


def _gpu_join(path, alphabet, gt_sites, batch):
    """The batches of a BAM through the tokeniser and the two kernels: (probs, labels, qpos, rpos, counts, status)."""
    from remora_amd.engine import get_engine
    from remora_amd.io import bam_reference_names, iter_bam_raw_batches
    from remora_amd.validate import ModBamTruth, modbam_batch_sites, tokenise_mod_tags

    eng = get_engine(None)
    truth = ModBamTruth(bam_reference_names(path), gt_sites, alphabet, eng.torch_device)
    parts = []
    for rb, _ in iter_bam_raw_batches(path, batch=batch):
        tok = tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off)
        out = modbam_batch_sites(eng, truth, alphabet[1:], rb.seq, rb.seq_off, rb.cigar, rb.cigar_off, rb.flag, rb.ref_id, rb.pos, rb.has, tok)
        parts.append([t.cpu().numpy() for t in out[:4]] + list(out[4:]))
    cat = [np.concatenate([p[i] for p in parts]) for i in range(6)]
    return cat[0].astype(np.float64), cat[1].astype(np.int64), cat[2], cat[3], cat[4], cat[5]


def _same(got, want):
    for g, w, what in zip(got, want, ("probs", "labels", "qpos", "rpos", "counts", "status")):
        assert g.shape == w.shape and np.array_equal(g, w), what


@pytest.fixture(scope="module")
def edge_bam(tmp_path_factory):
    path = tmp_path_factory.mktemp("modbam") / "edges.bam"
    recs = _edge_records()
    mr.write_bam(path, REFS, recs)
    return str(path), recs


def test_hand_built_records_equal_the_restatement(torch_cuda, edge_bam):
    path, recs = edge_bam
    want = mr.join_records(recs, ALPHABET, _truth())
    # the cases are what they are meant to be
    st = want[5].tolist()
    assert st.count(mr.MALFORMED) == 5 and st.count(mr.NO_MM) == 1 and st.count(mr.UNMAPPED) == 1 and st.count(mr.NO_MD) == 1
    assert st.count(mr.NO_VALID) == 2 and want[4][0] == 1 and want[4][2] == 6 and want[4][4] == 0 and want[4][3] == want[4][5] == 1
    assert 0 < want[4][9] < 40 and want[4][16] == 0 and want[4][17] == 0 and st[17] == 0 and want[4][18] > 0
    assert want[4][13] == want[4][15] == 2 and want[4][21] == 3 and want[4][22] > 0 and want[4][23] > 0
    _same(_gpu_join(path, ALPHABET, _truth(), 512), want)
    two = mr.join_records(recs, ["C", "m"], _truth_two())
    assert not np.array_equal(two[4], want[4])
    _same(_gpu_join(path, ["C", "m"], _truth_two(), 512), two)


def _truth_two():
    return {k: {p: ("C" if m == "h" else m) for p, m in v.items()} for k, v in _truth().items()}


def test_long_read_many_cigar_ops_and_many_calls_in_one_batch(torch_cuda, tmp_path):
    recs = _big_records()
    path = str(tmp_path / "big.bam")
    mr.write_bam(path, REFS, recs)
    want = mr.join_records(recs, ALPHABET, _truth())
    assert (want[5] == 0).all() and want[4][0] > 1500 and want[4][1] > 1000 and want[4][2] > 2000
    _same(_gpu_join(path, ALPHABET, _truth(), 512), want)


def test_batch_split_does_not_matter(torch_cuda, edge_bam):
    from remora_amd.validate import parse_mod_bam

    path, _ = edge_bam
    whole = _gpu_join(path, ALPHABET, _truth(), 512)
    for batch in (1, 3):
        _same(_gpu_join(path, ALPHABET, _truth(), batch), whole)
    for batch in (1, 3, 512):
        got = parse_mod_bam(path, _truth(), None, ALPHABET, None, batch=batch, return_sites=True)
        _same(got, whole[:5])


@pytest.mark.parametrize("tag,alphabet", [("two", ["C", "m"]), ("three", ["C", "h", "m"])])
def test_parse_mod_bam_equals_the_reference_on_the_fixtures(torch_cuda, fx, tag, alphabet):
    from remora_amd.io import parse_mods_bed
    from remora_amd.validate import parse_mod_bam

    cat_p, cat_l = [], []
    for (bam, bed), prefix in zip(PAIRS, ("can", "mod")):
        probs, labels, qpos, rpos, counts = parse_mod_bam(bam, parse_mods_bed(bed)[0], None, alphabet, None, return_sites=True)
        assert probs.dtype == np.float64 and labels.dtype == np.int64
        assert np.array_equal(counts, fx[f"{tag}__{prefix}__counts"])  # per read
        assert np.array_equal(probs, fx[f"{tag}__{prefix}__probs"]) and np.array_equal(labels, fx[f"{tag}__{prefix}__labels"])
        assert np.array_equal(qpos, fx[f"{prefix}__qpos"]) and np.array_equal(rpos, fx[f"{prefix}__rpos"])
        cat_p.append(probs)
        cat_l.append(labels)
    assert np.array_equal(np.vstack(cat_p), fx[f"{tag}__probs"]) and np.array_equal(np.concatenate(cat_l), fx[f"{tag}__labels"])


@pytest.mark.parametrize("key,kw", [
    ("two__line_balanced", dict(name="two_balanced")),
    ("two__line_unbalanced", dict(name="two_unbalanced", allow_unbalanced=True)),
    ("three__line_balanced", dict(name="three_balanced", extra_bases="h")),
    ("three__line_unbalanced", dict(name="three_unbalanced", extra_bases="h", allow_unbalanced=True)),
    ("max5__line", dict(name="max5", max_sites_per_read=5)),
])
def test_validate_modbams_gives_the_reference_lines(torch_cuda, fx, key, kw):
    from remora_amd.validate import validate_modbams

    assert validate_modbams(PAIRS, None, pct_filt=10.0, seed=int(fx["seed"]), **kw) == str(fx[key])


def test_no_valid_calls_is_the_reference_error(torch_cuda, tmp_path):
    from remora_amd import RemoraError
    from remora_amd.validate import parse_mod_bam

    path = str(tmp_path / "none.bam")
    mr.write_bam(path, REFS, [_rec("C" * 30, [("M", 30)], "C+m?,0;", [1], ref=2)])
    with pytest.raises(RemoraError, match="No valid modification calls from"):
        parse_mod_bam(path, _truth(), None, ALPHABET, None)


def test_command_line_prints_the_reference_line(torch_cuda, fx):
    argv = [sys.executable, "-m", "remora_amd", "validate", "from_modbams", "--seed", str(int(fx["seed"])), "--name", "two_balanced",
            "--explicit-mod-tag-used"]
    for bam, bed in PAIRS:
        argv += ["--bam-and-bed", bam, bed]
    p = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert p.stdout == str(fx["two__line_balanced"]).lstrip("\n")
