"""CPU-only checks of `validate from_modbams`: the MM / ML tokeniser (rmr_mod_tags_sizes / rmr_mod_tags_fill), parse_mods_bed,
process_mods_probs against the reference's lines (tests/golden/modbams.npz, tools/gen_golden.py --only modbams) and the command
line's arguments.  Every comparison is exact."""
import os
import struct

import numpy as np
import pytest

import modbam_restate as mr
from conftest import GOLDEN, golden

DATA = os.path.join(GOLDEN, "data")


def _tokenise(tag_regions, threads=1):
    """Records that are 32 zero bytes of fixed fields followed by the given tag bytes."""
    from remora_amd.validate import tokenise_mod_tags

    raws = [b"\x00" * 32 + t for t in tag_regions]
    raw_off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    return tokenise_mod_tags(b"".join(raws), raw_off, np.full(len(raws), 32, np.int64), threads=threads)


def _entries(tok, r):
    status, ent_off, _, _, entries, deltas, ml = tok
    out = []
    for e in entries[ent_off[r] : ent_off[r + 1]]:
        n, c = int(e["n_deltas"]), int(e["n_codes"])
        codes = [int(e["chebi"])] if e["chebi"] else list(e["codes"].decode())
        rows = ml[e["ml_off"] : e["ml_off"] + n * c].reshape(n, c).tolist()
        out.append((e["base"].decode(), e["strand"].decode(), codes, e["flag"].decode(), deltas[e["delta_off"] : e["delta_off"] + n].tolist(), rows))
    return out


CASES = [
    ("C+m?;", []),
    ("C+hm?,1,0,3;", [10, 11, 20, 21, 30, 31]),
    ("C+h?,1,0;C+m?,2,5,0;", [1, 2, 3, 4, 5]),
    ("A+a,0,1;C+76792,4;C+m?,0,0;", [200, 201, 99, 7, 8]),
    ("G-m,3,1;C+m.,0;", [50, 51, 52]),
    ("C+m.,1;C+h?,2;C+a,3;", [1, 2, 3]),
    ("N+m?,0,10;T-e,1;", [250, 251, 252]),
]


def test_tokeniser_matches_the_grammar_case_by_case():
    tok = _tokenise([mr.mod_tags(mm, ml) for mm, ml in CASES])
    assert tok[0].tolist() == [0] * len(CASES)
    for r, (mm, ml) in enumerate(CASES):
        assert _entries(tok, r) == mr.parse_mm_ml(mm, ml), mm
    # the kept entry's ML range lies behind the bytes of the entries in front of it
    a = _entries(tok, 3)
    assert a[2] == ("C", "+", ["m"], "?", [0, 0], [[7], [8]]) and a[1][2] == [76792] and a[1][5] == [[99]]
    assert _entries(tok, 4)[1] == ("C", "+", ["m"], ".", [0], [[52]])
    assert [e[3] for e in _entries(tok, 5)] == [".", "?", ""]
    assert _entries(tok, 0) == [("C", "+", ["m"], "?", [], [])]
    assert _entries(tok, 1)[0][5] == [[10, 11], [20, 21], [30, 31]]  # call-major: per call the codes in listed order


def test_tokeniser_spellings_and_neighbouring_tags():
    other = b"NMC\x05" + b"mvBc" + struct.pack("<i", 3) + b"\x05\x01\x00" + b"MDZ10\x00"
    regions = [other + mr.mod_tags("C+m?,1;", [9], lower=True) + b"tsi" + struct.pack("<i", 7),
               b"MLBC" + struct.pack("<i", 1) + b"\x09" + other + b"MMZC+m?,1;\x00",  # ML in front of MM
               other, b""]
    tok = _tokenise(regions)
    assert tok[0].tolist() == [0, 0, 1, 1]
    assert _entries(tok, 0) == _entries(tok, 1) == [("C", "+", ["m"], "?", [1], [[9]])]
    assert tok[1].tolist() == [0, 1, 2, 2, 2] and tok[2].tolist() == [0, 1, 2, 2, 2] and tok[3].tolist() == [0, 1, 2, 2, 2]


@pytest.mark.parametrize("mm,ml", [
    ("C+m?,0,1;", [1]),            # ML too short
    ("C+m?,0,1;", [1, 2, 3]),      # ML too long
    ("C+m?,0;", None),             # MM with deltas, no ML
    ("C+hm?,0;", [1]),             # two codes need two bytes per call
    ("C+m?,0", [1]),               # no terminating ;
    ("X+m?,0;", [1]), ("C*m?,0;", [1]), ("C+M?,0;", [1]), ("C+m?,;", []), ("C+m?,-1;", [1]), ("C+m?0;", []),
    ("C+m?,99999999999;", [1]), ("C+m1?,0;", [1]),
])
def test_tokeniser_malformed(mm, ml):
    good = mr.mod_tags("C+m?,0;", [77])
    tok = _tokenise([good, mr.mod_tags(mm, ml), good])
    assert tok[0].tolist() == [0, 2, 0]
    assert tok[1].tolist() == [0, 1, 1, 2]  # the malformed record owns nothing, its neighbours are whole
    assert _entries(tok, 0) == _entries(tok, 2) == [("C", "+", ["m"], "?", [0], [[77]])]


def test_tokeniser_other_malformed_forms_and_mm_without_deltas_needs_no_ml():
    tok = _tokenise([b"MMZC+m?;\x00", b"MMZ\x00", b"MMAx", b"MMZC+m?,0;\x00MLBc" + struct.pack("<i", 1) + b"\x01", b"MMZC+m?,0;", b"XX"])
    assert tok[0].tolist() == [0, 0, 2, 2, 2, 2]
    assert _entries(tok, 0) == [("C", "+", ["m"], "?", [], [])] and _entries(tok, 1) == []


def test_tokeniser_empty_batch_and_threads_agree():
    tok = _tokenise([])
    assert tok[0].size == 0 and tok[1].tolist() == [0] and tok[4].size == 0 and tok[5].size == 0 and tok[6].size == 0
    regions = [mr.mod_tags(mm, ml) for mm, ml in CASES] * 40 + [b"", b"MMZbad\x00"]
    one, many = _tokenise(regions, threads=1), _tokenise(regions, threads=8)
    for a, b in zip(one, many):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_tokeniser_fill_refuses_offsets_that_are_not_the_counts():
    import ctypes

    from remora_amd import RemoraError, _lib as L

    raw = np.frombuffer(b"\x00" * 32 + mr.mod_tags("C+m?,0,1;", [1, 2]), np.uint8)
    raw_off, tags_off, status = np.array([0, raw.size], np.int64), np.array([32], np.int64), np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ent = np.zeros(4, np.dtype(L.MOD_ENTRY_FIELDS))
    deltas, ml = np.full(8, -7, np.int32), np.full(8, 255, np.uint8)
    wrong = np.array([0, 1], np.int64)
    with pytest.raises(RemoraError):  # one delta where the record has two
        L.check(L.lib().rmr_mod_tags_fill(1, p(raw), p(raw_off), p(tags_off), p(status), p(wrong), p(wrong), p(wrong), p(ent), p(deltas), p(ml), 1))
    assert (deltas == -7).all() and (ml == 255).all()


def test_tokeniser_reads_the_fixture_bams():
    """The tagged fixtures: every record tokenises, carries MD (`has` bit 7) and the expected entries."""
    from remora_amd.io import iter_bam_raw_batches
    from remora_amd.validate import tokenise_mod_tags

    for prefix, want in (("can", ["m"]), ("mod", ["h", "m"])):
        n = 0
        for rb, _ in iter_bam_raw_batches(os.path.join(DATA, f"{prefix}_modbam.bam"), batch=5):
            tok = tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off)
            assert (tok[0] == 0).all() and (rb.has & 0x80).all()
            for r in range(rb.n):
                ents = _entries(tok, r)
                assert [(e[0], e[1], e[2], e[3]) for e in ents] == [("C", "+", [m], "?") for m in want]
                assert len({tuple(e[4]) for e in ents}) == 1  # the same CG sites for every modified base
            n += rb.n
        assert n == 14


def test_parse_mods_bed(tmp_path):
    from remora_amd.io import parse_mods_bed

    for name, mod in (("can_gt.bed", "C"), ("mod_gt.bed", "m")):
        sites, mods = parse_mods_bed(os.path.join(DATA, name))
        assert mods == {mod}
        want = {}
        for line in open(os.path.join(DATA, name)):
            f = line.split()
            for pos in range(int(f[1]), int(f[2])):
                want.setdefault((f[0], f[5]), {})[pos] = f[3]
        assert dict(sites) == want and sum(len(v) for v in want.values()) == 330
    bed = tmp_path / "both.bed"
    bed.write_text("chr1\t10\t12\tm\nchr1\t20\t21\th\t.\t-\nchr2\t5\t6\tC\t0\t.\n")
    sites, mods = parse_mods_bed(str(bed))
    assert mods == {"m", "h", "C"}
    assert dict(sites) == {("chr1", "+"): {10: "m", 11: "m"}, ("chr1", "-"): {10: "m", 11: "m", 20: "h"},
                           ("chr2", "+"): {5: "C"}, ("chr2", "-"): {5: "C"}}


@pytest.mark.parametrize("tag,bal", [("two", "balanced"), ("two", "unbalanced"), ("three", "balanced"), ("three", "unbalanced")])
def test_process_mods_probs_reproduces_the_reference_lines(tag, bal):
    from remora_amd.validate import process_mods_probs

    g = golden("modbams.npz")
    np.random.seed(int(g["seed"]))
    line = process_mods_probs(g[f"{tag}__probs"].copy(), g[f"{tag}__labels"].copy(), bal == "unbalanced", 10.0, f"{tag}_{bal}")
    assert line == str(g[f"{tag}__line_{bal}"])


def test_process_mods_probs_one_label_needs_allow_unbalanced():
    from remora_amd import RemoraError
    from remora_amd.validate import process_mods_probs

    with pytest.raises(RemoraError, match="Cannot balance dataset with 1 label"):
        process_mods_probs(np.ones((4, 1)), np.zeros(4, np.int64), False, 10.0, "x")


def test_validate_modbams_alphabet_errors(tmp_path):
    from remora_amd import RemoraError
    from remora_amd.validate import FULL_RESULTS_REFUSAL, validate_modbams

    two, none = tmp_path / "two.bed", tmp_path / "none.bed"
    two.write_text("chr1\t1\t2\tC\t.\t+\nchr1\t3\t4\tA\t.\t+\n")
    none.write_text("chr1\t1\t2\tm\t.\t+\n")
    with pytest.raises(RemoraError, match="More than one canonical base found"):
        validate_modbams([("x.bam", str(two))], None, "s", 10.0)
    with pytest.raises(RemoraError, match="No canonical bases found in ground truth."):
        validate_modbams([("x.bam", str(none))], None, "s", 10.0)
    with pytest.raises(RemoraError) as e:
        validate_modbams([("x.bam", str(none))], str(tmp_path / "full.tsv"), "s", 10.0)
    assert str(e.value) == FULL_RESULTS_REFUSAL


def test_command_line_takes_the_reference_arguments_and_refuses_the_full_table(capsys):
    from remora_amd.__main__ import build_parser, main
    from remora_amd.validate import FULL_RESULTS_REFUSAL

    argv = ["validate", "from_modbams", "--bam-and-bed", "a.bam", "a.bed", "--bam-and-bed", "b.bam", "b.bed", "--name", "n", "--pct-filt",
            "5", "--allow-unbalanced", "--max-sites-per-read", "5", "--seed", "3", "--extra-bases", "mh", "--log-filename", "l.txt",
            "--explicit-mod-tag-used", "--full-results-filename", "f.tsv", "--device", "0"]
    a = build_parser().parse_args(argv)
    assert a.bam_and_bed == [["a.bam", "a.bed"], ["b.bam", "b.bed"]] and (a.name, a.pct_filt, a.allow_unbalanced) == ("n", 5.0, True)
    assert (a.max_sites_per_read, a.seed, a.extra_bases, a.log_filename, a.explicit_mod_tag_used) == (5, 3, "mh", "l.txt", True)
    assert a.full_results_filename == "f.tsv" and a.device == 0
    d = build_parser().parse_args(["validate", "from_modbams", "--bam-and-bed", "a", "b"])
    assert (d.name, d.pct_filt, d.allow_unbalanced, d.max_sites_per_read, d.seed, d.extra_bases) == ("sample", 10.0, False, None, None, None)
    assert main(argv) == 1
    assert FULL_RESULTS_REFUSAL in capsys.readouterr().err
    # without --explicit-mod-tag-used the command stops with the warning about implicit tags
    assert main(["validate", "from_modbams", "--bam-and-bed", "a.bam", "a.bed"]) == 1
    assert "--explicit-mod-tag-used" in capsys.readouterr().err
    help_text = build_parser()._subparsers._group_actions[0].choices["validate"]._subparsers._group_actions[0].choices["from_modbams"].format_help()
    assert "np.random.seed" in help_text
