"""CPU-only tests of duplex calling: the restatement of the alignment (tests/duplex_restate.py) on the reference's seven known
answers, trimming and mapping from a CIGAR, the pair bookkeeping of infer_duplex, the command line, and the new entry of the
C ABI."""
import json
import os
import re

import numpy as np
import pytest

import duplex_restate as R
from conftest import GOLDEN, ROOT

CASES = json.load(open(os.path.join(GOLDEN, "duplex_known_answers.json")))


@pytest.mark.parametrize("case", range(7))
def test_restatement_gives_the_known_answers(case):
    from remora_amd import data_chunks as DC

    c = CASES[case]
    res = R.align(c["simplex"], c["duplex"])
    assert res["status"] == R.ST_OK
    assert c["duplex"][res["ref_start"]:res["ref_end"]] == c["trimmed_duplex_seq"] and res["ref_start"] == c["duplex_offset"]
    mapping = R.mapping(res)
    assert mapping.tolist() == c["duplex_to_simplex_mapping"] and mapping.size == res["ref_end"] - res["ref_start"] + 1
    sig = DC.map_ref_to_signal(query_to_signal=np.arange(len(c["simplex"])), ref_to_query_knots=mapping)
    assert sig.tolist() == c["duplex_to_signal"]
    score, q_end = R.path_score(c["simplex"], c["duplex"], res)
    assert score == res["score"] and q_end == res["end_row"]


def test_restatement_statuses_and_ties():
    assert R.align("", "ACGT")["status"] == R.ST_EMPTY and R.align("ACGT", "")["status"] == R.ST_EMPTY
    assert R.align("ACGU", "ACGT")["status"] == R.ST_BAD_BASE
    assert R.align("A", "CCCCCCCC")["status"] == R.ST_NO_MATCH  # H[0][m] == H[1][m]: the smaller end row wins, all deletions
    # a deletion inside a homopolymer: the walk back prefers the diagonal, so the gap sits at the homopolymer's start
    res = R.align("CCAAAAGG", "CCAAAAAAGG")
    assert res["ops"].tolist() == [0, 2, 0] and res["lens"].tolist() == [2, 2, 6]
    # N scores: -2 against a base, -1 against N
    assert R.align("ACGTNACGT", "ACGTNACGT")["score"] == 8 * 5 - 1 and R.align("ACGTNACGT", "ACGTCACGT")["score"] == 8 * 5 - 2
    # a gap of k bases costs 10 + 2 (k - 1)
    assert R.align("ACGTACGTTTGCA", "ACGTACGCCCTTTGCA")["score"] == 13 * 5 - (10 + 2 * 2)


def test_cpp_twin_equals_the_numpy_restatement(tmp_path):
    rng = np.random.default_rng(11)
    rand = lambda n: "".join(rng.choice(list("ACGTN"), n, p=[0.24, 0.24, 0.24, 0.24, 0.04]))  # noqa: E731
    pairs = [(c["simplex"], c["duplex"]) for c in CASES] + [("A" * 40, "A" * 33), ("A" * 3, "A" * 70), ("ACGU", "ACGT"), ("", "A"),
                                                           ("A", "CCCCCCCC")]
    for n, m in ((1, 1), (1, 90), (90, 1), (200, 180), (64, 300), (300, 64)):
        d = rand(m)
        pairs += [(rand(n), d), ((d[m // 3:] + rand(n))[:n], d)]
    for got, (q, r) in zip(R.align_cpp(pairs, R.build_cpp(tmp_path)), pairs):
        want = R.align(q, r)
        assert all(np.asarray(got[k]).tolist() == np.asarray(want[k]).tolist() for k in want), (q, r)


def test_trimming_and_mapping_from_a_cigar():
    """duplex_utils.mapping_from_alignment on the alignments the known answers imply (written by hand as trimmed CIGARs)."""
    from remora_amd import duplex_utils as DU

    for c in CASES:
        res = R.align(c["simplex"], c["duplex"])
        pa = DU.PairwiseAlignment(ref_start=res["ref_start"], ref_end=res["ref_end"], query_start=res["query_start"],
                                  query_end=res["end_row"], cigar=list(zip(res["ops"].tolist(), res["lens"].tolist())))
        got = DU.mapping_from_alignment(pa, c["duplex"])
        assert got.trimmed_duplex_seq == c["trimmed_duplex_seq"] and got.duplex_offset == c["duplex_offset"]
        assert got.duplex_to_simplex_mapping.tolist() == c["duplex_to_simplex_mapping"]
    # gaps inside: float64 interpolation across them, truncated; the array form of the CIGAR gives the same
    pa = DU.PairwiseAlignment(ref_start=3, ref_end=3 + 4 + 3 + 2, query_start=2, query_end=0, cigar=[(0, 4), (2, 3), (0, 1), (1, 5), (0, 1)])
    want = (np.interp(np.arange(10), [0, 0, 3, 7, 7, 8, 8, 9], [0, 0, 3, 4, 4, 10, 10, 11]).astype(int) + 2).tolist()
    assert DU.mapping_from_alignment(pa, "T" * 20).duplex_to_simplex_mapping.tolist() == want
    pa.cigar = (np.array([0, 2, 0, 1, 0]), np.array([4, 3, 1, 5, 1]))
    got = DU.mapping_from_alignment(pa, "T" * 20)
    assert got.duplex_to_simplex_mapping.tolist() == want and got.trimmed_duplex_seq == "T" * 9 and got.duplex_offset == 3


class _Index:
    def __init__(self, ids):
        self.read_ids = list(ids)


def test_check_simplex_alignments():
    from remora_amd.inference import check_simplex_alignments

    simplex, duplex = _Index(["t1", "c1", "t2", "c2", "t3"]), _Index(["t1", "t3", "t4"])
    pairs = [("t1", "c1"), ("t2", "c2"), ("t3", "c3"), ("t4", "c4")]
    # valid: both ids in the simplex BAM and the template id in the duplex BAM
    assert check_simplex_alignments(simplex_index=simplex, duplex_index=duplex, pairs=pairs) == ([("t1", "c1")], 1)
    assert check_simplex_alignments(simplex_index=simplex, duplex_index=_Index([]), pairs=pairs) == ([], 0)
    with pytest.raises(ValueError, match="no pairs found in file"):
        check_simplex_alignments(simplex_index=simplex, duplex_index=duplex, pairs=[])
    with pytest.raises(ValueError, match="zero simplex alignments found"):
        check_simplex_alignments(simplex_index=_Index(["x"]), duplex_index=duplex, pairs=pairs)


def test_cli_parses_the_reference_command_line():
    from remora_amd.__main__ import _infer_duplex, build_parser

    args = build_parser().parse_args(
        "infer duplex_from_pod5_and_bam reads.pod5 simplex.bam duplex.bam pairs.txt --model m.pt --out-bam out.bam --duplex-delim : "
        "--num-reads 5 --device 0 --log-filename log.txt --num-extract-alignment-workers 3 --num-duplex-prep-workers 4 "
        "--num-infer-workers 5".split())
    assert args.func is _infer_duplex
    assert (args.pod5, args.simplex_bam, args.duplex_bam, args.duplex_read_pairs) == ("reads.pod5", "simplex.bam", "duplex.bam", "pairs.txt")
    assert (args.model, args.out_bam, args.duplex_delim, args.num_reads, args.device, args.log_filename) == (
        ["m.pt"], "out.bam", ":", 5, 0, "log.txt")
    assert (args.num_extract_alignment_workers, args.num_duplex_prep_workers, args.num_infer_workers) == (3, 4, 5)
    dflt = build_parser().parse_args("infer duplex_from_pod5_and_bam a b c d --model m.pt --out-bam o.bam".split())
    assert (dflt.duplex_delim, dflt.num_reads, dflt.dtype, dflt.bam_level, dflt.reads_per_batch) == (";", None, None, None, 64)


def test_more_than_one_model_raises(tmp_path):
    from remora_amd.__main__ import main

    with pytest.raises(NotImplementedError, match="multiple models"):
        main(f"infer duplex_from_pod5_and_bam a b c d --model m1.pt --model m2.pt --out-bam {tmp_path}/o.bam".split())


def test_missing_input_is_named(tmp_path):
    from remora_amd.__main__ import main

    with pytest.raises(ValueError, match="didn't find pod5 at"):
        main(f"infer duplex_from_pod5_and_bam {tmp_path}/no.pod5 b c d --model m1.pt --out-bam {tmp_path}/o.bam".split())


def test_entry_is_declared_exported_and_bound():
    import ctypes

    from remora_amd import _lib
    from remora_amd import duplex_utils as DU

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "remora_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint rmr_duplex_align\s*\(([^;]*)\)\s*;", hdr)
    assert decl, "rmr_duplex_align is not declared in include/remora_hip.h"
    restype, argtypes = _lib.SIGNATURES["rmr_duplex_align"]
    assert restype is ctypes.c_int and len(argtypes) == len(decl.group(1).split(","))
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "rmr_duplex_align")
    # ONE constants block: the Python mirror and the restatement hold the header's values
    defs = dict(re.findall(r"#define (RMR_DUPLEX_\w+) \(?(-?\d+)\)?\s", hdr))
    want = {"MATCH": DU.MATCH, "MISMATCH": DU.MISMATCH, "N_BASE": DU.N_BASE, "N_N": DU.N_N, "GAP_OPEN": DU.GAP_OPEN,
            "GAP_EXTEND": DU.GAP_EXTEND, "ROWS_PER_LANE": DU.ROWS_PER_LANE, "STRIP_ROWS": DU.STRIP_ROWS, "OK": DU.STATUS_OK,
            "NO_MATCH": DU.STATUS_NO_MATCH, "BAD_BASE": DU.STATUS_BAD_BASE, "OVER_BUDGET": DU.STATUS_OVER_BUDGET,
            "EMPTY": DU.STATUS_EMPTY, "OUT_FIELDS": DU.OUT_FIELDS}
    for name, value in want.items():
        assert int(defs[f"RMR_DUPLEX_{name}"]) == value, name
    assert (R.MATCH, R.MISMATCH, R.N_BASE, R.N_N, R.OPEN, R.EXTEND) == (DU.MATCH, DU.MISMATCH, DU.N_BASE, DU.N_N, DU.GAP_OPEN, DU.GAP_EXTEND)
    assert "((int64_t)1 << 34)" in hdr and DU.DEFAULT_TRACE_BYTES == 1 << 34 and DU.trace_bytes(513, 1000) == 2 * 1063 * 256


def test_fixture_files_open_on_the_cpu(tmp_path):
    """The two BAMs through the native reader; the POD5 (committed in two parts, see tests/golden/README_duplex.md) joined and opened."""
    from duplex_fixture import duplex_pod5
    from remora_amd import io as rio

    pf = rio.Pod5File(duplex_pod5(tmp_path))
    pairs = [tuple(line.split()) for line in open(os.path.join(GOLDEN, "data", "duplex_pairs.txt"))]
    assert len(pairs) == 2 and all(rid in pf for p in pairs for rid in p)
    flags = [r.flag & 0x10 for r in rio.iter_bam_records(os.path.join(GOLDEN, "data", "duplex_reads_mapped.bam"))]
    assert sorted(flags) == [0, 16, 16, 16]
