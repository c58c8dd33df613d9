"""`analyze pileup_modbams --coverage-columns` on the host: the eighteen-column bedMethyl and the extended counts file from a
hand-made table, the refusal with --duplex / --hemi before anything is opened, the new entry points, and the restatement of
the coverage join (pileup_coverage_restate.py) asked alone whether the input of the GPU tests is vacuous."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pileup_coverage_restate as pc
import test_gpu_pileup as tp
from conftest import ROOT

ALPHABET = pc.ALPHABET
NEW_SYMBOLS = ("rmr_pileup_set_canonical", "rmr_pileup_cover", "rmr_pileup_read_cover")


def _table(coverage):
    from remora_amd.pileup import PileupTable

    return PileupTable(ref_names=["chrA", "chrB"], ref_id=np.array([0, 0, 1], np.int32), pos=np.array([5, 5, 2**31 - 1], np.int64),
                       strand=np.array([0, 1, 0], np.uint8), counts=np.array([[3, 1, 6, 2], [0, 0, 0, 4], [1200, 0, 300, 0]], np.int64),
                       alphabet=["C", "h", "m"], threshold_k=300, n_calls=1516, n_flushes=1, peak_device_bytes=0, hist=None,
                       coverage=None if coverage is None else np.array(coverage, np.int64))


def test_writers_on_a_hand_made_table(tmp_path):
    from remora_amd.pileup import PileupTable, write_bedmethyl, write_counts

    table = _table([[7, 8, 9], [1, 0, 2], [0, 30, 0]])
    assert PileupTable._fields[-1] == "combined" and table.coverage.dtype == np.int64 and table.coverage.shape == (3, 3)
    bed, tsv = tmp_path / "a.bed", tmp_path / "a.tsv"
    assert write_bedmethyl(table, bed) == 4 and write_counts(table, tsv) == 3
    end = "2147483647\t2147483648"
    # chrom start end code score strand start end colour N_valid pct | N_mod N_canonical N_other_mod N_delete N_fail N_diff N_nocall
    assert bed.read_text() == (
        "chrA\t5\t6\th\t10\t+\t5\t6\t255,0,0\t10\t10.00\t1\t3\t6\t7\t2\t8\t9\n"
        "chrA\t5\t6\tm\t10\t+\t5\t6\t255,0,0\t10\t60.00\t6\t3\t1\t7\t2\t8\t9\n"
        f"chrB\t{end}\th\t1000\t+\t{end}\t255,0,0\t1500\t0.00\t0\t1200\t300\t0\t0\t30\t0\n"
        f"chrB\t{end}\tm\t1000\t+\t{end}\t255,0,0\t1500\t20.00\t300\t1200\t0\t0\t0\t30\t0\n")
    assert all(len(line.split("\t")) == 18 for line in bed.read_text().splitlines())
    assert tsv.read_text() == ("chrom\tstart\tstrand\tN_C\tN_h\tN_m\tN_fail\tN_delete\tN_diff\tN_nocall\n"
                               "chrA\t5\t+\t3\t1\t6\t2\t7\t8\t9\n"
                               "chrA\t5\t-\t0\t0\t0\t4\t1\t0\t2\n"
                               "chrB\t2147483647\t+\t1200\t0\t300\t0\t0\t30\t0\n")
    assert write_bedmethyl(table, bed, min_coverage=11) == 2 and bed.read_text().startswith("chrB")  # row selection: N_valid alone
    # the same table without the coverage: today's eleven columns and today's counts file, byte for byte
    plain = _table(None)
    assert plain.coverage is None and write_bedmethyl(plain, bed) == 4 and write_counts(plain, tsv) == 3
    assert bed.read_text() == ("chrA\t5\t6\th\t10\t+\t5\t6\t255,0,0\t10\t10.00\n"
                               "chrA\t5\t6\tm\t10\t+\t5\t6\t255,0,0\t10\t60.00\n"
                               f"chrB\t{end}\th\t1000\t+\t{end}\t255,0,0\t1500\t0.00\n"
                               f"chrB\t{end}\tm\t1000\t+\t{end}\t255,0,0\t1500\t20.00\n")
    assert tsv.read_text() == ("chrom\tstart\tstrand\tN_C\tN_h\tN_m\tN_fail\nchrA\t5\t+\t3\t1\t6\t2\nchrA\t5\t-\t0\t0\t0\t4\n"
                               "chrB\t2147483647\t+\t1200\t0\t300\t0\n")
    # the restatement's text functions agree with the writers on this table
    want = {(0, 5, 0): [3, 1, 6, 2], (0, 5, 1): [0, 0, 0, 4], (1, 2**31 - 1, 0): [1200, 0, 300, 0]}
    cover = {(0, 5, 0): [7, 8, 9], (0, 5, 1): [1, 0, 2], (1, 2**31 - 1, 0): [0, 30, 0]}
    refs = [("chrA", 0), ("chrB", 0)]
    write_bedmethyl(table, bed), write_counts(table, tsv)
    assert bed.read_text() == pc.bed18_text(want, cover, ALPHABET, refs) and tsv.read_text() == pc.tsv_text(want, cover, ALPHABET, refs)


def test_partitioned_tables_carry_the_coverage(tmp_path):
    from remora_amd.pileup import PileupTable, partition_tables, write_partitioned

    base = _table([[7, 8, 9], [1, 0, 2], [0, 30, 0]])
    table = PileupTable(*base, partition=np.array([0, 1, 1], np.int32), partition_labels=["1", "ungrouped"], partition_tag="HP",
                        coverage=base.coverage)
    subs = partition_tables(table)
    assert subs["1"].coverage.tolist() == [[7, 8, 9]] and subs["ungrouped"].coverage.tolist() == [[1, 0, 2], [0, 30, 0]]
    write_partitioned(table, tmp_path / "p.bed", tmp_path / "p.tsv")
    assert (tmp_path / "p.HP_1.tsv").read_text() == ("chrom\tstart\tstrand\tN_C\tN_h\tN_m\tN_fail\tN_delete\tN_diff\tN_nocall\n"
                                                      "chrA\t5\t+\t3\t1\t6\t2\t7\t8\t9\n")
    assert (tmp_path / "p.ungrouped.bed").read_text().splitlines()[0].split("\t")[11:] == ["0", "1200", "300", "0", "0", "30", "0"]
    plain = PileupTable(*base, partition=np.array([0, 1, 1], np.int32), partition_labels=["1", "ungrouped"], partition_tag="HP")
    assert all(t.coverage is None for t in partition_tables(plain).values())


@pytest.mark.parametrize("other", ["duplex", "hemi"])
def test_refusal_with_duplex_or_hemi_comes_before_any_file(tmp_path, other):
    from remora_amd import RemoraError
    from remora_amd.pileup import pileup_modbams

    missing = str(tmp_path / "missing.bam")
    with pytest.raises(RemoraError) as e:
        pileup_modbams(missing, ALPHABET, coverage=True, **{other: True})
    assert "--coverage-columns" in str(e.value) and f"--{other}" in str(e.value)
    bed, tsv, log = tmp_path / "x.bed", tmp_path / "x.tsv", tmp_path / "x.log"
    run = subprocess.run([sys.executable, "-m", "remora_amd", "analyze", "pileup_modbams", "--bam", missing, "--canonical-base", "C", "--mod-bases",
                          "h", "m", "--out-bed", str(bed), "--counts-filename", str(tsv), "--log-filename", str(log), "--coverage-columns",
                          f"--{other}"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode != 0 and "--coverage-columns" in run.stderr and f"--{other}" in run.stderr, run.stderr
    assert not bed.exists() and not tsv.exists() and not log.exists()


def test_command_line_help_states_the_extra_pass():
    from remora_amd.__main__ import build_parser

    ap = build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["analyze", "pileup_modbams", "--bam", "x", "--out-bed", "y", "--canonical-base", "C", "--mod-bases", "m", "--no-such-flag"])
    args = ap.parse_args(["analyze", "pileup_modbams", "--bam", "x", "--out-bed", "y", "--canonical-base", "C", "--mod-bases", "m",
                          "--coverage-columns"])
    assert args.coverage_columns is True
    args = ap.parse_args(["analyze", "pileup_modbams", "--bam", "x", "--out-bed", "y", "--canonical-base", "C", "--mod-bases", "m"])
    assert args.coverage_columns is False


def test_new_symbols_are_declared_exported_and_bound():
    import ctypes

    from remora_amd import _lib

    header = open(os.path.join(ROOT, "include", "remora_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header) and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["rmr_pileup_cover"][1]) == 11 and len(_lib.SIGNATURES["rmr_pileup_read_cover"][1]) == 2
    assert "replaces: nothing in the reference" in header


# ---- the restatement alone: is the input of the GPU tests vacuous? ------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    recs, genome, expect = pc.coverage_input()
    table, k_t, _, statuses = tp.restate(recs, ALPHABET, k_t=410)
    return recs, genome, expect, table, pc.cover_restate(recs, ALPHABET, list(table)), statuses


def test_every_edge_record_does_what_its_case_says(restated):
    recs, _, expect, table, _, _ = restated
    sites = list(table)
    named = {r["case"]: r for r in recs if r.get("case")}
    assert set(named) == set(expect) and len(named) >= 25
    for case, (site, col) in expect.items():
        assert site in table, (case, site)
        got = pc.record_cover(named[case], ALPHABET, [s for s in sites if s[0] == site[0]])
        assert got.get(site) == col, (case, site, col, got.get(site))
    status = {case: tp.record_calls(named[case], ALPHABET)[0] for case in named}
    assert [status[f"status_{k}"] for k in (1, 2, 3, 5, 6)] == [1, 2, 3, 5, 6]
    assert all(st == 0 for case, st in status.items() if not case.startswith("status_"))
    assert tp.record_calls(named["no_call_kept"], ALPHABET) == (0, [])
    fail = tp.record_calls(named["failing_call"], ALPHABET)[1]
    assert [c[3:] for c in fail] == [(2, 257)] and table[expect["failing_call"][0]][-1] >= 1
    # the two records beside the span add nothing anywhere near it, the record inside a skip nothing inside the skip
    d = expect["inside_a_skip"][0][1]
    got = pc.record_cover(named["inside_a_skip"], ALPHABET, [s for s in sites if s[0] == 0])
    assert not any(d - 1 <= s[1] <= d + 1 and s[2] == 0 for s in got) and any(s[1] < d - 1 for s in got) and any(s[1] > d + 1 for s in got)
    both = expect["both_strands_at_one_position"][0][1]
    assert (0, both, 0) in table and (0, both, 1) in table and (1, both, 0) in table


def test_restated_coverage_is_not_vacuous(restated):
    recs, _, _, table, cover, statuses = restated
    assert set(cover) == set(table) and all(len(v) == 3 and min(v) >= 0 for v in cover.values())
    for col in range(3):  # every column on both strands and on both contigs
        for rid in (0, 1):
            for strand in (0, 1):
                assert sum(v[col] for k, v in cover.items() if k[0] == rid and k[2] == strand) > 0, (pc.COLS[col], rid, strand)
    assert any(min(v) > 0 for v in cover.values())  # a site with all three
    assert statuses.count(0) > 50 and all(statuses.count(st) >= 2 for st in (1, 2, 3, 5, 6))
    # a record of _synthetic() with a deletion and one with more operations than a workgroup has lanes take part
    assert any(("D", 5) in r["cigar"] for r in recs) and any(len(r["cigar"]) > 256 for r in recs)


def test_conservation_on_the_restatement(restated):
    """N_valid + N_fail + N_delete + N_diff + N_nocall = the status-0 records of that strand whose aligned pairs reach the
    position outside an N skip - from aligned_pairs alone."""
    import modbam_restate as mr

    recs, _, _, table, cover, statuses = restated
    reach = {}
    for rec, st in zip(recs, statuses):
        if st == 0:
            for _, r, marker in mr.aligned_pairs(rec["cigar"], rec["pos"]):
                if r is not None and marker is not None:
                    key = (rec["ref_id"], r, (rec["flag"] >> 4) & 1)
                    reach[key] = reach.get(key, 0) + 1
    for site, row in table.items():
        assert sum(row) + sum(cover[site]) == reach[site], site
