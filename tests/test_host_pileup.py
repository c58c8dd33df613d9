"""`analyze pileup_modbams`, the host side: the command line's arguments, the two threshold rules in exact arithmetic, the
bedMethyl and counts writers on a hand-made table, and the new symbols of the C ABI.  No GPU."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("rmr_pileup_emit_counts", "rmr_pileup_emit_fill", "rmr_pileup_create", "rmr_pileup_add", "rmr_pileup_finish", "rmr_pileup_read",
               "rmr_pileup_destroy")


def test_parser_takes_the_arguments():
    from remora_amd.__main__ import _pileup_modbams, build_parser

    ap = build_parser()
    a = ap.parse_args(["analyze", "pileup_modbams", "--bam", "a.bam", "--bam", "b.bam", "--out-bed", "s.bed", "--canonical-base", "C",
                       "--mod-bases", "m", "h", "--filter-threshold", "0.75", "--min-coverage", "3", "--counts-filename", "c.tsv", "--region",
                       "chr1:10-20", "--pileup-device-gib", "0.25", "--reads-per-batch", "7", "--device", "1", "--log-filename", "l.txt"])
    assert a.func is _pileup_modbams and a.bam == ["a.bam", "b.bam"] and a.out_bed == "s.bed" and a.canonical_base == "C"
    assert a.mod_bases == ["m", "h"] and a.filter_threshold == 0.75 and a.pct_filt is None and a.min_coverage == 3
    assert a.counts_filename == "c.tsv" and a.region == "chr1:10-20" and a.pileup_device_gib == 0.25 and a.reads_per_batch == 7
    assert a.device == 1 and a.log_filename == "l.txt"
    d = ap.parse_args(["analyze", "pileup_modbams", "--bam", "a.bam", "--out-bed", "s.bed", "--canonical-base", "C", "--mod-bases", "m"])
    assert d.filter_threshold is None and d.pct_filt is None and d.min_coverage == 1 and d.counts_filename is None and d.region is None
    assert d.pileup_device_gib == 8.0 and d.reads_per_batch == 512 and d.device == 0 and d.log_filename is None
    p = ap.parse_args(["analyze", "pileup_modbams", "--bam", "a.bam", "--out-bed", "s.bed", "--canonical-base", "C", "--mod-bases", "m",
                       "--pct-filt", "25"])
    assert p.pct_filt == 25.0
    for missing in ("--bam", "--out-bed", "--canonical-base", "--mod-bases"):
        argv = ["analyze", "pileup_modbams", "--bam", "a.bam", "--out-bed", "s.bed", "--canonical-base", "C", "--mod-bases", "m"]
        at = argv.index(missing)
        with pytest.raises(SystemExit):
            ap.parse_args(argv[:at] + argv[at + 2 :])


def test_threshold_is_the_exact_ceiling_of_512_t():
    from remora_amd import RemoraError
    from remora_amd.pileup import threshold_k

    assert threshold_k(0) == 0 and threshold_k(0.0) == 0
    assert threshold_k(Fraction(1, 512)) == 1 and threshold_k(1 / 512) == 1
    assert threshold_k(0.5) == 256 and threshold_k(1) == 512 and threshold_k(1.0) == 512
    # just above a grid point: the next one up, however small the excess
    assert threshold_k(Fraction(256, 512) + Fraction(1, 10**30)) == 257
    assert threshold_k(np.nextafter(0.5, 1.0).item()) == 257 and threshold_k(np.nextafter(0.5, 0.0).item()) == 256
    assert threshold_k(Fraction(511, 512) + Fraction(1, 10**9)) == 512
    assert threshold_k(0.1) == 52  # 51.2: the decimal the user wrote, not the binary double below or above it
    for bad in (-0.001, 1.001, Fraction(513, 512)):
        with pytest.raises(RemoraError, match="0 to 1"):
            threshold_k(bad)


def _restated_percentile(hist, pct):
    n = sum(hist)
    allowed = (Fraction(n) * Fraction(str(pct)) / 100).__floor__()
    best = 0
    for k in range(0, 514):
        if sum(hist[:k]) <= allowed:
            best = k
    return best


def test_percentile_rule_on_hand_made_histograms():
    from remora_amd import RemoraError
    from remora_amd.pileup import N_BINS, percentile_k

    assert N_BINS == 513
    h = [0] * 513
    h[300] = 100  # one value: a tie filters nothing, whatever the percentage below 100
    for pct in (0, 10, 50, 99.9):
        assert percentile_k(h, pct) == 300
    assert percentile_k(h, 100) == 513  # every call may go: the threshold lies above every kmax
    h = [0] * 513
    h[100], h[200], h[300], h[512] = 10, 10, 30, 50  # N = 100
    assert percentile_k(h, 0) == 100     # nothing may fail: up to the smallest kmax present
    assert percentile_k(h, 9.99) == 100  # floor(9.99) = 9 < 10
    assert percentile_k(h, 10) == 200    # exactly the ten calls at 100 fail
    assert percentile_k(h, 19) == 200 and percentile_k(h, 20) == 300 and percentile_k(h, 49.5) == 300 and percentile_k(h, 50) == 512
    assert percentile_k(h, 99) == 512 and percentile_k(h, 100) == 513
    h = [1] * 513  # every bin once
    for pct in (0, 10, 50, 100):
        assert percentile_k(h, pct) == (513 * Fraction(str(pct)) / 100).__floor__()
    rng = np.random.default_rng(3)
    for _ in range(20):
        h = (rng.integers(0, 50, 513) * (rng.random(513) < 0.2)).tolist()
        for pct in (0, 0.1, 10, 33.3, 50, 100):
            assert percentile_k(h, pct) == _restated_percentile(h, pct), (pct,)
    assert percentile_k([0] * 513, 10) == 513  # (no call: pileup_modbams refuses before it asks)
    for bad in (-1, 100.5):
        with pytest.raises(RemoraError, match="0 to 100"):
            percentile_k([0] * 513, bad)
    with pytest.raises(RemoraError, match="513 bins"):
        percentile_k([0] * 512, 10)


def _table():
    from remora_amd.pileup import PileupTable

    #            C   h   m  fail
    counts = [[3, 0, 1, 2],      # chrA 5 +
              [0, 0, 0, 4],      # chrA 5 -   nothing passes: no bedMethyl row at any coverage
              [1, 1, 1, 0],      # chrA 9 +
              [0, 2000, 1000, 7],  # chrB 0 -   the score column is capped at 1000
              [2, 0, 0, 0]]      # chrB 2147483647 +
    return PileupTable(ref_names=["chrA", "chrB"], ref_id=np.array([0, 0, 0, 1, 1], np.int32), pos=np.array([5, 5, 9, 0, 2**31 - 1], np.int64),
                       strand=np.array([0, 1, 0, 1, 0], np.uint8), counts=np.array(counts, np.int64), alphabet=["C", "h", "m"], threshold_k=300,
                       n_calls=3024, n_flushes=1, peak_device_bytes=0, hist=None)


def test_writers_on_a_hand_made_table(tmp_path):
    from remora_amd.pileup import write_bedmethyl, write_counts

    t = _table()
    bed, tsv = tmp_path / "s.bed", tmp_path / "c.tsv"
    assert write_bedmethyl(t, bed) == 8
    assert bed.read_text() == ("chrA\t5\t6\th\t4\t+\t5\t6\t255,0,0\t4\t0.00\n"
                               "chrA\t5\t6\tm\t4\t+\t5\t6\t255,0,0\t4\t25.00\n"
                               "chrA\t9\t10\th\t3\t+\t9\t10\t255,0,0\t3\t33.33\n"
                               "chrA\t9\t10\tm\t3\t+\t9\t10\t255,0,0\t3\t33.33\n"
                               "chrB\t0\t1\th\t1000\t-\t0\t1\t255,0,0\t3000\t66.67\n"
                               "chrB\t0\t1\tm\t1000\t-\t0\t1\t255,0,0\t3000\t33.33\n"
                               "chrB\t2147483647\t2147483648\th\t2\t+\t2147483647\t2147483648\t255,0,0\t2\t0.00\n"
                               "chrB\t2147483647\t2147483648\tm\t2\t+\t2147483647\t2147483648\t255,0,0\t2\t0.00\n")
    assert write_bedmethyl(t, bed, min_coverage=4) == 4
    assert [ln.split("\t")[1] for ln in bed.read_text().splitlines()] == ["5", "5", "0", "0"]
    assert write_bedmethyl(t, bed, min_coverage=3001) == 0 and bed.read_text() == ""
    assert write_counts(t, tsv) == 5
    assert tsv.read_text() == ("chrom\tstart\tstrand\tN_C\tN_h\tN_m\tN_fail\n"
                               "chrA\t5\t+\t3\t0\t1\t2\n"
                               "chrA\t5\t-\t0\t0\t0\t4\n"
                               "chrA\t9\t+\t1\t1\t1\t0\n"
                               "chrB\t0\t-\t0\t2000\t1000\t7\n"
                               "chrB\t2147483647\t+\t2\t0\t0\t0\n")


def test_region_and_dictionary_checks():
    from remora_amd import RemoraError
    from remora_amd.pileup import check_reference_dicts, check_site_fields, parse_region

    names, lens = ["chrA", "HLA:B", "chrC"], [1000, 500, 7]
    assert parse_region(None, names, lens) == (-1, 0, 0)
    assert parse_region("chrA", names, lens) == (0, 0, 1000) and parse_region("HLA:B", names, lens) == (1, 0, 500)
    assert parse_region("chrA:10-20", names, lens) == (0, 10, 20) and parse_region("HLA:B:1,000-2,000", names, lens) == (1, 1000, 2000)
    for bad, msg in (("chrZ", "does not have"), ("chrZ:1-2", "does not have"), ("chrA:5", "ctg:start-end"), ("chrA:9-3", "start <= end")):
        with pytest.raises(RemoraError, match=msg):
            parse_region(bad, names, lens)
    a = [("chrA", 10), ("chrB", 20)]
    check_reference_dicts(["x.bam", "y.bam"], [a, list(a)])
    with pytest.raises(RemoraError, match=r"contig #1: chrB \(20 bases\) against chrB \(21 bases\)"):
        check_reference_dicts(["x.bam", "y.bam"], [a, [("chrA", 10), ("chrB", 21)]])
    with pytest.raises(RemoraError, match="2 against 3 contigs"):
        check_reference_dicts(["x.bam", "y.bam"], [a, a + [("chrC", 1)]])
    check_site_fields(1 << 24, 1 << 31)
    with pytest.raises(RemoraError, match="24 bits"):
        check_site_fields((1 << 24) + 1, 10)
    with pytest.raises(RemoraError, match="31 bits"):
        check_site_fields(3, (1 << 31) + 1)


def test_new_symbols_are_declared_exported_and_bound():
    from remora_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "remora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
        # every new entry point says what it does: its name stands in a comment of the header
        assert any(name in c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S)), name
    assert "k_pileup.hip" in open(os.path.join(ROOT, "remora_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define RMR_PILEUP_BINS 513\b", hdr)
