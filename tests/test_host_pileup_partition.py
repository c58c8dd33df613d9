"""`analyze pileup_modbams --partition-tag`, the host side: the native aux tag reader on records built by hand, the bit plan
of the partition field, label order and file names, the splitter and the writer on a hand-made partitioned table, the
command line's argument, and the stand-alone sanitizer program of the reader.  No GPU."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import modbam_restate as mr
from conftest import ROOT

ABSENT, INT, CHAR, OTHER, UNWALKABLE = range(5)
INT_EXTREMES = [("c", "<b", -128), ("c", "<b", 127), ("C", "<B", 255), ("s", "<h", -32768), ("S", "<H", 65535), ("i", "<i", -2**31), ("I", "<I", 2**32 - 1),
                ("C", "<B", 0), ("i", "<i", 2**31 - 1)]


def aux(tag, typ, fmt, value):
    return tag.encode() + typ.encode() + struct.pack(fmt, value)


def b_array(tag, sub, n):
    width = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[sub]
    return tag.encode() + b"B" + sub.encode() + struct.pack("<i", n) + bytes(range(1, n * width + 1))


def read_tag(regions, tag="HP", threads=1):
    """(value, kind) of rmr_bam_aux_values for records whose aux region is exactly regions[r]."""
    from remora_amd.pileup import read_aux_values

    bodies, tags_off = [], []
    for r, region in enumerate(regions):
        body = mr.bam_record(f"read{r}", 0, 0, 10, [("M", 5)], "ACGTA"[: 4 + r % 2], tags=region, has_md=False)[4:]
        bodies.append(body)
        tags_off.append(len(body) - len(region))
    raw_off = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int64)
    value, kind = read_aux_values(b"".join(bodies), raw_off, np.asarray(tags_off, np.int64), tag, threads=threads)
    return value.tolist(), kind.tolist()


def test_reader_takes_every_integer_type_at_its_extremes_and_a_character():
    regions = [aux("HP", t, f, v) for t, f, v in INT_EXTREMES] + [b"HPA" + bytes([c]) for c in (ord("a"), ord("1"), ord("-"), 255)]
    value, kind = read_tag(regions)
    assert value == [v for _, _, v in INT_EXTREMES] + [ord("a"), ord("1"), ord("-"), 255]
    assert kind == [INT] * len(INT_EXTREMES) + [CHAR] * 4


def test_reader_finds_the_tag_wherever_it_stands_and_skips_every_size():
    hp = aux("HP", "c", "<b", -3)
    others = [aux("NM", "C", "<B", 7), b"RGZgroup one\x00", aux("ts", "i", "<i", -5), aux("de", "f", "<f", 0.25)]
    regions = [b"", b"".join(others),                                   # no aux field at all; the tag absent among others
               hp + b"".join(others), others[0] + others[1] + hp + others[2] + others[3], b"".join(others) + hp,  # first, middle, last
               b"XXZ\x00" + hp, b"XXZHPc\x01\x00" + hp,                 # behind a Z: an empty one, one whose text holds the tag's bytes
               b"XXH1AE301\x00" + hp]                                   # behind an H
    regions += [b_array("XB", sub, n) + hp for sub in "cCsSiIf" for n in (0, 1, 3)]  # behind a B of every subtype
    regions += [aux("hp", "c", "<b", 1) + aux("Hp", "c", "<b", 2) + aux("HQ", "c", "<b", 4), aux("HP", "C", "<B", 9) + hp]  # other names; the first wins
    value, kind = read_tag(regions)
    want = [(0, ABSENT), (0, ABSENT), (-3, INT), (-3, INT), (-3, INT), (-3, INT), (-3, INT), (-3, INT)] + [(-3, INT)] * 21 + [(0, ABSENT), (9, INT)]
    assert list(zip(value, kind)) == want
    assert read_tag(regions, tag="XB")[1][8:29] == [OTHER] * 21 and set(read_tag(regions, tag="XB")[0][8:29]) == {ord("B")}
    for threads in (1, 3):  # the thread ranges of a batch larger than four per thread
        assert read_tag(regions * 3, threads=threads) == (value * 3, kind * 3)


def test_reader_names_the_type_it_does_not_take_and_the_region_it_cannot_walk():
    hp = aux("HP", "i", "<i", 2)
    regions = [b"HPZ1\x00", b"HPH0A\x00", b_array("HP", "C", 2), aux("HP", "f", "<f", 1.0),   # Z H B f: another type, its letter
               hp[:-1], hp[:4], hp[:3], hp[:2], b"HPs\x01",                                   # cut inside the value, inside the header
               b_array("XB", "s", 3)[:6] + b"", b_array("XB", "s", 3)[:-1], b_array("XB", "s", 3)[:-1] + hp,  # inside a B count; inside its data
               b"XXZabc", b"XXZabc" + hp,                                                      # a Z without its NUL (the tag's bytes inside it)
               hp + b"NMC", hp + b"XB" + b"Bq" + struct.pack("<i", 1) + b"\x00", hp + b"XYB" + b"c" + struct.pack("<i", -1),  # found, then unwalkable
               hp + b"XY?\x00"]                                                                # an unknown type letter
    value, kind = read_tag(regions)
    assert list(zip(value, kind))[:4] == [(ord("Z"), OTHER), (ord("H"), OTHER), (ord("B"), OTHER), (ord("f"), OTHER)]
    # (b_array(...)[:-1] + hp: the B field swallows the first byte of the next field and the walk ends off the region's end)
    assert kind[4:] == [UNWALKABLE] * 14 and value[4:] == [0] * 14


def test_reader_on_no_record_and_on_bad_arguments():
    from remora_amd import RemoraError
    from remora_amd.pileup import read_aux_values

    value, kind = read_aux_values(b"", np.zeros(1, np.int64), np.zeros(0, np.int64), "HP")
    assert value.size == 0 and kind.size == 0 and value.dtype == np.int64 and kind.dtype == np.uint8
    for bad in ("H_", "1P", "H"):
        with pytest.raises(RemoraError, match="two characters"):
            read_aux_values(b"", np.zeros(1, np.int64), np.zeros(0, np.int64), bad)
    # a tag offset outside its record: unwalkable, nothing read
    body = mr.bam_record("r", 0, 0, 10, [("M", 4)], "ACGT", tags=b"HPc\x01", has_md=False)[4:]
    for off in (-1, len(body) + 1):
        assert [a.tolist() for a in read_aux_values(body, np.array([0, len(body)]), np.array([off]), "HP")] == [[0], [UNWALKABLE]]
    assert [a.tolist() for a in read_aux_values(body, np.array([0, len(body)]), np.array([len(body)]), "HP")] == [[0], [ABSENT]]


def test_reader_is_declared_exported_and_bound():
    import ctypes

    from remora_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "remora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rmr_bam_aux_values", "rmr_pileup_stamp_partition"):
        assert re.search(rf"\b{name}\s*\(", code) and hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert any(name in c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S)), name
    for k, name in enumerate(("ABSENT", "INT", "CHAR", "OTHER_TYPE", "UNWALKABLE")):
        assert re.search(rf"#define RMR_AUX_{name} {k}\b", hdr) and getattr(_lib, f"AUX_{name}") == k


# ---- the bit plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_contigs,contig_bits,part_bits", [(1, 0, 8), (2, 1, 8), (3, 2, 8), (65536, 16, 8), (65537, 17, 7), (2**23, 23, 1)])
def test_bit_plan(n_contigs, contig_bits, part_bits):
    from remora_amd.pileup import partition_bit_plan

    plan = partition_bit_plan(n_contigs, "HP")
    assert (plan.contig_bits, plan.part_bits) == (contig_bits, part_bits)
    assert (1 << contig_bits) >= n_contigs and (contig_bits == 0 or (1 << (contig_bits - 1)) < n_contigs)  # the rule of rmr_pileup_create
    assert plan.max_values == (1 << part_bits) - 1 and plan.shift == 36 + contig_bits and 36 <= plan.shift <= 59
    assert plan.n_contigs == 1 << (contig_bits + part_bits) and plan.n_contigs <= 1 << 24  # what rmr_pileup_create takes


def test_bit_plan_refuses_a_header_that_leaves_no_bit():
    from remora_amd import RemoraError
    from remora_amd.pileup import partition_bit_plan

    with pytest.raises(RemoraError, match=r"--partition-tag HP: the BAM header has 8388609 contigs.*none is left"):
        partition_bit_plan(2**23 + 1, "HP")
    with pytest.raises(RemoraError):
        partition_bit_plan(2**24, "HP")


# ---- ids, labels, file names ----------------------------------------------------------------------------------------------------
class _Batch:
    def __init__(self, n):
        self.names = b"".join(f"read{r}\x00".encode() for r in range(n))
        self.name_off = np.concatenate([[0], np.cumsum([len(f"read{r}") + 1 for r in range(n)])])


def test_ids_come_in_order_of_first_appearance_and_live_across_batches():
    from remora_amd import RemoraError
    from remora_amd.pileup import Partitioner, partition_bit_plan

    p = Partitioner("HP", partition_bit_plan(2**22, "HP"))  # two bits: three values
    assert p.plan.max_values == 3
    kind = np.array([INT, ABSENT, INT, UNWALKABLE, INT, INT], np.uint8)
    assert p.ids_of(_Batch(6), np.array([7, 0, -1, 0, 7, -1]), kind, "a.bam").tolist() == [1, 0, 2, 0, 1, 2]
    assert p.ids_of(_Batch(2), np.array([-1, 5]), np.array([INT, INT], np.uint8), "a.bam").tolist() == [2, 3]
    assert p.ids_of(_Batch(1), np.array([0]), np.array([ABSENT], np.uint8), "a.bam").tolist() == [0]
    assert p.key_of_id() == {0: None, 1: (INT, 7), 2: (INT, -1), 3: (INT, 5)}
    with pytest.raises(RemoraError, match=r"--partition-tag HP: more than 3 distinct values - HP = '9' of read read1 \(b.bam\) did not fit"):
        p.ids_of(_Batch(2), np.array([5, 9]), np.array([INT, INT], np.uint8), "b.bam")
    with pytest.raises(RemoraError, match=r"HP is a character in read read1 of b.bam and an integer in the records before"):
        p.ids_of(_Batch(2), np.array([5, 65]), np.array([INT, CHAR], np.uint8), "b.bam")
    with pytest.raises(RemoraError, match=r"read read2 of b.bam has HP of type Z"):
        p.ids_of(_Batch(3), np.array([5, 0, ord("Z")]), np.array([INT, ABSENT, OTHER], np.uint8), "b.bam")


def test_label_order_and_file_names():
    from remora_amd.pileup import partition_file_name, partition_label, partition_order

    keys = [None, (CHAR, ord("b")), (INT, 10), (INT, -1), (CHAR, ord("A")), (INT, 2), (CHAR, ord("-"))]
    ordered = partition_order(keys)
    assert [partition_label(k) for k in ordered] == ["-1", "2", "10", "-", "A", "b", "ungrouped"]
    assert partition_file_name("s.bed", "HP", "1") == "s.HP_1.bed" and partition_file_name("s.bed", "HP", "ungrouped") == "s.ungrouped.bed"
    assert partition_file_name("out.d/s", "HP", "2") == "out.d/s.HP_2" and partition_file_name("out.d/s", "HP", "ungrouped") == "out.d/s.ungrouped"
    assert partition_file_name("a/s.counts.tsv", "hp", "-12") == "a/s.counts.hp_-12.tsv"
    assert partition_file_name("s.bed", "HP", "A") == "s.HP_A.bed" and partition_file_name("s.bed", "HP", "7") == "s.HP_7.bed"
    assert partition_file_name("s.bed", "HP", "-") == "s.HP_x2D.bed" and partition_file_name("s.bed", "HP", "/") == "s.HP_x2F.bed"
    assert partition_file_name("s.bed", "HP", "\xff") == "s.HP_xFF.bed"


def _partitioned_table():
    from remora_amd.pileup import PileupTable

    #            C  m  fail                  partition
    counts = [[3, 1, 2],    # chrA 5 +       1
              [0, 0, 4],    # chrB 0 -       1   nothing passes: no bedMethyl row
              [1, 1, 0],    # chrA 5 +       2
              [2, 0, 0],    # chrA 9 -       2
              [0, 5, 1]]    # chrA 5 +       ungrouped
    return PileupTable(ref_names=["chrA", "chrB"], ref_id=np.array([0, 1, 0, 0, 0], np.int32), pos=np.array([5, 0, 5, 9, 5], np.int64),
                       strand=np.array([0, 1, 0, 1, 0], np.uint8), counts=np.array(counts, np.int64), alphabet=["C", "m"], threshold_k=300, n_calls=20,
                       n_flushes=1, peak_device_bytes=0, hist=np.arange(513, dtype=np.int64), combined=False,
                       partition=np.array([0, 0, 1, 1, 3], np.int32), partition_labels=["1", "2", "3", "ungrouped"], partition_tag="HP")


def test_partition_tables_and_write_partitioned_on_a_hand_made_table(tmp_path):
    from remora_amd import RemoraError
    from remora_amd.pileup import PileupTable, partition_tables, write_bedmethyl, write_counts, write_partitioned

    # the partition rides beside the tuple's fields, which stay the twelve they were: positional construction is as before
    assert PileupTable._fields[-1] == "combined" and len(PileupTable._fields) == 12
    plain = PileupTable(["chrA"], np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.uint8), np.ones((1, 3), np.int64), ["C", "m"], 0, 3, 1, 0, None)
    assert plain.partition is None and plain.partition_labels is None and plain.partition_tag is None and plain.combined is False
    for fn in (partition_tables, lambda t: write_partitioned(t, tmp_path / "no.bed")):
        with pytest.raises(RemoraError, match="a run with a partition tag"):
            fn(plain)
    t = _partitioned_table()
    subs = partition_tables(t)
    assert list(subs) == ["1", "2", "3", "ungrouped"]
    assert [s.pos.size for s in subs.values()] == [2, 2, 0, 1] and [s.n_calls for s in subs.values()] == [10, 4, 0, 6]
    for s in subs.values():
        assert s.partition is None and s.partition_labels is None and s.partition_tag is None
        assert s.threshold_k == 300 and s.hist is t.hist and s.ref_names == t.ref_names and s.alphabet == t.alphabet
    assert subs["2"].ref_id.tolist() == [0, 0] and subs["2"].pos.tolist() == [5, 9] and subs["2"].strand.tolist() == [0, 1]
    assert subs["2"].counts.tolist() == [[1, 1, 0], [2, 0, 0]]
    rows = write_partitioned(t, tmp_path / "s.bed", tmp_path / "c.tsv")
    assert rows == {"1": 1, "2": 2, "ungrouped": 1}
    assert sorted(os.listdir(tmp_path)) == ["c.HP_1.tsv", "c.HP_2.tsv", "c.ungrouped.tsv", "s.HP_1.bed", "s.HP_2.bed", "s.ungrouped.bed"]
    for label, name in (("1", "HP_1"), ("2", "HP_2"), ("ungrouped", "ungrouped")):
        write_bedmethyl(subs[label], tmp_path / "want.bed")
        write_counts(subs[label], tmp_path / "want.tsv")
        assert (tmp_path / f"s.{name}.bed").read_bytes() == (tmp_path / "want.bed").read_bytes()
        assert (tmp_path / f"c.{name}.tsv").read_bytes() == (tmp_path / "want.tsv").read_bytes()
    assert (tmp_path / "s.HP_1.bed").read_text() == "chrA\t5\t6\tm\t4\t+\t5\t6\t255,0,0\t4\t25.00\n"
    assert (tmp_path / "c.ungrouped.tsv").read_text() == "chrom\tstart\tstrand\tN_C\tN_m\tN_fail\nchrA\t5\t+\t0\t5\t1\n"
    assert write_partitioned(t, tmp_path / "deep", min_coverage=5) == {"1": 0, "2": 0, "ungrouped": 1}  # no extension: appended
    assert (tmp_path / "deep.HP_1").read_text() == "" and (tmp_path / "deep.ungrouped").read_text().count("\n") == 1


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_parser_takes_the_partition_tag(capsys):
    from remora_amd.__main__ import _pileup_modbams, build_parser

    ap = build_parser()
    base = ["analyze", "pileup_modbams", "--bam", "a.bam", "--out-bed", "s.bed", "--canonical-base", "C", "--mod-bases", "m"]
    assert ap.parse_args(base).partition_tag is None
    a = ap.parse_args(base + ["--partition-tag", "HP"])
    assert a.partition_tag == "HP" and a.func is _pileup_modbams and a.out_bed == "s.bed"
    assert ap.parse_args(base + ["--partition-tag", "h1"]).partition_tag == "h1"
    for bad in ("H", "HPX", "1P", "H_", ""):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--partition-tag", bad])
        assert "--partition-tag is the two characters of an aux tag" in capsys.readouterr().err


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------
def test_sanitizer_program_of_the_reader_passes(tmp_path):
    """tools/fuzz/aux_tag_asan.cpp, compiled by the line tools/fuzz/run.sh has for it (its output path replaced) and run: a
    program of its own, nothing of it is loaded into this process."""
    fuzz = os.path.join(ROOT, "tools", "fuzz")
    script = open(os.path.join(fuzz, "run.sh")).read().splitlines()
    line = [ln for ln in script if ln.startswith("g++") and ln.endswith(" aux_tag_asan.cpp")]
    assert len(line) == 1 and "-fsanitize=address,undefined" in line[0] and "/tmp/rmr_aux_tag_asan" in script
    exe = str(tmp_path / "aux_tag_asan")
    subprocess.run(line[0].replace("/tmp/rmr_aux_tag_asan", exe).split(), cwd=fuzz, check=True, timeout=300)
    out = subprocess.run([exe], cwd=fuzz, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    m = re.fullmatch(r"aux regions: (\d+) absent, (\d+) integer, (\d+) character, (\d+) of another type, (\d+) unwalkable\n", out.stdout)
    assert m and all(int(g) >= 1000 for g in m.groups()), out.stdout
