"""`analyze pileup_modbams --ref`, the host side: the span index of a FASTA file on hand-written files, the motif descriptors
against a Python statement of the rule, the refusals of the command line, the writers' strand column, and the new symbols of
the C ABI.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW_SYMBOLS = ("rmr_ref_genome_create", "rmr_ref_genome_load", "rmr_ref_genome_read", "rmr_ref_genome_destroy", "rmr_pileup_emit_counts",
               "rmr_pileup_emit_fill")
REMOVED_SYMBOLS = ("rmr_modbam_call_counts", "rmr_modbam_call_fill", "rmr_modbam_call_counts_ref", "rmr_modbam_call_fill_ref",
                   "rmr_modbam_call_counts_duplex", "rmr_modbam_call_fill_duplex")


# ---- the FASTA span index -------------------------------------------------------------------------------------------------------
def spans_of(text):
    from remora_amd.pileup import fasta_spans

    return [(s.name, text[s.start : s.end], s.line_bases, s.line_width, s.n_bases) for s in fasta_spans(text)]


def test_span_index_on_hand_written_files():
    # LF: last line short, last line full, a single-line contig, a header with a description
    text = b">one first contig\nACGTAC\nGTACGT\nAC\n>two\nACGT\nACGT\n>three\tx=1\nACGTACGTAC\n"
    assert spans_of(text) == [("one", b"ACGTAC\nGTACGT\nAC", 6, 7, 14), ("two", b"ACGT\nACGT", 4, 5, 8), ("three", b"ACGTACGTAC", 10, 11, 10)]
    # CRLF, in the headers too
    text = b">one first contig\r\nACGTAC\r\nGTACGT\r\nAC\r\n>two\r\nACGT\r\nACGT\r\n"
    assert spans_of(text) == [("one", b"ACGTAC\r\nGTACGT\r\nAC", 6, 8, 14), ("two", b"ACGT\r\nACGT", 4, 6, 8)]
    # no trailing newline; blank lines at the end and between contigs; a contig without a sequence
    assert spans_of(b">a\nACG\nT") == [("a", b"ACG\nT", 3, 4, 4)]
    assert spans_of(b">a\nACG\nACG") == [("a", b"ACG\nACG", 3, 4, 6)]
    assert spans_of(b">a\nACG\nT\n\n\n>b\nAC\n \n\r\n\n") == [("a", b"ACG\nT", 3, 4, 4), ("b", b"AC", 2, 3, 2)]
    assert spans_of(b">a\n>b\nAC\n>c") == [("a", b"", 0, 1, 0), ("b", b"AC", 2, 3, 2), ("c", b"", 0, 1, 0)]
    # the number of bases is what `samtools faidx` computes from the first line, whatever the lines in between look like:
    # the device verifies them when the contig is loaded
    assert spans_of(b">a\nACGT\nAC\nACGT\n") == [("a", b"ACGT\nAC\nACGT", 4, 5, 10)]
    # a '>' inside a header is part of it
    assert spans_of(b">a b>c\nAC\n")[0][:2] == ("a", b"AC")


def test_span_index_refusals(tmp_path):
    from remora_amd import RemoraError
    from remora_amd.pileup import RefGenome, check_fasta_contigs, fasta_spans

    with pytest.raises(RemoraError, match="decompress it first"):
        fasta_spans(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff", "g.fa.gz")
    with pytest.raises(RemoraError, match="does not begin with '>'"):
        fasta_spans(b"ACGT\n")
    with pytest.raises(RemoraError, match="does not begin with '>'"):
        fasta_spans(b"")
    with pytest.raises(RemoraError, match="the contig name chr1 occurs twice"):
        fasta_spans(b">chr1 a\nAC\n>chr2\nAC\n>chr1 b\nAC\n")
    with pytest.raises(RemoraError, match="header without a name"):
        fasta_spans(b">chr1\nAC\n> \nAC\n")
    with pytest.raises(RemoraError, match="contig a: a blank line after the header"):
        fasta_spans(b">a\n\nAC\n")
    spans = fasta_spans(b">chr1\nACGT\nAC\n>chr2\nAC\n>extra\nA\n")
    got = check_fasta_contigs(spans, ["chr2", "chr1"], [2, 6], [0, 1])  # FASTA contigs the header does not name are skipped
    assert {c: s.name for c, s in got.items()} == {0: "chr2", 1: "chr1"}
    with pytest.raises(RemoraError, match="no contig chrM,"):
        check_fasta_contigs(spans, ["chr1", "chrM"], [6, 16569], [0, 1])
    check_fasta_contigs(spans, ["chr1", "chrM"], [6, 16569], [0])  # (not asked for: not missed)
    with pytest.raises(RemoraError, match=r"contig chr1 has 6 bases \(lines of 4\), the BAM header says 7"):
        check_fasta_contigs(spans, ["chr1", "chr2"], [7, 2], [0, 1])
    # from_fasta refuses all of these before it asks for a device
    gz = tmp_path / "g.fa.gz"
    gz.write_bytes(b"\x1f\x8b\x08\x00" + b"\x00" * 20)
    with pytest.raises(RemoraError, match=r"g\.fa\.gz is gzip- or BGZF-compressed: decompress it first"):
        RefGenome.from_fasta(gz, ["chr1"], [6])
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">chr1\nACGT\nAC\n")
    with pytest.raises(RemoraError, match="no contig chr2"):
        RefGenome.from_fasta(fa, ["chr1", "chr2"], [6, 5])
    with pytest.raises(RemoraError, match="contig chr1 has 6 bases"):
        RefGenome.from_fasta(fa, ["chr1"], [5])
    empty = tmp_path / "e.fa"
    empty.write_bytes(b"")
    with pytest.raises(RemoraError, match="it is empty"):
        RefGenome.from_fasta(empty, ["chr1"], [5])
    assert RefGenome.n_open == 0


# ---- motif descriptors ----------------------------------------------------------------------------------------------------------
SETS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT",
        "V": "ACG", "N": "ACGT"}


def stated(motif, focus):
    """The rule in a dozen lines: a nibble per base, bit 0 A, 1 C, 2 G, 3 T; the reverse complement reads the motif backwards
    with A <-> T and C <-> G, which on a nibble is its bits in reverse order; a '-' call moves down by L - 1 - 2 f."""
    bit = {"A": 1, "C": 2, "G": 4, "T": 8}
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    nibbles = [sum(bit[b] for b in SETS[c]) for c in motif]
    rc_nibbles = [sum(bit[comp[b]] for b in SETS[c]) for c in reversed(motif)]
    word = lambda ns: sum(n << (4 * i) for i, n in enumerate(ns))  # noqa: E731
    return len(motif), focus, word(nibbles), word(rc_nibbles), len(motif) - 1 - 2 * focus


@pytest.mark.parametrize("motif,focus,mask,rc,d", [("CG", 0, 0x42, 0x42, 1), ("GC", 1, 0x24, 0x24, -1), ("GATC", 1, 0x2814, 0x2814, 1),
                                                    ("CHH", 0, 0xBB2, 0x4DD, 2), ("CN", 0, 0xF2, 0x4F, 1)])
def test_motif_descriptors(motif, focus, mask, rc, d):
    from remora_amd.pileup import motif_descriptor

    got = motif_descriptor(motif, focus)
    assert (got.length, got.focus, got.mask, got.rc_mask, got.shift) == stated(motif, focus) == (len(motif), focus, mask, rc, d)
    assert got.motif == motif  # as written: the N of CN is a base of the window
    assert motif_descriptor(motif.lower(), str(focus)) == got


def test_motif_descriptor_of_every_letter_and_refusals():
    from remora_amd import RemoraError
    from remora_amd.pileup import check_pileup_motifs, motif_descriptor

    every = "ACGTRYSWKMBDHVNC"
    got = motif_descriptor(every, 15)
    assert (got.length, got.focus, got.mask, got.rc_mask, got.shift) == stated(every, 15)
    assert motif_descriptor("CU", 0).mask == motif_descriptor("CT", 0).mask
    ok = check_pileup_motifs([("CG", 0), ("GC", 1), ("GATC", 3), ("CCGG", 0)], "C", True)
    assert [d.shift for d in ok] == [1, -1, -3, 3] and all(d.mask == d.rc_mask for d in ok)
    assert [d.motif for d in check_pileup_motifs([("CHH", 0), ("CHG", 0)], "C", False)] == ["CHH", "CHG"]
    assert check_pileup_motifs([("TA", 0)], "U", False)[0].mask == 0x18
    with pytest.raises(RemoraError, match="--combine-strands: the motif CHH is not its own reverse complement"):
        check_pileup_motifs([("CG", 0), ("CHH", 0)], "C", True)
    with pytest.raises(RemoraError, match="--motif: 1 to 4 motifs, got 5"):
        check_pileup_motifs([("CG", 0), ("CA", 0), ("CC", 0), ("CT", 0), ("CN", 0)], "C", False)
    with pytest.raises(RemoraError, match="--motif: 1 to 4 motifs, got 0"):
        check_pileup_motifs([], "C", False)
    with pytest.raises(RemoraError, match="--motif CGCGCGCGCGCGCGCGC: a motif has 1 to 16 bases, this one 17"):
        check_pileup_motifs([("CG" * 8 + "C", 0)], "C", False)
    with pytest.raises(RemoraError, match=r"--motif CG 1: the focus base is G, the canonical base of the pileup is C \(--canonical-base\)"):
        check_pileup_motifs([("CG", 1)], "C", False)
    with pytest.raises(RemoraError, match="past the end"):
        motif_descriptor("CG", 2)
    with pytest.raises(RemoraError, match="outside the motif"):
        motif_descriptor("CG", -1)
    with pytest.raises(RemoraError, match="invalid characters"):
        motif_descriptor("CX", 0)
    with pytest.raises(RemoraError, match="not an integer"):
        motif_descriptor("CG", "x")


# ---- the command line -----------------------------------------------------------------------------------------------------------
BASE = ["analyze", "pileup_modbams", "--bam", "absent.bam", "--out-bed", "absent.bed", "--canonical-base", "C", "--mod-bases", "m"]


def test_parser_takes_the_reference_arguments():
    from remora_amd.__main__ import build_parser

    ap = build_parser()
    a = ap.parse_args(BASE + ["--ref", "g.fa", "--motif", "CG", "0", "--motif", "GC", "1", "--combine-strands"])
    assert a.ref == "g.fa" and a.motif == [["CG", "0"], ["GC", "1"]] and a.combine_strands is True and a.cpg is False
    a = ap.parse_args(BASE + ["--ref", "g.fa", "--cpg"])
    assert a.cpg is True and a.motif is None and a.combine_strands is False
    d = ap.parse_args(BASE)
    assert d.ref is None and d.motif is None and d.cpg is False and d.combine_strands is False
    with pytest.raises(SystemExit):
        ap.parse_args(BASE + ["--motif", "CG"])


@pytest.mark.parametrize("extra,message", [
    (["--motif", "CG", "0"], "--motif needs --ref"),
    (["--cpg"], "--cpg needs --ref"),
    (["--combine-strands"], "--combine-strands needs --ref"),
    (["--ref", "g.fa"], "--ref needs a motif: give --motif MOTIF FOCUS or --cpg"),
    (["--ref", "g.fa", "--cpg", "--motif", "CG", "0"], "--cpg is --motif CG 0: give one of --cpg and --motif, not both"),
    (["--ref", "g.fa", "--motif", "CA", "0", "--motif", "CC", "0", "--motif", "CG", "0", "--motif", "CT", "0", "--motif", "CN", "0"],
     "--motif: 1 to 4 motifs, got 5"),
    (["--ref", "g.fa", "--motif", "C" * 17, "0"], "a motif has 1 to 16 bases, this one 17"),
    (["--ref", "g.fa", "--motif", "CG", "1"], "--motif CG 1: the focus base is G, the canonical base of the pileup is C"),
    (["--ref", "g.fa", "--motif", "CHH", "0", "--combine-strands"], "--combine-strands: the motif CHH is not its own reverse complement"),
])
def test_command_line_refusals_name_the_argument(extra, message, capsys, tmp_path):
    """Each is refused before the BAM, the FASTA or a device is touched: none of the files exists."""
    from remora_amd.__main__ import main

    argv = list(BASE)
    argv[argv.index("absent.bed")] = str(tmp_path / "absent.bed")
    assert main(argv + extra) == 1
    assert message in capsys.readouterr().err and not (tmp_path / "absent.bed").exists()


def test_cpg_needs_canonical_base_c(capsys):
    from remora_amd.__main__ import main
    from remora_amd.pileup import check_ref_arguments

    argv = list(BASE)
    argv[argv.index("--canonical-base") + 1] = "A"
    assert main(argv + ["--ref", "g.fa", "--cpg"]) == 1
    assert "--cpg needs --canonical-base C, got A" in capsys.readouterr().err
    assert check_ref_arguments("g.fa", None, True, True, "C") == [("CG", 0)]
    assert check_ref_arguments("g.fa", [["GATC", "1"]], False, False, "A") == [["GATC", "1"]]
    assert check_ref_arguments(None, None, False, False, "C") is None


# ---- the table and the writers --------------------------------------------------------------------------------------------------
def test_writers_print_a_dot_for_combined_strands(tmp_path):
    from remora_amd.pileup import PileupTable, write_bedmethyl, write_counts

    kw = dict(ref_names=["chrA"], ref_id=np.array([0, 0], np.int32), pos=np.array([5, 9], np.int64), strand=np.array([0, 0], np.uint8),
              counts=np.array([[3, 1, 0], [0, 2, 2]], np.int64), alphabet=["C", "m"], threshold_k=300, n_calls=8, n_flushes=1, peak_device_bytes=0,
              hist=None)
    plain = PileupTable(**kw)  # the trailing field has a default: tables built before it existed still build
    assert plain.combined is False and PileupTable._fields[-1] == "combined" and PileupTable(*kw.values()).combined is False
    bed, tsv = tmp_path / "s.bed", tmp_path / "c.tsv"
    write_bedmethyl(plain, bed), write_counts(plain, tsv)
    assert bed.read_text() == "chrA\t5\t6\tm\t4\t+\t5\t6\t255,0,0\t4\t25.00\nchrA\t9\t10\tm\t2\t+\t9\t10\t255,0,0\t2\t100.00\n"
    assert tsv.read_text() == "chrom\tstart\tstrand\tN_C\tN_m\tN_fail\nchrA\t5\t+\t3\t1\t0\nchrA\t9\t+\t0\t2\t2\n"
    comb = PileupTable(combined=True, **kw)
    write_bedmethyl(comb, bed), write_counts(comb, tsv)
    assert bed.read_text() == "chrA\t5\t6\tm\t4\t.\t5\t6\t255,0,0\t4\t25.00\nchrA\t9\t10\tm\t2\t.\t9\t10\t255,0,0\t2\t100.00\n"
    assert tsv.read_text() == "chrom\tstart\tstrand\tN_C\tN_m\tN_fail\nchrA\t5\t.\t3\t1\t0\nchrA\t9\t.\t0\t2\t2\n"


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from remora_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "remora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), f"{name} is not declared"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
        assert any(name in c for c in re.findall(r"/\*.*?\*/", hdr, flags=re.S)), name
    mk = open(os.path.join(ROOT, "remora_amd", "csrc", "Makefile")).read()
    assert "k_ref_genome.hip" in mk and "api_ref.hip" in mk
    assert re.search(r"#define RMR_PILEUP_MAX_MOTIFS 4\b", hdr) and re.search(r"#define RMR_PILEUP_MAX_MOTIF_LEN 16\b", hdr)
    assert ctypes.sizeof(_lib.PileupMotif) == 24 and ctypes.sizeof(_lib.PileupRef) == 16 + 4 * 24  # the layout of the C structs
    # one emit pair: the engine, the batch, the options, (k_t,) and six arrays
    assert len(_lib.SIGNATURES["rmr_pileup_emit_counts"][1]) == 9 and len(_lib.SIGNATURES["rmr_pileup_emit_fill"][1]) == 10
    # the three generations of entries it replaces are gone: not declared, not bound, not exported
    for name in REMOVED_SYMBOLS:
        assert not re.search(rf"\b{name}\b", code), f"{name} is still declared"
        assert name not in _lib.SIGNATURES and not hasattr(L, name), name
    # the options struct of the header, field for field (names and C types), in the ctypes binding
    body = re.search(r"typedef struct rmr_pileup_emit_opts \{(.*?)\} rmr_pileup_emit_opts;", code, flags=re.S).group(1)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "const rmr_pileup_ref *": ctypes.POINTER(_lib.PileupRef)}
    fields = [(n.strip(), ctype[t]) for t, names in re.findall(r"(int32_t|int64_t|const rmr_pileup_ref \*)\s*([\w\s,]+);", body)
              for n in names.split(",")]
    assert fields == list(_lib.PileupEmitOpts._fields_)
    assert [n for n, _ in fields] == ["region_ref", "region_lo", "region_hi", "ref", "duplex", "hemi"]
    assert len(re.findall(r";", body)) == 5  # (five declarations, region_lo and region_hi in one: nothing the pattern above passed over)
    assert ctypes.sizeof(_lib.PileupEmitOpts) == 40 and _lib.PileupEmitOpts.ref.offset == 24
