"""`analyze pileup_modbams`: the modified-base calls of mapped BAM files (MM / ML tags, as `infer from_pod5_and_bam` writes
them) counted per reference site - the bedMethyl table that genome browsers and differential-methylation tools read.  The
reference's command line stops at the per-read BAM; its users go through a CPU pileup over a sorted, indexed file next.

Here the BAM is streamed in any order (no index, no MD tag): a batch of records is tokenised on native threads
(rmr_mod_tags_sizes / _fill, shared with `validate from_modbams`), its calls are laid along the reads and carried through the
CIGARs on the GPU (rmr_pileup_emit_counts / _fill: the walk of the site join without the truth table), classified there in
integers and written as one 64-bit word per call; the words are sorted, counted per site and merged into a resident table on
the device (rmr_pileup_*, csrc/k_pileup.hip).  One row per site crosses PCIe.  What a run asks of the emit - the region, the
reference, `duplex`, `hemi` - travels in one rmr_pileup_emit_opts, filled once per run.

Which calls count, and how they are classified, is DESIGN.md section 4's "Pileup"; in short: mapped primary records, '+'-strand
entries with single-letter codes of the alphabet, the positions an entry lists, p = (ML + 0.5) / 256, the later entry wins,
bases inside M / = / X; class = argmax (ties to the lower column), confidence kmax = 512 x the winning probability, the call
passes when kmax >= k_T.

With a reference FASTA (`ref`, `motifs`) the genome is packed into nibbles on the device once (RefGenome, rmr_ref_genome_*,
csrc/k_ref_genome.hip) and the emit keeps a call only where the reference shows one of the motifs around it; with
`combine_strands` a '-' call is written at the '+' position of its motif, so that a CpG is one row (DESIGN.md section 4,
"Pileup: the reference").

With `partition_tag` (HP of phased reads) the records are piled per value of that aux tag in the same run: the value is read
on the host (rmr_bam_aux_values), given an id, and the id is stamped into the free bits above the contig index of the
record's words (rmr_pileup_stamp_partition) - the sort and the table then keep the partitions apart, under the one threshold
of the whole input ("Pileup: the partition field").

With `duplex` the '-'-strand entries of duplex records count too, on the reference strand opposite to the record's; with
`hemi` the '+' and the '-' call of one record at one motif site are paired on the device (rmr_pileup_pair_counts / _fill,
csrc/k_pileup_duplex.hip) and the table counts the strand patterns per site ("Pileup: duplex entries
and strand pairs").

With `coverage` the BAMs are streamed once more after the table is finished and every record is joined on the device against
the sites it spans (rmr_pileup_cover): N_delete, N_diff and N_nocall per site, the columns that make the bedMethyl the
eighteen-column form ("Pileup: the coverage join")."""
import ctypes
import logging
import mmap
import os
import re
from collections import namedtuple
from fractions import Fraction
from functools import partial

import numpy as np

from . import RemoraError

LOGGER = logging.getLogger("Remora")

N_BINS = 513                 # kmax = 0 .. 512
MAX_CONTIGS = 1 << 24        # the fields of a site word: ref_id 24 bits, position 31 bits
MAX_POS = 1 << 31
DEFAULT_PCT_FILT = 10.0
DEFAULT_DEVICE_GIB = 8.0
PILEUP_STATUS = {1: "no MM tag", 2: "malformed modified-base tags", 3: "unmapped", 5: "no modified base of the alphabet",
                 6: "secondary or supplementary"}
MOD_NOT_IN_ALPHABET = "Modified base found in BAM ({}) not among --mod-bases: its calls are not counted."

MAX_MOTIFS = 4               # RMR_PILEUP_MAX_MOTIFS, RMR_PILEUP_MAX_MOTIF_LEN of include/remora_hip.h
MAX_MOTIF_LEN = 16
DEFAULT_PIECE_BYTES = 64 << 20
# a base's code: the IUPAC set as a mask, A 1, C 2, G 4, T 8 (the complement of a code is its four bits reversed)
IUPAC_MASK = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 12, "M": 3, "B": 14, "D": 13, "H": 11, "V": 7, "N": 15}

_PileupFields = namedtuple("PileupTable", ("ref_names", "ref_id", "pos", "strand", "counts", "alphabet", "threshold_k", "n_calls", "n_flushes",
                                           "peak_device_bytes", "hist", "combined"), defaults=(False,))


class PileupTable(_PileupFields):
    """One row per site with a kept call, ordered by (ref_id, pos, strand): ref_id i32[n], pos i64[n], strand u8[n]
    (0 '+', 1 '-'), counts i64[n, len(alphabet) + 1] (canonical, the modified bases in alphabet order, fail).  threshold_k: k_T;
    n_calls: kept calls; n_flushes: flushes of the device call buffer; peak_device_bytes: the pileup's device memory at its
    peak (the reference genome included); hist: i64[513], the calls per kmax, when the threshold came from a percentile, else
    None; combined: the strands were combined - every row stands on '+' in `strand` and belongs to both strands (the writers
    print '.').
    A run with `partition_tag` has three more, keyword arguments and attributes beside the tuple's twelve fields (None
    otherwise, and in what _replace returns): one row per (partition, site), partition i32[n] an index into partition_labels -
    the labels that have a row, integers ascending, then characters by code, then "ungrouped" - and the rows ordered by
    (partition, ref_id, pos, strand); partition_tag names the tag.  partition_tables splits it into plain tables.
    A run with `hemi` has two more of that kind, hemi=True and n_unpaired: one row per motif site (its '+' position; combined is
    set) and counts i64[n, (n_mods + 2)^2] indexed by the pattern code a (n_mods + 2) + b - a / b the class of the '+' / '-' call
    of a pair, 0 canonical, 1 .. n_mods the modified bases, n_mods + 1 fail; n_calls counts the pairs, n_unpaired the kept
    calls without a partner in their record, and hist / threshold_k are those of all kept single calls.
    A run with `coverage` has one more of that kind: coverage i64[n, 3], per row the records that cover the site without a call
    there - N_delete, N_diff, N_nocall (pileup_modbams) - and None otherwise."""

    partition = partition_labels = partition_tag = n_unpaired = coverage = None
    hemi = False

    def __new__(cls, *args, partition=None, partition_labels=None, partition_tag=None, hemi=False, n_unpaired=None, coverage=None, **fields):
        self = super().__new__(cls, *args, **fields)
        self.partition, self.partition_labels, self.partition_tag = partition, partition_labels, partition_tag
        self.hemi, self.n_unpaired, self.coverage = bool(hemi), n_unpaired, coverage
        return self


# ---- the partition tag -----------------------------------------------------------------------------------------------------
CONTIG_SHIFT = 36            # the contig index starts at this bit of a site word (include/remora_hip.h)
MAX_PART_BITS = 8
UNGROUPED = "ungrouped"
_UNGROUPED_KEY = (3, 0)      # sorts behind (_lib.AUX_INT, value) and (_lib.AUX_CHAR, code)
PartitionPlan = namedtuple("PartitionPlan", ("contig_bits", "part_bits", "max_values", "shift", "n_contigs"))
PartitionPlan.__doc__ = """Where the partition id stands in a site word: above the contig_bits of the contig index, part_bits wide (ids 1 ..
max_values = 2^part_bits - 1; 0 is `ungrouped`), from bit `shift`; n_contigs: what the device pileup is created for."""


def check_partition_tag(tag):
    if not isinstance(tag, str) or re.fullmatch(r"[A-Za-z][A-Za-z0-9]", tag) is None:
        raise RemoraError(f"--partition-tag is the two characters of an aux tag, [A-Za-z][A-Za-z0-9] (HP for example), got {tag!r}")
    return tag


def partition_bit_plan(n_contigs, tag="the partition tag"):
    """The 24 bits of a site word's contig field shared between the contig index and the partition id -> PartitionPlan.
    contig_bits by the rule of rmr_pileup_create (the smallest c with 2^c >= n_contigs), the partition gets the rest, 8 bits
    at the most; refused when nothing is left."""
    n_contigs = int(n_contigs)
    if n_contigs < 1:
        raise RemoraError("the BAM header has no contig: nothing to pile up on")
    contig_bits = (n_contigs - 1).bit_length()
    part_bits = min(MAX_PART_BITS, 24 - contig_bits)
    if part_bits < 1:
        raise RemoraError(f"--partition-tag {tag}: the BAM header has {n_contigs} contigs, whose index takes {contig_bits} of the 24 bits of a "
                          f"site word's contig field: none is left for a partition (up to {1 << 23} contigs leave one)")
    return PartitionPlan(contig_bits, part_bits, (1 << part_bits) - 1, CONTIG_SHIFT + contig_bits, 1 << (contig_bits + part_bits))


def partition_label(key):
    """(kind, value) -> the label: the decimal of an integer, the character of an `A` value, "ungrouped"."""
    from . import _lib as L

    kind, value = key
    return str(int(value)) if kind == L.AUX_INT else chr(int(value)) if kind == L.AUX_CHAR else UNGROUPED


def partition_order(keys):
    """(kind, value) keys in label order: integers ascending numerically, characters by code, `ungrouped` (None) last."""
    return sorted(_UNGROUPED_KEY if k is None else (int(k[0]), int(k[1])) for k in keys)


def read_aux_values(raw, raw_off, tags_off, tag, threads=1):
    """rmr_bam_aux_values for the records of a batch -> (value i64[n], kind u8[n]).  One thread by default: the aux regions of
    512 records are walked in 35 us, less than it takes to start more threads."""
    from . import _lib as L

    lib = L.lib()
    threads = int(threads)
    raw_off, tags_off = np.ascontiguousarray(raw_off, np.int64), np.ascontiguousarray(tags_off, np.int64)
    n = int(tags_off.size)
    raw_arr = np.frombuffer(raw, np.uint8) if len(raw) else np.zeros(1, np.uint8)
    value, kind = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    L.check(lib.rmr_bam_aux_values(n, p(raw_arr), p(raw_off), p(tags_off), str(tag).encode("latin-1"), p(value), p(kind), threads))
    return value[:n], kind[:n]


class Partitioner:
    """The partition ids of a run: 0 is `ungrouped`, a value gets the next id when it is first seen, in either pass - ids are
    internal, the table is put into label order once it is read.  No Python object per record: np.unique per batch."""

    def __init__(self, tag, plan):
        self.tag, self.plan, self.ids, self.kind = tag, plan, {}, None

    def _read_name(self, rb, r):
        return bytes(rb.names[int(rb.name_off[r]) : int(rb.name_off[r + 1])]).rstrip(b"\x00").decode("latin-1")

    def ids_of(self, rb, value, kind, path):
        """part i32[n] of a batch's records, or the refusal: a tag of a type that is neither an integer nor a character, a tag
        that is an integer here and a character there, more values than the field holds."""
        from . import _lib as L

        tag = self.tag
        other = np.nonzero(kind == L.AUX_OTHER_TYPE)[0]
        if other.size:
            r = int(other[0])
            raise RemoraError(f"--partition-tag {tag}: read {self._read_name(rb, r)} of {path} has {tag} of type {chr(int(value[r]))}; a partition "
                              "is named by an integer (c C s S i I) or a character (A)")
        tagged = np.nonzero((kind == L.AUX_INT) | (kind == L.AUX_CHAR))[0]
        part = np.zeros(kind.size, np.int32)
        if not tagged.size:
            return part
        if self.kind is None:
            self.kind = int(kind[tagged[0]])
        odd = tagged[kind[tagged] != self.kind]
        if odd.size:
            r = int(odd[0])
            names = {L.AUX_INT: "an integer", L.AUX_CHAR: "a character"}
            raise RemoraError(f"--partition-tag {tag}: {tag} is {names[int(kind[r])]} in read {self._read_name(rb, r)} of {path} and "
                              f"{names[self.kind]} in the records before it; one run takes one kind")
        uniq, first, inverse = np.unique(value[tagged], return_index=True, return_inverse=True)
        for j in np.argsort(first, kind="stable").tolist():
            v = int(uniq[j])
            if v not in self.ids:
                if len(self.ids) >= self.plan.max_values:
                    r = int(tagged[first[j]])
                    raise RemoraError(f"--partition-tag {tag}: more than {self.plan.max_values} distinct values - {tag} = "
                                      f"{partition_label((self.kind, v))!r} of read {self._read_name(rb, r)} ({path}) did not fit: beside the "
                                      f"{self.plan.contig_bits} bits of the contig index a site word has {self.plan.part_bits} bits for the partition")
                self.ids[v] = len(self.ids) + 1
        part[tagged] = np.array([self.ids[int(v)] for v in uniq.tolist()], np.int32)[inverse.reshape(-1)]
        return part

    def key_of_id(self):
        """{id: (kind, value)}, None for `ungrouped`."""
        out = {0: None}
        out.update({i: (self.kind, v) for v, i in self.ids.items()})
        return out


def threshold_k(filter_threshold):
    """k_T = ceil(512 T) for a probability threshold 0 <= T <= 1, exactly."""
    t = Fraction(filter_threshold) if not isinstance(filter_threshold, float) else Fraction(repr(filter_threshold))
    if not 0 <= t <= 1:
        raise RemoraError(f"--filter-threshold is a probability, 0 to 1, got {filter_threshold}")
    k = 512 * t
    return int(-((-k.numerator) // k.denominator))


def percentile_k(hist, pct_filt):
    """k_T that filters `pct_filt` percent of the calls or fewer (ties): the largest k in 0 .. 513 with
    sum_{j<k} hist[j] <= floor(N pct / 100), N = sum(hist).  (k = 513, above every kmax, only at 100 percent.)"""
    p = Fraction(repr(float(pct_filt)))
    if not 0 <= p <= 100:
        raise RemoraError(f"--pct-filt is a percentage, 0 to 100, got {pct_filt}")
    hist = [int(h) for h in hist]
    if len(hist) != N_BINS:
        raise RemoraError(f"a confidence histogram has {N_BINS} bins, got {len(hist)}")
    n = sum(hist)
    allowed = (n * p.numerator) // (100 * p.denominator)
    below, k_t = 0, 0
    for k in range(1, N_BINS + 1):
        below += hist[k - 1]
        if below <= allowed:
            k_t = k
        else:
            break
    return k_t


def parse_region(region, ref_names, ref_lens):
    """`ctg` or `ctg:start-end` (0-based, half-open, the coordinates of the output's second and third column) ->
    (ref_id, start, end); None -> (-1, 0, 0)."""
    if region is None:
        return -1, 0, 0
    if isinstance(region, (tuple, list)):
        name, lo, hi = region
    elif region in ref_names:
        name, lo, hi = region, 0, None
    else:
        name, sep, span = str(region).rpartition(":")
        if not sep:
            raise RemoraError(f"--region names the contig {region!r}, which the BAM header does not have")
        m = re.fullmatch(r"([0-9,]+)-([0-9,]+)", span)
        if m is None:
            raise RemoraError(f"--region is ctg or ctg:start-end, got {region!r}")
        lo, hi = (int(x.replace(",", "")) for x in m.groups())
    if name not in ref_names:
        raise RemoraError(f"--region names the contig {name!r}, which the BAM header does not have")
    rid = ref_names.index(name)
    hi = int(ref_lens[rid]) if hi is None else int(hi)
    if lo < 0 or hi < lo:
        raise RemoraError(f"--region {region!r}: start-end must be 0 <= start <= end")
    return rid, int(lo), hi


def bam_reference_dict(bam_path):
    """[(name, length)] of a BAM header in ref_id order."""
    import struct

    from .io import read_bam_header_bytes

    hdr = read_bam_header_bytes(bam_path)
    at = 8 + struct.unpack_from("<i", hdr, 4)[0]
    n_ref = struct.unpack_from("<i", hdr, at)[0]
    at += 4
    out = []
    for _ in range(n_ref):
        ln = struct.unpack_from("<i", hdr, at)[0]
        out.append((hdr[at + 4 : at + 4 + ln - 1].decode(), struct.unpack_from("<I", hdr, at + 4 + ln)[0]))
        at += 8 + ln
    return out


def check_reference_dicts(bams, dicts):
    """The reference dictionaries of several BAMs must be equal; the refusal names the first difference."""
    for path, d in zip(bams[1:], dicts[1:]):
        for i, (a, b) in enumerate(zip(dicts[0], d)):
            if a != b:
                raise RemoraError(f"the reference dictionaries of {bams[0]} and {path} differ at contig #{i}: {a[0]} ({a[1]} bases) "
                                  f"against {b[0]} ({b[1]} bases); one pileup takes BAMs mapped to one reference")
        if len(d) != len(dicts[0]):
            raise RemoraError(f"the reference dictionaries of {bams[0]} and {path} differ: {len(dicts[0])} against {len(d)} contigs "
                              f"(the first {min(len(d), len(dicts[0]))} are equal)")


def check_site_fields(n_contigs, max_len):
    """What a 64-bit site word cannot hold is refused, before any launch."""
    if n_contigs < 1:
        raise RemoraError("the BAM header has no contig: nothing to pile up on")
    if n_contigs > MAX_CONTIGS:
        raise RemoraError(f"the BAM header has {n_contigs} contigs; a pileup holds up to {MAX_CONTIGS} (24 bits of a site word)")
    if max_len > MAX_POS:
        raise RemoraError(f"the longest contig has {max_len} bases; a pileup holds positions below {MAX_POS} (31 bits of a site word)")


def check_alphabet(alphabet):
    alphabet = list(alphabet)
    mods = alphabet[1:]
    if not 1 <= len(mods) <= 7 or any(len(m) != 1 for m in alphabet) or len(set(alphabet)) != len(alphabet):
        raise RemoraError(f"pileup_modbams takes 1 to 7 distinct single-letter modified bases beside the canonical base, got {alphabet}")
    return alphabet


def bytes_per_buffered_call(n_alpha):
    """Device bytes the pileup's work block takes per word of its call buffer (include/remora_hip.h, rmr_pileup_create)."""
    return 52 + 4 * (n_alpha + 1)


# ---- motifs --------------------------------------------------------------------------------------------------------------
MotifDescriptor = namedtuple("MotifDescriptor", ("motif", "length", "focus", "mask", "rc_mask", "shift"))
MotifDescriptor.__doc__ = """A motif as the emit kernel takes it: `length` nibbles of IUPAC masks, base i in bits 4 i .. 4 i + 3 of
`mask`; rc_mask[i] = complement(mask[length - 1 - i]); shift = length - 1 - 2 focus, what a '-' call moves down by when the
strands are combined."""


def _reverse4(code):
    return ((code & 1) << 3) | ((code & 2) << 1) | ((code & 4) >> 1) | ((code & 8) >> 3)


def motif_descriptor(motif, focus):
    """(motif, focus) -> MotifDescriptor.  util.Motif validates the letters and the focus; the motif is taken as written - a
    leading or trailing N, which util.Motif clips, stays: next to a contig's end, or where the reference itself has an N, it
    is not neutral."""
    from .util import Motif

    raw = str(motif).upper().replace("U", "T")
    Motif(raw, focus)  # RemoraError for a letter outside IUPAC, a focus that is no integer or lies past the end
    focus = int(focus)
    if not 1 <= len(raw) <= MAX_MOTIF_LEN:
        raise RemoraError(f"--motif {motif}: a motif has 1 to {MAX_MOTIF_LEN} bases, this one {len(raw)}")
    if not 0 <= focus < len(raw):
        raise RemoraError(f"--motif {motif} {focus}: the focus position lies outside the motif")
    codes = [IUPAC_MASK[c] for c in raw]
    mask = sum(c << (4 * i) for i, c in enumerate(codes))
    rc_mask = sum(_reverse4(c) << (4 * i) for i, c in enumerate(reversed(codes)))
    return MotifDescriptor(raw, len(raw), focus, mask, rc_mask, len(raw) - 1 - 2 * focus)


def check_pileup_motifs(motifs, canonical_base, combine_strands):
    """[(motif, focus)] -> [MotifDescriptor], or RemoraError naming the argument: more than 4 motifs, a motif longer than 16
    bases, a focus base that is not the canonical base, and with `combine_strands` a motif that is not its own reverse
    complement."""
    motifs = [tuple(m) for m in motifs]
    if not 1 <= len(motifs) <= MAX_MOTIFS:
        raise RemoraError(f"--motif: 1 to {MAX_MOTIFS} motifs, got {len(motifs)}")
    can = "T" if canonical_base == "U" else canonical_base
    out = []
    for motif, focus in motifs:
        d = motif_descriptor(motif, focus)
        if d.motif[d.focus] != can:
            raise RemoraError(f"--motif {motif} {focus}: the focus base is {d.motif[d.focus]}, the canonical base of the pileup is "
                              f"{canonical_base} (--canonical-base)")
        if combine_strands and d.mask != d.rc_mask:
            raise RemoraError(f"--combine-strands: the motif {d.motif} is not its own reverse complement (CG, GC, GATC, ... are); its "
                              "two strands do not share a site")
        out.append(d)
    return out


def check_ref_arguments(ref, motifs, cpg, combine_strands, canonical_base):
    """The command line's --ref / --motif / --cpg / --combine-strands -> the `motifs` of pileup_modbams (None without a
    reference), or RemoraError naming the argument."""
    motifs = list(motifs or [])
    if cpg and motifs:
        raise RemoraError("--cpg is --motif CG 0: give one of --cpg and --motif, not both")
    if cpg:
        if canonical_base != "C":
            raise RemoraError(f"--cpg needs --canonical-base C, got {canonical_base}")
        motifs = [("CG", 0)]
    if ref is None:
        for given, name in ((cpg, "--cpg"), (motifs, "--motif"), (combine_strands, "--combine-strands")):
            if given:
                raise RemoraError(f"{name} needs --ref: the motif is looked up in the reference FASTA")
        return None
    if not motifs:
        raise RemoraError("--ref needs a motif: give --motif MOTIF FOCUS or --cpg")
    check_pileup_motifs(motifs, canonical_base, combine_strands)
    return motifs


def check_hemi_arguments(ref, motifs, combine_strands, partition_tag, alphabet):
    """What `hemi` needs beside it, or RemoraError naming the argument: a reference, exactly one motif that is its own reverse
    complement, at most two modified bases ((n_mods + 2)^2 pattern codes fit the 4 bits of a site word's code), no
    --combine-strands (the fold is implied) and no --partition-tag.  `motifs`: [(motif, focus)] as check_ref_arguments returns
    them.  -> the motif's MotifDescriptor.  No device is touched."""
    alphabet = check_alphabet(alphabet)
    if ref is None:
        raise RemoraError("--hemi needs --ref: the two strands of a site are found through the motif in the reference FASTA")
    motifs = [tuple(m) for m in (motifs or [])]
    if len(motifs) != 1:
        raise RemoraError(f"--hemi takes exactly one motif (--cpg, or one --motif MOTIF FOCUS), got {len(motifs)}")
    if combine_strands:
        raise RemoraError("--hemi implies the fold of --combine-strands: give --hemi alone")
    if partition_tag is not None:
        raise RemoraError("--hemi with --partition-tag is not built: give one of them")
    if len(alphabet) - 1 > 2:
        raise RemoraError(f"--hemi counts (n + 2)^2 strand patterns of n modified bases in the 16 codes of a site word: at most two "
                          f"--mod-bases, got {len(alphabet) - 1} ({' '.join(alphabet[1:])})")
    d = check_pileup_motifs(motifs, alphabet[0], False)[0]
    if d.mask != d.rc_mask:
        raise RemoraError(f"--hemi: the motif {d.motif} is not its own reverse complement (CG, GC, GATC, ... are); its two strands do "
                          "not share a site")
    return d


def hemi_class_names(alphabet):
    """The classes of one strand's call in a hemi table: the canonical base, the modified bases, `fail`."""
    return list(alphabet) + ["fail"]


# ---- the reference FASTA -------------------------------------------------------------------------------------------------
FastaSpan = namedtuple("FastaSpan", ("name", "start", "end", "line_bases", "line_width", "n_bases"))
FastaSpan.__doc__ = """One contig of a FASTA file: its sequence lines are the bytes [start, end) (trailing white space stripped), in
lines of line_bases bases and line_width bytes (by the first line and its terminator); n_bases as `samtools faidx` computes it."""
REWRAP = "the lines of a contig must have one width: re-wrap the file, as `samtools faidx` requires"


def fasta_spans(buf, path="FASTA"):
    """[FastaSpan] of a FASTA file held in `buf` (bytes or an mmap), in file order, found with `find` only: no line of the
    sequence is looked at here - the device verifies them when a contig is loaded."""
    size = len(buf)
    if buf[:2] == b"\x1f\x8b":
        raise RemoraError(f"{path} is gzip- or BGZF-compressed: decompress it first, the reference is read as plain text")
    if size == 0 or buf[:1] != b">":
        raise RemoraError(f"{path} is not a FASTA file: it does not begin with '>'")
    spans, seen, h = [], set(), 0
    while h >= 0:
        eol = buf.find(b"\n", h)
        words = bytes(buf[h + 1 : eol if eol >= 0 else size]).split()
        if not words:
            raise RemoraError(f"{path}: a header without a name at byte {h}")
        name = words[0].decode("latin-1")
        if name in seen:
            raise RemoraError(f"{path}: the contig name {name} occurs twice")
        seen.add(name)
        start = eol + 1 if eol >= 0 else size
        nxt = buf.find(b"\n>", eol) if eol >= 0 else -1  # (from the header's own line end: a contig without a sequence)
        end = max(start, nxt + 1 if nxt >= 0 else size)
        while end > start and buf[end - 1] in b" \t\r\n":
            end -= 1
        nl = buf.find(b"\n", start, end)
        term = 2 if nl > start and buf[nl - 1] == 13 else 1
        line_bases = (nl if nl >= 0 else end) - start - (term - 1 if nl >= 0 else 0)
        width, n_text = line_bases + term, end - start
        if n_text and line_bases < 1:
            raise RemoraError(f"{path}: contig {name}: a blank line after the header; {REWRAP}")
        n_bases = (n_text // width) * line_bases + min(n_text % width, line_bases) if n_text else 0
        spans.append(FastaSpan(name, start, end, line_bases, width, n_bases))
        h = nxt + 1 if nxt >= 0 else -1
    return spans


def check_fasta_contigs(spans, ref_names, ref_lens, contigs, path="FASTA", bam="the BAM header"):
    """The contigs to load (indices into ref_names) must be in the FASTA with the header's length -> {index: FastaSpan}."""
    by_name = {s.name: s for s in spans}
    out = {}
    for c in contigs:
        name, want = ref_names[c], int(ref_lens[c])
        sp = by_name.get(name)
        if sp is None:
            raise RemoraError(f"{path} has no contig {name}, which {bam} names ({len(spans)} contigs in the FASTA)")
        if sp.n_bases != want:
            raise RemoraError(f"{path}: contig {name} has {sp.n_bases} bases (lines of {sp.line_bases}), {bam} says {want}: "
                              "this is not the reference the reads were mapped to")
        out[c] = sp
    return out


class RefGenome:
    """rmr_ref_genome_*: the contigs of a reference FASTA as nibbles on the device, loaded once and reused over several
    pileup_modbams calls.  ref_names / ref_lens: the BAM header's contigs, in its order; contig i of the table is contig i of
    the header."""

    n_open = 0  # tables alive in this process

    def __init__(self):
        raise TypeError("use RefGenome.from_fasta")

    @classmethod
    def from_fasta(cls, path, ref_names, ref_lens, device=None, contigs=None, piece_bytes=None):
        """Loads `contigs` (names or indices of ref_names; None: all) from the FASTA at `path`.  Refused before anything is
        allocated: a compressed file, a contig name twice in the file, a contig to load that the file lacks or has at
        another length.  Refused by the device's check while a contig is loaded, naming contig and line: a byte that is no
        IUPAC letter, lines of differing width.  FASTA contigs that are not asked for are skipped unread."""
        from . import _lib as L
        from .engine import get_engine

        path = os.fspath(path)
        ref_names, ref_lens = list(ref_names), [int(n) for n in ref_lens]
        want = list(range(len(ref_names))) if contigs is None else [c if isinstance(c, int) else ref_names.index(c) for c in contigs]
        piece = DEFAULT_PIECE_BYTES if piece_bytes is None else int(piece_bytes)
        if piece < 16:
            raise RemoraError(f"piece_bytes is at least 16, got {piece_bytes}")
        with open(path, "rb") as fh:
            if os.fstat(fh.fileno()).st_size == 0:
                raise RemoraError(f"{path} is not a FASTA file: it is empty")
            mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        self = object.__new__(cls)
        self.h, self._lib, self._L = ctypes.c_void_p(), L.lib(), L
        text = None
        try:
            spans = check_fasta_contigs(fasta_spans(mm, path), ref_names, ref_lens, want, path)
            self.path, self.ref_names, self.ref_lens, self.loaded = path, ref_names, ref_lens, sorted(spans)
            self.eng = get_engine(device)
            lens = np.zeros(max(len(ref_names), 1), np.int64)
            for c, sp in spans.items():
                lens[c] = sp.n_bases
            n_bytes = ctypes.c_int64(0)
            L.check(self._lib.rmr_ref_genome_create(self.eng.handle, len(ref_names), lens.ctypes.data_as(ctypes.c_void_p), ctypes.byref(self.h),
                                                    ctypes.byref(n_bytes)))
            RefGenome.n_open += 1
            self.device_bytes = int(n_bytes.value)
            text = np.frombuffer(mm, np.uint8)
            for c, sp in sorted(spans.items()):
                if sp.n_bases == 0:
                    continue
                bad = ctypes.c_int64(-1)
                rc = self._lib.rmr_ref_genome_load(self.h, c, text.ctypes.data + sp.start, sp.end - sp.start, sp.line_bases, sp.line_width, piece,
                                                   ctypes.byref(bad))
                if rc != 0 and bad.value >= 0:
                    at = sp.start + int(bad.value)
                    line = 1 + sum(int(np.count_nonzero(text[lo : min(lo + (1 << 26), at)] == 10)) for lo in range(0, at, 1 << 26))
                    col = int(bad.value) % sp.line_width
                    byte = int(text[at])
                    if col >= sp.line_bases:
                        what = f"the line does not end after {sp.line_bases} bases like the contig's first; {REWRAP}"
                    elif byte in (10, 13):
                        what = f"the line has {col} bases, the contig's first line has {sp.line_bases}; {REWRAP}"
                    else:
                        what = f"byte {byte} ({chr(byte)!r}) at column {col + 1} is not an IUPAC letter"
                    raise RemoraError(f"{path}: contig {sp.name}, line {line} (line {int(bad.value) // sp.line_width + 1} of its sequence): {what}")
                L.check(rc)
            LOGGER.info(f"reference: {len(spans)} contigs, {sum(s.n_bases for s in spans.values())} bases of {path} in "
                        f"{self.device_bytes / 2**20:.1f} MiB of device memory")
        except BaseException:
            self.close()
            raise
        finally:
            del text
            mm.close()
        return self

    def read(self, contig, lo=0, hi=None):
        """The codes of bases [lo, hi) of a loaded contig (name or index) -> u8 array, one code per base."""
        c = contig if isinstance(contig, int) else self.ref_names.index(contig)
        if c not in self.loaded:
            raise RemoraError(f"contig {self.ref_names[c]} was not loaded")
        hi = self.ref_lens[c] if hi is None else int(hi)
        out = np.zeros(max(hi - int(lo), 1), np.uint8)
        self._L.check(self._lib.rmr_ref_genome_read(self.h, c, int(lo), hi, out.ctypes.data_as(ctypes.c_void_p)))
        return out[: max(hi - int(lo), 0)]

    def close(self):
        if self.h:
            self._lib.rmr_ref_genome_destroy(self.h)
            self.h = ctypes.c_void_p()
            RefGenome.n_open -= 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _pileup_ref_struct(genome, descriptors, combine_strands):
    from . import _lib as L

    pr = L.PileupRef()
    pr.genome, pr.n_motifs, pr.combine = genome.h, len(descriptors), 1 if combine_strands else 0
    for j, d in enumerate(descriptors):
        pr.motifs[j].len, pr.motifs[j].focus, pr.motifs[j].mask, pr.motifs[j].rc_mask = d.length, d.focus, d.mask, d.rc_mask
    return pr


class DevicePileup:
    """rmr_pileup_*: the call buffer and the resident per-site table on the device."""

    def __init__(self, eng, n_contigs, max_contig_len, n_alpha, buffer_calls, ncol=None):
        """`ncol` (3 to 16, rmr_pileup_create_cols): the columns of a row when they are not the n_alpha + 1 of a plain table."""
        from . import _lib as L

        self._L, self._lib, self.eng, self.n_alpha = L, L.lib(), eng, int(n_alpha) if ncol is None else int(ncol) - 1
        self.h = ctypes.c_void_p()
        if ncol is None:
            L.check(self._lib.rmr_pileup_create(eng.handle, int(n_contigs), int(max_contig_len), int(n_alpha), int(buffer_calls), ctypes.byref(self.h)))
        else:
            L.check(self._lib.rmr_pileup_create_cols(eng.handle, int(n_contigs), int(max_contig_len), int(ncol), int(buffer_calls),
                                                     ctypes.byref(self.h)))

    def add(self, words, n):
        """n site words of a device tensor (kept alive by the caller until the engine's stream has passed them)."""
        self._L.check(self._lib.rmr_pileup_add(self.h, words.data_ptr(), int(n)))

    def finish(self):
        """(n_sites, n_calls, n_flushes, peak_device_bytes) after flushing what the buffer holds."""
        out = [ctypes.c_int64(0) for _ in range(4)]
        self._L.check(self._lib.rmr_pileup_finish(self.h, *[ctypes.byref(o) for o in out]))
        return tuple(int(o.value) for o in out)

    def read(self, n_sites):
        """keys u64[n_sites] (ref_id << 32 | pos << 1 | strand, ascending), counts u32[n_sites, n_alpha + 1]."""
        keys, counts = np.zeros(max(n_sites, 1), np.uint64), np.zeros((max(n_sites, 1), self.n_alpha + 1), np.uint32)
        self._L.check(self._lib.rmr_pileup_read(self.h, keys.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p)))
        return keys[:n_sites], counts[:n_sites]

    def set_canonical(self, base):
        """The canonical base of the table (rmr_pileup_set_canonical): what the coverage join tells N_nocall from N_diff by."""
        self._L.check(self._lib.rmr_pileup_set_canonical(self.h, ord(str(base))))

    def cover(self, b, pref, status, cig_q, cig_r, out_off, words, n_words, part=None, shift=0):
        """rmr_pileup_cover for one batch: device tensors of the emit of that batch (words may be None when n_words is 0), kept
        alive by the caller until the engine's stream has passed them."""
        self._L.check(self._lib.rmr_pileup_cover(self.h, ctypes.byref(b), None if pref is None else ctypes.byref(pref), status.data_ptr(),
                                                 cig_q.data_ptr(), cig_r.data_ptr(), out_off.data_ptr(), None if words is None else words.data_ptr(),
                                                 int(n_words), None if part is None else part.data_ptr(), int(shift)))

    def read_cover(self, n_sites):
        """u32[n_sites, 3]: N_delete, N_diff, N_nocall per site, in the order of read()'s keys."""
        cover = np.zeros((max(n_sites, 1), 3), np.uint32)
        self._L.check(self._lib.rmr_pileup_read_cover(self.h, cover.ctypes.data_as(ctypes.c_void_p)))
        return cover[:n_sites]

    def close(self):
        if self.h:
            self._lib.rmr_pileup_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _emit_batch(eng, b, opts, k_t, hist, n_cig, n_deltas, part=None, shift=0, cover=None):
    """One batch through the emit: the count pass (with the histogram when `hist` is a device tensor), and - k_t not None -
    the fill pass.  `opts`: the run's rmr_pileup_emit_opts (_lib.PileupEmitOpts).  `part` (i32 per record, a partitioned run): after the
    fill pass the records' partition ids are stamped into their words from bit `shift`.  With opts.hemi the fill keeps the
    strand bits and its words go through the pair passes (n_codes = n_mods + 2) - what comes back are the pair words.  `cover`
    (the DevicePileup of a finished table; the pass of `coverage`): the batch is joined against the table's sites,
    rmr_pileup_cover, while its workspaces are alive - also when it has no word.
    -> (words device tensor or None, calls per record, status per record, pairs in the batch or None)."""
    from . import _lib as L
    from .engine import _torch

    torch, lib, dev = _torch(), L.lib(), eng.torch_device
    n = int(b.n_records)
    n_codes, pref = int(b.n_mods) + 2 if opts.hemi else 0, opts.ref.contents if opts.ref else None
    ords = torch.empty(max(n_deltas, 1), dtype=torch.int32, device=dev)
    cig_qr = torch.empty((2, max(n_cig, 1)), dtype=torch.int64, device=dev)
    counts = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    d_status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    L.check(lib.rmr_pileup_emit_counts(eng.handle, ctypes.byref(b), ctypes.byref(opts), ords.data_ptr(), cig_qr[0].data_ptr(), cig_qr[1].data_ptr(),
                                       counts.data_ptr(), d_status.data_ptr(), hist.data_ptr() if hist is not None else None))
    eng.synchronize()
    h_counts, h_status = counts[:n].cpu().numpy(), d_status[:n].cpu().numpy()
    words, n_pairs = None, (0 if n_codes else None)
    total = int(h_counts.sum())
    if k_t is not None and total:
        out_off = np.zeros(n + 1, np.int64)
        np.cumsum(h_counts, out=out_off[1:])
        d_off = torch.from_numpy(out_off).to(dev)
        words = torch.empty(total, dtype=torch.int64, device=dev)
        L.check(lib.rmr_pileup_emit_fill(eng.handle, ctypes.byref(b), ctypes.byref(opts), int(k_t), ords.data_ptr(), cig_qr[0].data_ptr(),
                                         cig_qr[1].data_ptr(), d_status.data_ptr(), d_off.data_ptr(), words.data_ptr()))
        if part is not None:
            d_part = torch.from_numpy(np.ascontiguousarray(part, np.int32)).to(dev)
            L.check(lib.rmr_pileup_stamp_partition(eng.handle, n, d_off.data_ptr(), d_part.data_ptr(), int(shift), words.data_ptr(), total))
        if n_codes:  # the two strands' calls of a record at one site -> one pair word
            d_pairs = torch.empty(n, dtype=torch.int64, device=dev)
            L.check(lib.rmr_pileup_pair_counts(eng.handle, n, d_off.data_ptr(), words.data_ptr(), total, d_pairs.data_ptr()))
            eng.synchronize()
            pair_off = np.zeros(n + 1, np.int64)
            np.cumsum(d_pairs.cpu().numpy(), out=pair_off[1:])
            n_pairs = int(pair_off[-1])
            if not 0 <= 2 * n_pairs <= total:
                raise RemoraError(f"pileup: {n_pairs} pairs out of {total} calls")
            singles, words = words, None
            if n_pairs:
                d_pair_off = torch.from_numpy(pair_off).to(dev)
                words = torch.empty(n_pairs, dtype=torch.int64, device=dev)
                L.check(lib.rmr_pileup_pair_fill(eng.handle, n, d_off.data_ptr(), singles.data_ptr(), total, int(n_codes), d_pair_off.data_ptr(),
                                                 words.data_ptr()))
        if cover is not None:
            cover.cover(b, pref, d_status, cig_qr[0], cig_qr[1], d_off, words, total, d_part if part is not None else None, shift)
        eng.synchronize()  # the inputs and the workspaces may go once the kernel is through
    elif cover is not None and n:  # no word in the batch: its status-0 records still cover sites
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_part = None if part is None else torch.from_numpy(np.ascontiguousarray(part, np.int32)).to(dev)
        cover.cover(b, pref, d_status, cig_qr[0], cig_qr[1], d_off, None, 0, d_part, shift)
        eng.synchronize()
    return words, h_counts, h_status, n_pairs


def pileup_modbams(bams, alphabet, filter_threshold=None, pct_filt=DEFAULT_PCT_FILT, region=None, device=None, batch=512, buffer_calls=None,
                   device_gib=DEFAULT_DEVICE_GIB, ref=None, motifs=None, combine_strands=False, partition_tag=None, duplex=False, hemi=False,
                   coverage=False):
    """The per-site counts of the modified-base calls of `bams` (one path or several, piled into one table) -> PileupTable.
    `alphabet`: the canonical base followed by 1 to 7 single-letter modified-base codes.  The threshold: either
    `filter_threshold` T (k_T = ceil(512 T); give pct_filt=None with it) or `pct_filt` P - then a first pass over the input
    builds the histogram of the calls' confidence and k_T filters P percent of the calls, or fewer given ties.  `region`:
    "ctg" or "ctg:start-end", 0-based half-open.  `buffer_calls`: the capacity of the device call buffer in calls; by default
    what `device_gib` GiB (capped at half the free device memory) hold.
    `ref`: a reference FASTA path, or a RefGenome loaded before (reused, left open); with it `motifs`, 1 to 4 (motif, focus)
    whose focus base is the canonical base: a call is kept only where the reference shows one of them around its position (on
    '-' its reverse complement), and the percentile is taken over those calls.  Loaded are the header's contigs, with a region
    only the region's.  `combine_strands` (every motif its own reverse complement): a '-' call is written at the '+' position
    of its motif, one row per motif site; the region is asked of the position written.
    `partition_tag` (two characters, "HP" for phased reads): one table per value of that aux field in one run - a record
    belongs to the partition its tag names (an integer of type c C s S i I, or a character of type A), without the tag to
    `ungrouped`; which calls count, their classes and the threshold (one histogram, one k_T for the whole input) are those of
    the run without it, and the PileupTable has its three partition fields set (partition_tables, write_partitioned).  The
    id stands in the bits of a site word the contig index leaves free: 2^part_bits - 1 values, partition_bit_plan.
    `duplex`: the '-'-strand MM entries of duplex records (`G-m?` beside `C+m?`) count too; their calls lie on the reference
    strand opposite to the record's, and that strand is what the rows, the motif test and the fold see.  A position that
    entries of both strands list takes the strand of the last entry, in tag order, that lists it with a code of the alphabet.
    `hemi` (implies duplex; needs `ref`, one motif that is its own reverse complement, at most two modified bases, neither
    combine_strands nor partition_tag): one row per motif site with the counts of the strand pairs - the '+' call at rp and
    the '-' call at rp + (len - 1 - 2 focus) of ONE record are a pair of pattern (class on '+', class on '-'); a kept call
    without a partner in its record is counted in n_unpaired only.  The threshold is that of all kept single calls.
    `coverage` (not with duplex or hemi): once the table is finished the BAMs are streamed once more and every record that
    ended the emit with status 0 - also one none of whose calls was kept - is asked about every site of the table on its
    contig, on its strand, in its partition, whose position rp lies in its reference span.  The first rule that fits: the
    record has a kept call at the site (passing or fail): nothing, it is in the row; rp lies inside a D: N_delete + 1; rp lies
    inside M / = / X: the base of the original read there (U as T) is the canonical base: N_nocall + 1, anything else, N
    included: N_diff + 1; an N skip: nothing.  Only the positions an MM entry lists are calls, for `.` and `?` alike, and a
    position listed only with codes outside the alphabet is no call either: both are N_nocall.  With combine_strands a '+'
    record is asked at rp = S of a site S, a '-' record at S + (len - 1 - 2 focus) of the first motif, in the order given, that
    matches the reference at S.  The table, the threshold and the histogram are those of the run without it; the PileupTable
    has `coverage` set, and the writers print the eighteen-column bedMethyl.  12 bytes of device memory per site more.
    Everything that is refused is refused before any pileup launch; RemoraError when no call is kept.  (What a partition tag
    is refused for - another type, both kinds in one run, too many values - is known when the batch with that record is read:
    before any launch for that batch, and before any file is written.)"""
    bams = [bams] if isinstance(bams, (str, bytes)) or hasattr(bams, "__fspath__") else list(bams)
    if not bams:
        raise RemoraError("pileup_modbams needs at least one BAM")
    if coverage and (duplex or hemi):
        raise RemoraError(f"--coverage-columns with {'--hemi' if hemi else '--duplex'} is not built: there a record stands for two strands; "
                          "give one of them")
    if filter_threshold is not None and pct_filt is not None:
        raise RemoraError("give either --filter-threshold or --pct-filt, not both")
    if filter_threshold is None and pct_filt is None:
        pct_filt = DEFAULT_PCT_FILT
    alphabet = check_alphabet(alphabet)
    if hemi:
        check_hemi_arguments(ref, motifs, combine_strands, partition_tag, alphabet)
    duplex = bool(duplex or hemi)
    k_t = threshold_k(filter_threshold) if filter_threshold is not None else None
    if k_t is None:
        percentile_k([0] * N_BINS, pct_filt)  # the range check
    if ref is None and (motifs or combine_strands):
        raise RemoraError(("--motif" if motifs else "--combine-strands") + " needs --ref: the motif is looked up in the reference FASTA")
    if ref is not None and not motifs:
        raise RemoraError("--ref needs a motif: give --motif MOTIF FOCUS or --cpg")
    descriptors = check_pileup_motifs(motifs, alphabet[0], combine_strands or hemi) if ref is not None else None
    dicts = [bam_reference_dict(p) for p in bams]
    check_reference_dicts(bams, dicts)
    ref_names, ref_lens = [d[0] for d in dicts[0]], [d[1] for d in dicts[0]]
    check_site_fields(len(ref_names), max(ref_lens, default=0))
    parts = None if partition_tag is None else Partitioner(check_partition_tag(partition_tag), partition_bit_plan(len(ref_names), partition_tag))
    reg = parse_region(region, ref_names, ref_lens)
    if buffer_calls is not None and not 1 <= int(buffer_calls) < 2**31:
        raise RemoraError(f"buffer_calls is 1 to 2^31 - 1, got {buffer_calls}")
    if buffer_calls is None and not device_gib > 0:
        raise RemoraError("--pileup-device-gib must be positive")

    from . import _lib as L

    genome = None
    if isinstance(ref, RefGenome):
        genome = ref
        if not genome.h or genome.ref_names != ref_names or genome.ref_lens != [int(n) for n in ref_lens]:
            raise RemoraError(f"the RefGenome of {genome.path} is closed or was loaded for another reference dictionary than that of {bams[0]}")
        missing = [ref_names[c] for c in ([reg[0]] if reg[0] >= 0 else range(len(ref_names))) if c not in genome.loaded]
        if missing:
            raise RemoraError(f"the RefGenome of {genome.path} was loaded without contig {missing[0]}")
    elif ref is not None:  # refused here, before any pileup launch: what the FASTA lacks, and what the device finds wrong in it
        genome = RefGenome.from_fasta(ref, ref_names, ref_lens, device=device, contigs=[reg[0]] if reg[0] >= 0 else None)
    try:
        pref = None if genome is None else ctypes.pointer(_pileup_ref_struct(genome, descriptors, combine_strands or hemi))
        opts = L.PileupEmitOpts(region_ref=reg[0], region_lo=reg[1], region_hi=reg[2], ref=pref, duplex=int(duplex), hemi=int(bool(hemi)))
        return _pileup_run(PileupRun(bams, alphabet, k_t, pct_filt, region, ref_names, ref_lens, device, batch, buffer_calls, device_gib, genome,
                                     opts, bool(combine_strands or hemi), parts, bool(coverage)))
    finally:
        if genome is not None and genome is not ref:
            genome.close()


PileupRun = namedtuple("PileupRun", ("bams", "alphabet", "k_t", "pct_filt", "region", "ref_names", "ref_lens", "device", "batch", "buffer_calls",
                                     "device_gib", "genome", "opts", "combined", "parts", "coverage"))
PileupRun.__doc__ = """The checked arguments of one pileup_modbams run.  k_t: None when the threshold comes from pct_filt; region: the text, for
messages; opts: the rmr_pileup_emit_opts of every emit (the parsed region, the reference, duplex, hemi); parts: the Partitioner or None."""


def _one_pass(run, eng, warn, k_fill, hist, pile, log_skipped, cover=False):
    """All BAMs of `run` once: the count pass of every batch, and with k_fill the fill pass and the append - or, `cover`, the
    coverage join against the finished table of `pile` in place of the append.  -> (kept calls, pairs)."""
    from .io import _readahead, iter_bam_raw_batches
    from .validate import modbam_device_batch, tokenise_mod_tags, warn_ignored_entries

    parts, dev, mods = run.parts, eng.torch_device, run.alphabet[1:]
    n_kept = n_paired = n_asked = 0
    for path in run.bams:
        skipped, n_records = {}, 0

        def tokenised(path=path):  # the reader and the tokeniser of batch k + 1 run beside the GPU work of batch k
            for rb, _ in iter_bam_raw_batches(path, want_ref=False, batch=int(run.batch)):
                yield rb, tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off), (None if parts is None else
                                                                               read_aux_values(rb.raw, rb.raw_off, rb.tags_off, parts.tag))

        for rb, tok, aux in _readahead(tokenised(), depth=2):
            part = None if aux is None else parts.ids_of(rb, aux[0], aux[1], path)  # (in both passes: a refusal comes early)
            warn_ignored_entries(tok[4], run.alphabet, warn, MOD_NOT_IN_ALPHABET)
            buf, b = modbam_device_batch(dev, mods, rb.seq, rb.seq_off, rb.cigar, rb.cigar_off, rb.flag, rb.ref_id, rb.pos, rb.has, tok)
            b.n_refs = len(run.ref_names)
            words, h_counts, h_status, n_pairs = _emit_batch(eng, b, run.opts, k_fill, hist, int(np.asarray(rb.cigar).size), int(tok[5].size), part,
                                                               0 if parts is None else parts.plan.shift, pile if cover else None)
            n_paired += n_pairs or 0
            del buf
            if cover:  # a record adds at most 1 per site and column: 2^32 of them could pass a u32 count
                n_asked += int(np.count_nonzero(h_status == 0))
                if n_asked >= 2**32:
                    raise RemoraError(f"--coverage-columns: {n_asked} records take part, N_delete / N_diff / N_nocall are counted in 32 bits "
                                      "(fewer than 2^32 records)")
            elif words is not None:
                pile.add(words, words.numel())
                eng.synchronize()  # the words are in the call buffer (or the table) now
            n_kept += int(h_counts.sum())
            n_records += rb.n
            for st, k in zip(*np.unique(h_status, return_counts=True)):
                if st:
                    skipped[int(st)] = skipped.get(int(st), 0) + int(k)
        if log_skipped:
            for st, k in sorted(skipped.items()):
                LOGGER.info(f"{k} of {n_records} records skipped: {PILEUP_STATUS.get(st, st)} ({path})")
    return n_kept, n_paired


def _pileup_run(run):
    """pileup_modbams once its arguments are checked (`run`, a PileupRun) and the reference is on the device."""
    from .engine import _torch, get_engine

    alphabet, n_alpha, ref_names, parts, hemi = run.alphabet, len(run.alphabet), run.ref_names, run.parts, bool(run.opts.hemi)
    ncol = (n_alpha + 1) ** 2 if hemi else n_alpha + 1  # (hemi: a pair of classes of one strand's call - the alphabet and fail)
    torch, eng, buffer_calls = _torch(), get_engine(run.device), run.buffer_calls
    if buffer_calls is None:
        free = torch.cuda.mem_get_info(eng.torch_device)[0]
        gib = min(float(run.device_gib), free / 2 / 2**30)
        buffer_calls = int(max(1, min(2**31 - 1, (gib * 2**30 - (1 << 20)) // bytes_per_buffered_call(ncol - 1))))
        LOGGER.info(f"pileup call buffer: {buffer_calls} calls in {gib:.3g} GiB of device memory (--pileup-device-gib {run.device_gib:g}, "
                    f"{free / 2**30:.1f} GiB free)")
    one_pass = partial(_one_pass, run, eng, {"strand": not run.opts.duplex, "mod": True})  # (a duplex run counts the '-' entries: no warning)
    no_calls = (f"No modified-base call of {alphabet[1:]} on an aligned base" + (f" inside {run.region}" if run.region is not None else "") +
                (" on a motif of the reference" if run.genome is not None else "") +
                f" in {', '.join(map(str, run.bams))}.")
    h_hist, k_t = None, run.k_t
    if k_t is None:  # the percentile needs every call's confidence first: one pass that emits no rows
        hist = torch.zeros(N_BINS, dtype=torch.int64, device=eng.torch_device)
        n_kept, _ = one_pass(None, hist, None, True)
        eng.synchronize()
        h_hist = hist.cpu().numpy()
        if n_kept < 1 or int(h_hist.sum()) != n_kept:
            if n_kept < 1:
                raise RemoraError(no_calls)
            raise RemoraError(f"pileup: the histogram holds {int(h_hist.sum())} calls, the records {n_kept}")
        k_t = percentile_k(h_hist, run.pct_filt)
        LOGGER.info(f"--pct-filt {run.pct_filt:g}: {int(h_hist[:k_t].sum())} of {n_kept} calls fail at k_T = {k_t} (probability {k_t / 512:.6g})")
    # a partitioned run: the id stands above the contig index, and the sort covers its bits too
    with DevicePileup(eng, len(ref_names) if parts is None else parts.plan.n_contigs, max(run.ref_lens), n_alpha, buffer_calls,
                      ncol if hemi else None) as pile:
        n_kept, n_paired = one_pass(k_t, None, pile, h_hist is None)
        n_sites, n_calls, n_flushes, peak = _finish(pile, ref_names, parts)
        if hemi and n_kept >= 1 and n_paired < 1:
            raise RemoraError(f"{n_kept} modified-base calls are kept, none of them has a partner on the other strand in its record: "
                              "--hemi counts the strand pairs of duplex records (C+m? with G-m?)")
        if n_calls < 1:
            raise RemoraError(no_calls)
        if n_calls != (n_paired if hemi else n_kept):
            raise RemoraError(f"pileup: {n_calls} calls reached the table, the records hold {n_paired if hemi else n_kept}")
        keys, counts = pile.read(n_sites)
        cover = None
        if run.coverage:  # the third pass: the same emit with the final k_T and no histogram, joined against the finished table
            pile.set_canonical(alphabet[0])
            n_again, _ = one_pass(k_t, None, pile, False, cover=True)
            if n_again != n_kept:
                raise RemoraError(f"pileup: the coverage pass kept {n_again} calls, the pass before it {n_kept}: the input changed between them")
            peak = pile.finish()[3]  # (nothing to flush: the peak with the coverage counts in it)
            cover = pile.read_cover(n_sites).astype(np.int64)
            LOGGER.info(f"--coverage-columns: N_delete {int(cover[:, 0].sum())}, N_diff {int(cover[:, 1].sum())}, N_nocall "
                        f"{int(cover[:, 2].sum())} on {n_sites} sites")
    if run.genome is not None:
        peak += run.genome.device_bytes
    if hemi:
        LOGGER.info(f"{n_calls} strand pairs on {n_sites} sites, {n_kept - 2 * n_calls} of {n_kept} calls unpaired; {n_flushes} flushes, "
                    f"{peak / 2**20:.1f} MiB of device memory at the peak")
    else:
        LOGGER.info(f"{n_calls} calls on {n_sites} sites; {n_flushes} flushes, {peak / 2**20:.1f} MiB of device memory at the peak")
    table = PileupTable(ref_names=ref_names, ref_id=(keys >> np.uint64(32)).astype(np.int32),
                        pos=((keys >> np.uint64(1)) & np.uint64(0x7FFFFFFF)).astype(np.int64), strand=(keys & np.uint64(1)).astype(np.uint8),
                        counts=counts.astype(np.int64), alphabet=alphabet, threshold_k=int(k_t), n_calls=n_calls, n_flushes=n_flushes,
                        peak_device_bytes=peak, hist=None if h_hist is None else h_hist.astype(np.int64), combined=run.combined,
                        hemi=hemi, n_unpaired=n_kept - 2 * n_calls if hemi else None, coverage=cover)
    return table if parts is None else _partitioned(table, parts)


def _partitioned(table, parts):
    """The table as it was read, its ref_id holding id << contig_bits | ref_id and its rows ordered by (id, site) -> the
    partitioned table: the ids mapped to the labels that have rows, the blocks stably re-ordered into label order."""
    cb = parts.plan.contig_bits
    ids = (table.ref_id >> cb).astype(np.int64)
    key_of_id = parts.key_of_id()
    present = np.unique(ids).tolist()
    by_key = {_UNGROUPED_KEY if key_of_id[i] is None else key_of_id[i]: i for i in present}
    ordered = partition_order(by_key)
    rank = np.zeros(max(present) + 1, np.int32)
    for k, key in enumerate(ordered):
        rank[by_key[key]] = k
    partition = rank[ids]
    order = np.argsort(partition, kind="stable")
    rows = table._replace(ref_id=(table.ref_id & np.int32((1 << cb) - 1))[order], pos=table.pos[order], strand=table.strand[order],
                          counts=table.counts[order])
    return PileupTable(*rows, partition=partition[order], partition_labels=[partition_label(k) for k in ordered], partition_tag=parts.tag,
                       coverage=None if table.coverage is None else table.coverage[order])


def _finish(pile, ref_names, parts=None):
    try:
        return pile.finish()
    except RemoraError as e:  # the refusal of a count beyond 32 bits names the site by its contig index: add the name
        m = re.search(r"contig #(\d+)", str(e))
        if m and parts is not None:  # the index read there holds the partition id above the contig's
            rid, pid = int(m.group(1)) & ((1 << parts.plan.contig_bits) - 1), int(m.group(1)) >> parts.plan.contig_bits
            key = parts.key_of_id().get(pid, None)
            if rid < len(ref_names):
                text = str(e).replace(m.group(0), f"contig #{rid}")
                raise RemoraError(f"{text} ({ref_names[rid]}, {parts.tag} {partition_label(_UNGROUPED_KEY if key is None else key)})")
        elif m and int(m.group(1)) < len(ref_names):
            raise RemoraError(f"{e} ({ref_names[int(m.group(1))]})")
        raise


def write_bedmethyl(table, path, min_coverage=1):
    """The eleven ENCODE bedMethyl columns, header-less, tab-separated: one row per (site, modified base) whose N_valid - the
    passing calls of any class - is at least max(min_coverage, 1):
    chrom pos pos+1 code min(N_valid, 1000) strand pos pos+1 255,0,0 N_valid pct, pct = 100 N_mod / N_valid to two decimals.
    Rows: contigs in header order, then position, then + before -, then the codes in alphabet order.  Returns the rows written.
    A hemi table: per site whose N_valid - the pairs whose two classes both pass - reaches the coverage, one row per pattern of
    passing classes, (n_mods + 1)^2 rows ordered by the '+' class, then the '-' class; the name column is `<a>,<b>,<canonical>`
    (a modified base's code, `-` for the canonical class: m,m,C  m,-,C  -,m,C  -,-,C), the strand column `.`, pct = 100
    N_pattern / N_valid.
    A table with `coverage`: eighteen columns, all tab-separated - the eleven, then N_mod N_canonical N_other_mod N_delete
    N_fail N_diff N_nocall, N_other_mod = N_valid - N_mod - N_canonical of that row's code; the same rows."""
    if getattr(table, "hemi", False):
        return _write_bedmethyl_hemi(table, path, min_coverage)
    mods = list(table.alphabet[1:])
    combined = bool(getattr(table, "combined", False))
    coverage = getattr(table, "coverage", None)
    valid = table.counts[:, :-1].sum(axis=1)
    keep = np.nonzero(valid >= max(int(min_coverage), 1))[0]
    n_rows = 0
    with open(path, "w") as fh:
        for lo in range(0, keep.size, 65536):
            lines = []
            idx = keep[lo : lo + 65536]
            cover = [None] * idx.size if coverage is None else coverage[idx].tolist()
            for rid, pos, st, nv, row, cov in zip(table.ref_id[idx].tolist(), table.pos[idx].tolist(), table.strand[idx].tolist(),
                                                  valid[idx].tolist(), table.counts[idx].tolist(), cover):
                name, sc = table.ref_names[rid], "." if combined else "-" if st else "+"
                for j, code in enumerate(mods):
                    more = "" if cov is None else f"\t{row[1 + j]}\t{row[0]}\t{nv - row[1 + j] - row[0]}\t{cov[0]}\t{row[-1]}\t{cov[1]}\t{cov[2]}"
                    lines.append(f"{name}\t{pos}\t{pos + 1}\t{code}\t{min(nv, 1000)}\t{sc}\t{pos}\t{pos + 1}\t255,0,0\t{nv}\t"
                                 f"{100 * row[1 + j] / nv:.2f}{more}\n")
            fh.write("".join(lines))
            n_rows += len(lines)
    return n_rows


def _write_bedmethyl_hemi(table, path, min_coverage):
    n_alpha = len(table.alphabet)
    nc = n_alpha + 1
    names = ["-"] + list(table.alphabet[1:])
    cols = [(a * nc + b, f"{names[a]},{names[b]},{table.alphabet[0]}") for a in range(n_alpha) for b in range(n_alpha)]
    valid = table.counts[:, [c for c, _ in cols]].sum(axis=1)
    keep = np.nonzero(valid >= max(int(min_coverage), 1))[0]
    n_rows = 0
    with open(path, "w") as fh:
        for lo in range(0, keep.size, 65536):
            lines = []
            idx = keep[lo : lo + 65536]
            for rid, pos, nv, row in zip(table.ref_id[idx].tolist(), table.pos[idx].tolist(), valid[idx].tolist(), table.counts[idx].tolist()):
                name = table.ref_names[rid]
                for c, label in cols:
                    lines.append(f"{name}\t{pos}\t{pos + 1}\t{label}\t{min(nv, 1000)}\t.\t{pos}\t{pos + 1}\t255,0,0\t{nv}\t{100 * row[c] / nv:.2f}\n")
            fh.write("".join(lines))
            n_rows += len(lines)
    return n_rows


def write_counts(table, path):
    """TSV with the header chrom start strand N_<canonical> N_<code>... N_fail: one row per site that has a kept call.  A hemi
    table: N_<a>_<b> for all (n_mods + 2)^2 pattern codes in code order, the classes named by the canonical base's letter, the
    modified bases' codes and `fail`; one row per site that has a pair.  A table with `coverage`: N_delete N_diff N_nocall behind
    N_fail."""
    if getattr(table, "hemi", False):
        cls = hemi_class_names(table.alphabet)
        with open(path, "w") as fh:
            fh.write("\t".join(["chrom", "start", "strand"] + [f"N_{a}_{b}" for a in cls for b in cls]) + "\n")
            for lo in range(0, table.pos.size, 65536):
                sl = slice(lo, lo + 65536)
                fh.write("".join(f"{table.ref_names[rid]}\t{pos}\t.\t" + "\t".join(map(str, row)) + "\n"
                                 for rid, pos, row in zip(table.ref_id[sl].tolist(), table.pos[sl].tolist(), table.counts[sl].tolist())))
        return int(table.pos.size)
    combined = bool(getattr(table, "combined", False))
    coverage = getattr(table, "coverage", None)
    with open(path, "w") as fh:
        fh.write("\t".join(["chrom", "start", "strand"] + [f"N_{a}" for a in table.alphabet] + ["N_fail"] +
                           ([] if coverage is None else ["N_delete", "N_diff", "N_nocall"])) + "\n")
        for lo in range(0, table.pos.size, 65536):
            sl = slice(lo, lo + 65536)
            rows = table.counts[sl].tolist() if coverage is None else np.concatenate([table.counts[sl], coverage[sl]], axis=1).tolist()
            fh.write("".join(f"{table.ref_names[rid]}\t{pos}\t{'.' if combined else '-' if st else '+'}\t" + "\t".join(map(str, row)) + "\n"
                             for rid, pos, st, row in zip(table.ref_id[sl].tolist(), table.pos[sl].tolist(), table.strand[sl].tolist(), rows)))
    return int(table.pos.size)


# ---- a partitioned table: splitting and writing ------------------------------------------------------------------------
def partition_tables(table):
    """A partitioned table -> {label: PileupTable} in label order, each a plain table of that partition's rows: n_calls the
    sum of its counts (the fail column included); threshold_k and hist the whole run's - the threshold is the sample's."""
    if table.partition is None or table.partition_labels is None:
        raise RemoraError("partition_tables takes the table of a run with a partition tag")
    out = {}
    for k, label in enumerate(table.partition_labels):
        rows = np.nonzero(table.partition == k)[0]
        out[label] = table._replace(ref_id=table.ref_id[rows], pos=table.pos[rows], strand=table.strand[rows], counts=table.counts[rows],
                                    n_calls=int(table.counts[rows].sum()))  # (a plain table: _replace leaves the partition attributes behind)
        out[label].coverage = None if table.coverage is None else table.coverage[rows]
    return out


def partition_file_name(path, tag, label):
    """The file of one partition: `.<tag>_<label>` - `.ungrouped` for that partition - before the last extension of `path`, or
    at its end when it has none: s.bed -> s.HP_1.bed, s.ungrouped.bed.  A character label outside [0-9A-Za-z] is written xHH,
    its code in hexadecimal."""
    label = str(label)
    if label == UNGROUPED:
        insert = "." + UNGROUPED
    else:
        if len(label) == 1 and re.fullmatch(r"[0-9A-Za-z]", label) is None:  # (an integer label of one character is a digit)
            label = f"x{ord(label):02X}"
        insert = f".{tag}_{label}"
    root, ext = os.path.splitext(os.fspath(path))
    return root + insert + ext


def write_partitioned(table, out_bed, counts_path=None, min_coverage=1):
    """write_bedmethyl - and with `counts_path` write_counts - once per label that has a row, into the files
    partition_file_name makes of the two paths.  -> {label: bedMethyl rows written}."""
    tag = table.partition_tag
    if tag is None:
        raise RemoraError("write_partitioned takes the table of a run with a partition tag")
    rows = {}
    for label, sub in partition_tables(table).items():
        if sub.pos.size == 0:
            continue
        rows[label] = write_bedmethyl(sub, partition_file_name(out_bed, tag, label), min_coverage=min_coverage)
        if counts_path is not None:
            write_counts(sub, partition_file_name(counts_path, tag, label))
    return rows
