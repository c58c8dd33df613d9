"""Simplex-to-duplex alignment (src/remora/duplex_utils.py): where the reference calls parasail on the CPU for one pair
at a time, a batch of alignments runs on the GPU (rmr_duplex_align_mode, csrc/k_duplex.hip).  The alignment, its scores and the
rule among co-optimal paths: include/remora_hip.h and DESIGN.md, "Duplex"."""
import ctypes
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np

from . import RemoraError
from . import _lib as L
from . import data_chunks as DC

CigarTuples = List[Tuple[int, int]]

# ---- the constants block of include/remora_hip.h (tests/test_host_duplex.py holds the two together) ----
MATCH, MISMATCH, N_BASE, N_N = 5, -4, -2, -1
GAP_OPEN, GAP_EXTEND = 10, 2  # a gap of k bases costs GAP_OPEN + GAP_EXTEND * (k - 1)
ROWS_PER_LANE = 8
STRIP_ROWS = 64 * ROWS_PER_LANE  # simplex rows one sweep of the kernel covers
DEFAULT_TRACE_BYTES = 1 << 34  # 16 GiB of trace (4 bits per DP cell) alive at a time; more alignments run in more groups
OUT_FIELDS = 8
STATUS_OK, STATUS_NO_MATCH, STATUS_BAD_BASE, STATUS_OVER_BUDGET, STATUS_EMPTY = range(5)
STATUS_MESSAGE = {
    STATUS_NO_MATCH: "failed to find match operations in pairwise alignment",
    STATUS_BAD_BASE: "duplex alignment of a sequence with a base other than A, C, G, T or N",
    STATUS_OVER_BUDGET: "duplex alignment exceeds the trace budget",
    STATUS_EMPTY: "duplex alignment of an empty sequence",
}


# how the walk back gets its trace (rmr_duplex_align_mode): stored for every cell, recomputed strip by strip from one kept DP line
# per strip, or the first where the whole call fits the budget as one group and the second otherwise.  Same results in all three.
MODE_FULL, MODE_CHECKPOINT, MODE_AUTO = range(3)
MODES = {"full": MODE_FULL, "checkpoint": MODE_CHECKPOINT, "auto": MODE_AUTO}


def trace_bytes(simplex_len, duplex_len):
    """Bytes of trace one alignment takes (include/remora_hip.h)."""
    return -(-simplex_len // STRIP_ROWS) * (duplex_len + 63) * 256


def checkpoint_bytes(simplex_len, duplex_len):
    """Bytes one alignment takes in checkpointed memory: a line of duplex_len (H, F) pairs per strip and one strip of trace."""
    return -(-simplex_len // STRIP_ROWS) * duplex_len * 8 + (duplex_len + 63) * 256


@dataclass
class PairwiseAlignment:
    ref_start: int
    ref_end: int
    query_start: int
    query_end: int
    cigar: CigarTuples


@dataclass
class SimplexDuplexMapping:
    duplex_to_simplex_mapping: np.ndarray
    trimmed_duplex_seq: str
    duplex_offset: int


@dataclass
class AlignmentBatch:
    """What rmr_duplex_align returns for a batch: per alignment its status, score, end row (simplex bases consumed),
    query_start, ref_start, ref_end, and its runs (ops, lengths) with M = 0, I = 1, D = 2; the number of groups the trace
    budget made and the number of alignments that ran in checkpointed memory."""
    status: np.ndarray
    score: np.ndarray
    end_row: np.ndarray
    query_start: np.ndarray
    ref_start: np.ndarray
    ref_end: np.ndarray
    run_off: np.ndarray  # i64[n + 1]: the runs of alignment a are words[run_off[a] : run_off[a] + n_runs[a]]
    n_runs: np.ndarray
    words: np.ndarray
    n_groups: int
    n_checkpointed: int = 0

    def runs(self, a):
        w = self.words[self.run_off[a]:self.run_off[a] + self.n_runs[a]]
        return (w & 15).astype(np.int64), (w >> 4).astype(np.int64)

    def pairwise_alignment(self, a):
        ops, lens = self.runs(a)
        qlen = int(lens[ops != 2].sum())
        return PairwiseAlignment(ref_start=int(self.ref_start[a]), ref_end=int(self.ref_end[a]), query_start=int(self.query_start[a]),
                                 query_end=int(self.query_start[a]) + qlen, cigar=list(zip(ops.tolist(), lens.tolist())))


def align_batch(pairs, engine=None, trace_budget=None, mode="full"):
    """Align every (simplex_seq, duplex_seq) of `pairs` in one call (upper-cased here).  No status raises: the caller decides.
    `mode`: "full", "checkpoint" or "auto" (MODES); it changes the memory the call takes, never a result."""
    from .engine import get_engine

    n = len(pairs)
    eng = engine if engine is not None else get_engine()
    seqs = [s.upper().encode("ascii", "replace") for p in pairs for s in p]
    lens = np.array([len(s) for s in seqs], np.int64)
    off = np.zeros(2 * n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    bases = np.frombuffer(b"".join(seqs) + b"\0", np.uint8)
    q_off, r_off = np.ascontiguousarray(off[0:2 * n:2]), np.ascontiguousarray(off[1:2 * n:2])
    q_len, r_len = np.ascontiguousarray(lens[0::2]), np.ascontiguousarray(lens[1::2])
    run_off = np.zeros(n + 1, np.int64)
    np.cumsum(2 * r_len + 2, out=run_off[1:])
    out = np.zeros((n, OUT_FIELDS), np.int32)
    words = np.zeros(int(run_off[-1]), np.uint32)
    if mode not in MODES:
        raise RemoraError(f"unknown duplex alignment mode {mode!r} (one of {', '.join(MODES)})")
    groups, checkpointed = ctypes.c_int64(0), ctypes.c_int64(0)
    if n:
        L.check(L.lib().rmr_duplex_align_mode(eng.handle, n, bases.ctypes.data, q_off.ctypes.data, q_len.ctypes.data, r_off.ctypes.data,
                                              r_len.ctypes.data, int(trace_budget or 0), MODES[mode], out.ctypes.data,
                                              run_off.ctypes.data, words.ctypes.data, ctypes.byref(groups), ctypes.byref(checkpointed)))
    return AlignmentBatch(status=out[:, 0].copy(), score=out[:, 1].copy(), end_row=out[:, 2].copy(), query_start=out[:, 3].copy(),
                          ref_start=out[:, 4].copy(), ref_end=out[:, 5].copy(), run_off=run_off, n_runs=out[:, 6].astype(np.int64),
                          words=words, n_groups=int(groups.value), n_checkpointed=int(checkpointed.value))


def mapping_from_alignment(pairwise_alignment, duplex_seq):
    """src/remora/duplex_utils.py:98-115 from the trimmed alignment on: the simplex coordinate of every trimmed duplex
    position (np.interp in float64 across the gaps, truncated) and the trimmed duplex sequence."""
    pa = pairwise_alignment
    cigar = pa.cigar
    if isinstance(cigar, list):
        cigar = (np.array([c[0] for c in cigar], np.int64), np.array([c[1] for c in cigar], np.int64))
    mapping = DC.make_sequence_coordinate_mapping(cigar).astype(int) + pa.query_start
    return SimplexDuplexMapping(duplex_to_simplex_mapping=mapping, trimmed_duplex_seq=duplex_seq[pa.ref_start:pa.ref_end],
                                duplex_offset=pa.ref_start)


def map_simplexes_to_duplexes(pairs, engine=None, trace_budget=None, mode="full"):
    """The batch form of map_simplex_to_duplex: one rmr_duplex_align_mode call for every (simplex_seq, duplex_seq) of `pairs`.
    Returns a list with a SimplexDuplexMapping per pair, or the error text (str) of a pair that has none."""
    res = align_batch(pairs, engine, trace_budget, mode)
    out = []
    for a, (_, duplex_seq) in enumerate(pairs):
        st = int(res.status[a])
        if st != STATUS_OK:
            out.append(STATUS_MESSAGE.get(st, f"duplex alignment failed with status {st}"))
            continue
        ops, lens = res.runs(a)
        pa = PairwiseAlignment(int(res.ref_start[a]), int(res.ref_end[a]), int(res.query_start[a]), 0, (ops, lens))
        out.append(mapping_from_alignment(pa, duplex_seq))
    return out


def map_simplex_to_duplex(*, simplex_seq: str, duplex_seq: str):
    """src/remora/duplex_utils.py:98-115 (a batch of one).  RuntimeError where the alignment holds no match operation, as in
    the reference; RemoraError for what parasail has no word for (an unsupported letter, the trace budget)."""
    res = map_simplexes_to_duplexes([(simplex_seq, duplex_seq)])[0]
    if isinstance(res, str):
        if res == STATUS_MESSAGE[STATUS_NO_MATCH]:
            raise RuntimeError(res)
        raise RemoraError(res)
    return res
