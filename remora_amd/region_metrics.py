"""The region API of the reference's io module (src/remora/io.py:579-922): which reads cover a reference region, their per-base
metrics there and their signal - what the reference's notebooks and `analyze plot ref_region` draw from.  io.py exports these
names; drawing itself stays out.

Three layers:
  - plan_region_pairs: host arithmetic that joins reference spans of reads with regions into (read, region) pairs;
  - device_region_metrics / device_region_signals (DeviceReads.region_metrics / region_signals): one launch each of
    rmr_region_base_metrics / rmr_region_signals (csrc/k_metrics.hip) for the pairs of a resident batch;
  - the pass (_region_pass): every BAM streamed once for all regions of a call, the covering records picked from the raw batches'
    fixed fields before any signal is decoded, the picked records through the batch ingest (io._ingest_batch, reference-anchored),
    refined on the device as Read.set_refine_signal_mapping(refiner, ref_mapping=True) does, then the two kernels.  Batches the
    array ingest or the resident refiner does not cover go read by read through the same kernels.
The per-read host forms are io.Read.extract_ref_reg / extract_basecall_region / compute_per_base_metric(region=)."""
import ctypes
import dataclasses
import random

import numpy as np

from . import RemoraError
from . import _lib as L

PAIR_WORDS = 8  # int64 per pair on the device: read, first, last, lead, row, region length, flip, spare (csrc/k_metrics.hip)


# ---------------------------------------------------------------------------------------
# host helpers under the reference's names
# ---------------------------------------------------------------------------------------
def strands_match(strand, bam_read):
    """src/remora/io.py:157-164: a region without a strand (or with anything but + / -) matches both."""
    if strand is None:
        return True
    return strand not in "+-" or (strand == "+" and not bam_read.is_reverse) or (strand == "-" and bam_read.is_reverse)


def compute_base_space_sig_coords(seq_to_sig_map):
    """A coordinate in base space for every sample, linear inside each base (src/remora/io.py:579-587)."""
    return np.interp(np.arange(seq_to_sig_map[-1] - seq_to_sig_map[0]), seq_to_sig_map, np.arange(seq_to_sig_map.size))


@dataclasses.dataclass
class ReadRefReg:
    """The part of a read inside a reference region, on the reference's strand (src/remora/io.py:590-607; no plot methods)."""

    read_id: str
    norm_signal: np.ndarray
    seq: str
    seq_to_sig_map: np.ndarray
    ref_reg: object
    sig_start: int = 0

    @property
    def ref_sig_coords(self):
        return compute_base_space_sig_coords(self.seq_to_sig_map) + self.ref_reg.start


@dataclasses.dataclass
class ReadBasecallRegion:
    """A stretch of a read in basecall coordinates (src/remora/io.py:637-644; no plot methods)."""

    read_id: str
    norm_signal: np.ndarray
    seq: str
    seq_to_sig_map: np.ndarray
    start: int
    sig_start: int = 0


# indexed by a base code; numpy counts a negative index from the end, so -1 (N) reads the last entry and -2 (not covered) the one
# before it: both stay what they are
_NP_COMP = np.array([3, 2, 1, 0, -2, -1], np.int32)


def get_ref_int_seq_from_reads(ref_reg, bam_reads, ref_orient=True):
    """The region's bases (int32: 0-3, -1 = N, -2 = no read covers the position) from the reference sequences of the records
    (src/remora/io.py:671-695)."""
    from .util import seq_to_int

    int_seq = np.full(ref_reg.len, -2, np.int32)
    for bam_read in bam_reads:
        read_ref_seq = bam_read.get_reference_sequence().upper()
        int_seq[max(0, bam_read.reference_start - ref_reg.start) : bam_read.reference_end - ref_reg.start] = seq_to_int(
            read_ref_seq[max(0, ref_reg.start - bam_read.reference_start) : ref_reg.end - bam_read.reference_start])
        if not np.any(int_seq == -2):
            break
    if ref_reg.strand == "-":
        return _NP_COMP[int_seq] if ref_orient else _NP_COMP[int_seq][::-1]
    return int_seq


def get_ref_seq_from_reads(ref_reg, bam_reads, ref_orient=True):
    """The same as a string, N where nobody covers (src/remora/io.py:698-703)."""
    from .util import int_to_seq

    int_seq = get_ref_int_seq_from_reads(ref_reg, bam_reads, ref_orient=ref_orient)
    int_seq[np.equal(int_seq, -2)] = -1
    return int_to_seq(int_seq)


def get_ref_seq_and_levels_from_reads(ref_reg, bam_reads, sig_map_refiner, ref_orient=True):
    """(sequence, expected level of every position or None without a refiner), src/remora/io.py:706-765.  One difference: the
    reference looks its level table up with whatever a k-mer holding a -1 / -2 base computes (bounds checks off: undefined); here
    a position whose k-mer holds a base that is not covered or not ACGT gets NaN."""
    from .util import int_to_seq

    if sig_map_refiner is None:
        levels = None
        ctx = get_ref_int_seq_from_reads(ref_reg, bam_reads, ref_orient=False)
        ctx[np.equal(ctx, -2)] = -1
        seq = int_to_seq(ctx)
    else:
        kb, ka = int(sig_map_refiner.bases_before), int(sig_map_refiner.bases_after)
        ctx = get_ref_int_seq_from_reads(ref_reg.adjust(-kb, ka, ref_orient=False), bam_reads, ref_orient=False)
        known = ctx >= 0
        levels = np.asarray(sig_map_refiner.extract_levels(np.where(known, ctx, 0))).copy()
        bad = np.concatenate([[0], np.cumsum(~known)])  # positions whose whole k-mer is known: no unknown base in [i - kb, i + ka]
        whole = np.zeros(ctx.size, bool)
        if ctx.size >= kb + ka + 1:
            whole[kb : ctx.size - ka] = bad[kb + ka + 1 :] - bad[: ctx.size - kb - ka] == 0
        levels[~whole] = np.nan
        ctx[np.equal(ctx, -2)] = -1
        seq = int_to_seq(ctx)[kb : kb + ref_reg.len]
        levels = levels[kb : kb + ref_reg.len]
    if ref_reg.strand == "-" and ref_orient:
        seq = seq[::-1]
        if levels is not None:
            levels = levels[::-1]
    return seq, levels


# ---------------------------------------------------------------------------------------
# the host plan
# ---------------------------------------------------------------------------------------
def _span_in_read(ref_start, ref_len, is_rev, reg_start, reg_end, extract):
    """(first, last, lead) of a region inside reads, read-oriented (scalars or arrays): the strand decides which end of the
    alignment the read's first base lies on.  Read.compute_per_base_metric (:2448-2460) clips both ends and counts the region
    positions in front of the read (`lead`); Read.extract_ref_reg (:2359-2366) clips the start, and python's slice clips the end."""
    st = np.where(is_rev, ref_start + ref_len - reg_end, reg_start - ref_start)
    first, last = np.maximum(st, 0), np.minimum(st + (reg_end - reg_start), ref_len)
    return first, last, (np.zeros_like(first) if extract else np.maximum(-st, 0))


def plan_region_pairs(regions, ref_names, ref_id, ref_start, ref_len, flag, ref_orient=True, extract=False):
    """Joins reads with regions.  `regions`: RefRegion objects; `ref_names`: contig name per reference index of the BAM; per
    read `ref_id`, `ref_start`, `ref_len` (reference positions its alignment spans) and `flag`.  A read belongs to a region as
    the reference's get_reg_bam_reads selects it (src/remora/io.py:540-549): primary, mapped to the region's contig, on its
    strand (both when the region has none), and overlapping as fetch defines it: start < region.end and end > region.start.
    -> dict of int64 arrays, one entry per pair, ordered by (region, read): `region`, `read`, `first`, `last` (bases [first,
    last) of the read in read orientation), `lead` (region positions in front of the read's first base), `row` (the pair's
    number inside its region), `rlen`, `flip`.
    The arithmetic is Read.compute_per_base_metric's (:2448-2460) or, with `extract`, Read.extract_ref_reg's (:2359-2366): there
    `lead` is 0, the mapping entries first .. last (inclusive) are what is kept, and reverse-strand pairs are always flipped,
    where the metrics flip them only for `ref_orient`."""
    ref_id, ref_start, ref_len, flag = (np.asarray(x, np.int64) for x in (ref_id, ref_start, ref_len, flag))
    ref_end = ref_start + ref_len
    is_rev = (flag & 16) != 0
    usable = ((flag & 0x900) == 0) & ((flag & 4) == 0) & (ref_id >= 0) & (ref_len > 0)
    name_to_id = {}
    for i, name in enumerate(ref_names):
        name_to_id.setdefault(name, i)
    cols = {k: [] for k in ("region", "read", "first", "last", "lead", "row", "rlen", "flip")}
    for r, reg in enumerate(regions):
        rid = name_to_id.get(reg.ctg)
        if rid is None:
            continue
        end = reg.start + 1 if reg.end is None else reg.end
        hit = usable & (ref_id == rid) & (ref_start < end) & (ref_end > reg.start)
        if reg.strand is not None and reg.strand in "+-":
            hit &= is_rev == (reg.strand == "-")
        idx = np.nonzero(hit)[0]
        if not idx.size:
            continue
        rev = is_rev[idx]
        first, last, lead = _span_in_read(ref_start[idx], ref_len[idx], rev, reg.start, end, extract)
        cols["region"].append(np.full(idx.size, r, np.int64))
        cols["read"].append(idx)
        cols["first"].append(first)
        cols["last"].append(last)
        cols["lead"].append(lead)
        cols["row"].append(np.arange(idx.size, dtype=np.int64))
        cols["rlen"].append(np.full(idx.size, end - reg.start, np.int64))
        cols["flip"].append((rev & (bool(ref_orient) or bool(extract))).astype(np.int64))
    return {k: (np.concatenate(v) if v else np.zeros(0, np.int64)) for k, v in cols.items()}


def _ref_lens_of_batch(rb):
    """Reference positions every record of a raw BAM batch spans, from its CIGAR (M, D, N, =, X)."""
    ops, lens = (rb.cigar & 0xF).astype(np.int64), (rb.cigar >> 4).astype(np.int64)
    consumes = (ops == 0) | (ops == 2) | (ops == 3) | (ops == 7) | (ops == 8)
    rec = np.repeat(np.arange(rb.n), np.diff(rb.cigar_off))
    out = np.zeros(rb.n, np.int64)
    np.add.at(out, rec, np.where(consumes, lens, 0))
    return out


# ---------------------------------------------------------------------------------------
# the two launches
# ---------------------------------------------------------------------------------------
def _checked_pairs(dr, pairs, rows=None, width=None, span_only=False):
    """int64 [n, PAIR_WORDS] ready for the device, refused unless every pair fits its read, its region and the output
    (`span_only`: its read alone - rmr_region_signals looks at no lead, row or region length)."""
    pairs = np.asarray(pairs, np.int64)
    if pairs.ndim != 2 or pairs.shape[1] not in (7, PAIR_WORDS):
        raise RemoraError("Region pairs are rows of (read, first, last, lead, row, region length, flip)")
    full = np.zeros((pairs.shape[0], PAIR_WORDS), np.int64)
    full[:, : pairs.shape[1]] = pairs
    full[:, 7] = 0
    if not full.shape[0]:
        return full
    read, first, last, lead, row, rlen, flip = (full[:, k] for k in range(7))
    if read.min() < 0 or read.max() >= dr.n_reads:
        raise RemoraError("Region pair names a read outside the batch")
    n_bases = np.diff(dr.seq_off)[read]
    if ((first < 0) | (first >= last) | (last > n_bases)).any():
        raise RemoraError("Region pair does not fit its read: 0 <= first < last <= bases of the read must hold")
    if not span_only and ((lead < 0) | (rlen <= 0) | (lead + (last - first) > rlen)).any():
        raise RemoraError("Region pair does not fit its region: lead + (last - first) <= region length must hold")
    if ((flip != 0) & (flip != 1)).any():
        raise RemoraError("Region pair with a flip other than 0 or 1")
    if rows is not None and (row.min() < 0 or row.max() >= rows or np.unique(row).size != row.size):
        raise RemoraError("Region pair outside the rows of the output (or two pairs for one row)")
    if width is not None and rlen.max() > width:
        raise RemoraError("Region longer than the output is wide")
    return full


def _scaling_tensors(dr, shift, scale):
    import torch

    if shift is None and scale is None:
        return dr.shift, dr.scale
    if shift is None or scale is None:
        raise RemoraError("shift and scale go together")
    dev = dr.engine.torch_device
    sh, sc = (torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(dev) for x in (shift, scale))
    if sh.numel() != dr.n_reads or sc.numel() != dr.n_reads:
        raise RemoraError("shift / scale need one value per read of the batch")
    return sh, sc


def _raise_on_status(status, what):
    bad = np.nonzero(status)[0]
    if bad.size:
        why = "the mapping leaves the read's signal" if int(status[bad[0]]) == 2 else "the pair does not fit"
        raise RemoraError(f"{what}: pair {int(bad[0])} was refused on the device ({why})")


def device_region_metrics(dr, pairs, metric, start_trim=1, end_trim=1, rows=None, width=None, shift=None, scale=None):
    """DeviceReads.region_metrics."""
    import torch

    from .metrics import _OUTPUTS, METRIC_KEYS

    if metric not in METRIC_KEYS:
        raise RemoraError(f"Unknown per-base metric: {metric}")
    if int(start_trim) < 0 or int(end_trim) < 0:
        raise RemoraError("Signal trims must not be negative")
    raw = _checked_pairs(dr, pairs)  # refused here, and again below with rows and width: nothing is allocated or launched for a bad pair
    if rows is None:
        rows = int(raw[:, 4].max()) + 1 if raw.ndim == 2 and raw.shape[0] else 0
    if width is None:
        width = int(raw[:, 5].max()) if raw.ndim == 2 and raw.shape[0] else 0
    rows, width = int(rows), int(width)
    full = _checked_pairs(dr, raw, rows, width)
    dr.wait_ready()
    dev = dr.engine.torch_device
    wanted = {src for _, src in METRIC_KEYS[metric]}
    out = {name: torch.full((max(rows, 1), max(width, 1)), float("nan"), dtype=torch.float64, device=dev) for name in wanted}
    if full.shape[0]:
        sh, sc = _scaling_tensors(dr, shift, scale)
        d_pairs = torch.from_numpy(full).to(dev)
        status = torch.zeros(full.shape[0], dtype=torch.int32, device=dev)
        ptr = lambda name: ctypes.c_void_p(out[name].data_ptr()) if name in out else None  # noqa: E731
        torch.cuda.current_stream(dev).synchronize()  # fills and uploads ran on torch's stream, the kernel runs on the engine's
        L.check(L.lib().rmr_region_base_metrics(dr.engine.handle, dr.n_reads, dr.dacs.data_ptr(), dr.d_sig_off.data_ptr(), dr.s2s.data_ptr(),
                                                dr.d_seq_off.data_ptr(), sh.data_ptr(), sc.data_ptr(), full.shape[0], d_pairs.data_ptr(),
                                                int((full[:, 2] - full[:, 1]).max()), int(start_trim), int(end_trim), rows, width,
                                                *(ptr(name) for name in _OUTPUTS), status.data_ptr()))
        dr.engine.synchronize()
        _raise_on_status(status.cpu().numpy(), "rmr_region_base_metrics")
    return {key: out[src][:rows, :width] for key, src in METRIC_KEYS[metric]}


def device_region_signals(dr, pairs, shift=None, scale=None, raw=False):
    """DeviceReads.region_signals."""
    import torch

    full = _checked_pairs(dr, pairs, span_only=True)
    n = full.shape[0]
    sig_off, map_off = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    sig_dtype = np.int16 if raw else np.float64
    if not n:
        return np.zeros(0, sig_dtype), sig_off, np.zeros(0, np.int64), map_off, np.zeros(0, np.int64)
    dr.wait_ready()
    dev = dr.engine.torch_device
    read, first, last = full[:, 0], full[:, 1], full[:, 2]
    at = dr.seq_off[read] + read  # a read's mapping starts at seq_off[r] + r: one more entry than bases per read
    # the two mapping entries that bound every pair's samples: all the host needs to lay the pairs out back to back
    ends = dr.s2s[torch.from_numpy(np.concatenate([at + first, at + last])).to(dev)].cpu().numpy()
    n_sig = ends[n:] - ends[:n]
    if (n_sig < 0).any():
        raise RemoraError("Region pair on a mapping that runs backwards")
    np.cumsum(n_sig, out=sig_off[1:])
    np.cumsum(last - first + 1, out=map_off[1:])
    sh, sc = _scaling_tensors(dr, shift, scale)
    sig = torch.empty(max(int(sig_off[-1]), 1), dtype=torch.int16 if raw else torch.float64, device=dev)
    smap = torch.empty(int(map_off[-1]), dtype=torch.int64, device=dev)
    start = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    d_pairs, d_so, d_mo = (torch.from_numpy(x).to(dev) for x in (full, sig_off, map_off))
    torch.cuda.current_stream(dev).synchronize()
    L.check(L.lib().rmr_region_signals(dr.engine.handle, dr.n_reads, dr.dacs.data_ptr(), dr.d_sig_off.data_ptr(), dr.s2s.data_ptr(),
                                       dr.d_seq_off.data_ptr(), sh.data_ptr(), sc.data_ptr(), n, d_pairs.data_ptr(), d_so.data_ptr(),
                                       d_mo.data_ptr(), int(bool(raw)), sig.data_ptr(), int(sig_off[-1]), smap.data_ptr(), int(map_off[-1]),
                                       start.data_ptr(), status.data_ptr()))
    dr.engine.synchronize()
    _raise_on_status(status.cpu().numpy(), "rmr_region_signals")
    return sig[: int(sig_off[-1])].cpu().numpy(), sig_off, smap.cpu().numpy(), map_off, start.cpu().numpy()


# ---------------------------------------------------------------------------------------
# the pass
# ---------------------------------------------------------------------------------------
class _Ready:
    """Reads of one batch that are resident and refined: what both kernels need beside the pairs.  `slot[j]`: the number (inside
    its sample) of the picked record read j was built from; `ref_start`, `ref_len`, `is_rev`: the read's span on the reference and its strand; `seq(j)`: the read's
    reference bases in read orientation; `scaling(signal_type)`: per-read (shift, scale) or (None, None) for the batch's own."""

    def __init__(self, dr, slot, ref_start, ref_len, is_rev, map0, read_ids, seq, scaling):
        self.dr, self.slot, self.ref_start, self.ref_len, self.is_rev = dr, slot, ref_start, ref_len, is_rev
        self.map0, self.read_ids, self.seq, self.scaling = map0, read_ids, seq, scaling


def _refine_resident(refiner, dr, stubs):
    loaded = refiner is not None and getattr(refiner, "is_loaded", False)
    if loaded and refiner.do_rough_rescale:
        refiner.rough_rescale_device(dr, stubs)
    if loaded and refiner.scale_iters >= 0:
        refiner.refine_device_reads(dr, stubs)


def _ready_from_io_reads(io_reads, slots, refiner, missing_ok, device):
    """The read-by-read way into the same kernels: io.Read objects (with their alignment) refined one by one as
    Read.set_refine_signal_mapping(refiner, ref_mapping=True) does and uploaded as one batch.  A read that cannot be built or
    refined is left out with `missing_ok` and raises otherwise."""
    from .data_chunks import DeviceReads
    from .engine import get_engine

    rrs, kept, kept_slots = [], [], []
    for io_read, slot in zip(io_reads, slots):
        try:
            if io_read.ref_to_signal is None:
                raise RemoraError("Missing ref_to_signal (move table)")
            if refiner is not None:
                io_read.set_refine_signal_mapping(refiner, ref_mapping=True)
            rr = io_read.into_remora_read(True)
        except RemoraError:
            if missing_ok:
                continue
            raise
        rrs.append(rr)
        kept.append(io_read)
        kept_slots.append(slot)
    if not rrs:
        return None
    dr = DeviceReads(rrs, get_engine(device))

    def scaling(signal_type):
        got = [r._sig_scaling(signal_type) for r in kept]
        return np.asarray([g[0] for g in got], np.float64), np.asarray([g[1] for g in got], np.float64)

    return _Ready(dr, np.asarray(kept_slots, np.int64), np.asarray([r.ref_reg.start for r in kept], np.int64),
                  np.asarray([r.ref_to_signal.size - 1 for r in kept], np.int64), np.asarray([r.ref_reg.strand == "-" for r in kept], bool),
                  np.asarray([int(r.ref_to_signal[0]) for r in kept], np.int64), [r.read_id for r in kept],
                  lambda j: kept[j].ref_seq, scaling)


def _io_reads_of_records(records, signals, reverse_signal, pa_scaling, missing_ok, device):
    """(io.Read list, their positions in `records`) as the reference's get_io_reads builds them (src/remora/io.py:775-796): a
    record whose read cannot be built raises RemoraError("BAM record not found in POD5") unless `missing_ok`."""
    from . import io as rio
    from .engine import get_ingest_engine

    built = {}
    for io_read, err in rio._reads_of_records(records, signals, get_ingest_engine(device), bool(reverse_signal), pa_scaling, False,
                                              max(len(records), 2), True):
        if err is None:
            built[id(io_read.record)] = io_read
    reads, where = [], []
    for k, rec in enumerate(records):
        io_read = built.get(id(rec))
        if io_read is None:
            if missing_ok:
                continue
            raise RemoraError("BAM record not found in POD5")
        reads.append(io_read)
        where.append(k)
    return reads, where


def _ready_from_batch(rb, records, picked, slots, signals, refiner, reverse_signal, pa_scaling, missing_ok, device):
    """_Ready for the picked records of one raw BAM batch (`picked`: record indices, `slots`: their numbers), through the batch
    ingest and the resident refiner where they cover the batch, read by read otherwise."""
    from . import io as rio
    from .engine import get_ingest_engine

    select = np.zeros(rb.n, bool)
    select[picked] = True
    got = "slow" if pa_scaling is not None else rio._ingest_batch(
        rb, records, signals, get_ingest_engine(device), None, True, ref_anchored=True, reverse_signal=reverse_signal, select=select)
    if isinstance(got, rio.IngestBatch):
        gk = got.keep[got.good]
        if not missing_ok and gk.size != len(picked):
            raise RemoraError("BAM record not found in POD5")
        if not gk.size:
            return None
        try:
            _refine_resident(refiner, got.dr, got.reads)
        except RemoraError:
            got = "slow"  # a read whose band the refiner rejects: the per-read path says which, and keeps the others
    elif got is None:
        if not missing_ok:
            raise RemoraError("BAM record not found in POD5")
        return None
    if isinstance(got, str):
        recs = records(rb)
        chosen = [recs[i] for i in picked]
        io_reads, where = _io_reads_of_records(chosen, signals, reverse_signal, pa_scaling, missing_ok, device)
        return _ready_from_io_reads(io_reads, [slots[k] for k in where], refiner, missing_ok, device)
    slot_of = dict(zip(picked, slots))
    lens = np.diff(got.seq_off)
    has_pi = (rb.has & 64) != 0
    ids = [(rb.pi[rb.pi_off[i] : rb.pi_off[i + 1]] if has_pi[i] else rb.names[rb.name_off[i] : rb.name_off[i + 1]]).decode("latin-1")
           for i in gk.tolist()]
    seq, seq_off, cal_off, cal_scale = got.seq, got.seq_off, got.cal_off, got.cal_scale

    def scaling(signal_type):
        if signal_type == "pa":
            return cal_off, cal_scale
        if signal_type == "zc_pa":
            raise RemoraError("Zero-centred pA scaling factors not set")
        if signal_type in ("norm", "dac"):
            return None, None
        raise RemoraError(f"Invalid signal_type: {signal_type}")

    return _Ready(got.dr, np.asarray([slot_of[i] for i in gk.tolist()], np.int64), rb.pos[gk].astype(np.int64), lens,
                  (rb.flag[gk] & 16) != 0, got.map0, ids, lambda j: seq[seq_off[j] : seq_off[j + 1]].decode("latin-1"), scaling)


def _pairs_of_ready(ready, regions, wanted, ref_orient, extract):
    """The pairs of one resident batch: `wanted[r]` = {slot: row} for region r.  -> (int64 [n, 7] pair table with batch-local
    rows, and per pair its region, its row there and its read)."""
    table, meta = [], []
    pos_of = {int(s): j for j, s in enumerate(ready.slot.tolist())}
    for r, reg in enumerate(regions):
        for slot, row in wanted[r].items():
            j = pos_of.get(slot)
            if j is None:
                continue
            rev = bool(ready.is_rev[j])
            end = reg.start + 1 if reg.end is None else reg.end
            first, last, lead = _span_in_read(ready.ref_start[j], ready.ref_len[j], rev, reg.start, end, extract)
            table.append((j, int(first), int(last), int(lead), len(table), end - reg.start, int(rev and (extract or ref_orient))))
            meta.append((r, row, j))
    return np.asarray(table, np.int64).reshape(-1, 7), meta


def _region_pass(ref_regs, pod5_bam_pairs, extract, sig_map_refiner, skip_sig_map_refine, max_reads, reverse_signal, missing_ok, pa_scaling,
                 signal_type, metric, ref_orient, start_trim, end_trim, reads_per_batch, device):
    """-> per region None (some sample has no read there) or a list per sample of (records, rows): the picked BamRecords and, per
    record that could be built, in the same order, {metric key: float64 row} or a ReadRefReg.
    The raw batches that hold a covering record stay in host memory (16 KB a record) until their sample's reads are drawn, since
    `max_reads` draws from all records of a region: a few loci hold a few batches, regions tiled over a whole BAM hold the BAM."""
    from . import io as rio

    refiner = None if skip_sig_map_refine else sig_map_refiner
    n_reg = len(ref_regs)
    # 1. every BAM once: the records that cover some region, from the raw batches' fixed fields; no signal is touched
    samples = []
    for pod5, bam_path in pod5_bam_pairs:
        signals = rio.open_pod5(pod5, device=device)
        names = rio.bam_reference_names(bam_path)
        held, cands = [], [[] for _ in range(n_reg)]
        for rb, records in rio.iter_bam_raw_batches(bam_path, want_ref=True, batch=reads_per_batch):
            plan = plan_region_pairs(ref_regs, names, rb.ref_id, rb.pos, _ref_lens_of_batch(rb), rb.flag)
            if not plan["read"].size:
                continue
            for r, i in zip(plan["region"].tolist(), plan["read"].tolist()):
                cands[r].append((len(held), i))
            held.append((rb, records))
        samples.append((signals, held, cands))
    # 2. who is used: everybody, or max_reads of them drawn as the reference draws (random.sample, for region: for sample:)
    live = [all(len(cands[r]) > 0 for _, _, cands in samples) for r in range(n_reg)]
    for r, reg in enumerate(ref_regs):
        if live[r] and not extract and (reg.strand is None or reg.strand not in "+-"):
            raise RemoraError("Region contig/strand do not match read")  # (Read.compute_per_base_metric compares the strands, :2438-2442)
    for r in range(n_reg):
        for _, _, cands in samples:
            if live[r] and max_reads is not None and len(cands[r]) > max_reads:
                cands[r] = [cands[r][k] for k in random.sample(range(len(cands[r])), max_reads)]
    # 3. per sample and held batch: ingest what was picked, refine, run the kernel for all regions at once
    out = [None if not live[r] else [] for r in range(n_reg)]
    for signals, held, cands in samples:
        slots, wanted, rows = {}, [dict() for _ in range(n_reg)], [dict() for _ in range(n_reg)]
        for r in range(n_reg):
            if not live[r]:
                continue
            for row, key in enumerate(cands[r]):
                wanted[r][slots.setdefault(key, len(slots))] = row
        per_batch = {}
        for (b, i), slot in slots.items():
            per_batch.setdefault(b, []).append((i, slot))
        recs_of_batch = {}
        for b in sorted(per_batch):
            rb, records = held[b]
            picked = sorted(per_batch[b])
            recs_of_batch[b] = records(rb)
            ready = _ready_from_batch(rb, records, [i for i, _ in picked], [s for _, s in picked], signals, refiner, reverse_signal,
                                      pa_scaling, missing_ok, device)
            if ready is not None:
                _run_ready(ready, ref_regs, wanted, rows, extract, signal_type, metric, ref_orient, start_trim, end_trim)
        for r in range(n_reg):
            if live[r]:
                out[r].append(([recs_of_batch[b][i] for b, i in cands[r]], [rows[r][k] for k in sorted(rows[r])]))
    return out


def _run_ready(ready, ref_regs, wanted, rows, extract, signal_type, metric, ref_orient, start_trim, end_trim):
    """Both kernels' host side for one resident batch: results land in rows[region][row]."""
    from . import io as rio
    from .metrics import METRIC_KEYS

    table, meta = _pairs_of_ready(ready, ref_regs, wanted, ref_orient, extract)
    if not table.shape[0]:
        return
    shift, scale = ready.scaling(signal_type)
    if not extract:
        if signal_type == "dac":
            shift, scale = np.zeros(ready.dr.n_reads), np.ones(ready.dr.n_reads)
        got = {k: v.cpu().numpy() for k, v in ready.dr.region_metrics(table, metric, start_trim, end_trim, shift=shift, scale=scale).items()}
        for p, (r, row, _j) in enumerate(meta):
            n, partial = int(table[p, 5]), int(table[p, 2] - table[p, 1]) < int(table[p, 5])
            rows[r][row] = ({key: got[key][p, :n] for key, _ in METRIC_KEYS[metric]}, partial)
        return
    sig, sig_off, smap, map_off, start = ready.dr.region_signals(table, shift, scale, raw=signal_type == "dac")
    for p, (r, row, j) in enumerate(meta):
        first, last, flip = int(table[p, 1]), int(table[p, 2]), bool(table[p, 6])
        reg, seq = ref_regs[r], ready.seq(j)[first:last]
        ref_st = max(int(ready.ref_start[j]), reg.start)
        rows[r][row] = ReadRefReg(read_id=ready.read_ids[j], norm_signal=sig[sig_off[p] : sig_off[p + 1]].copy(), seq=seq[::-1] if flip else seq,
                                  seq_to_sig_map=smap[map_off[p] : map_off[p + 1]].copy(),
                                  ref_reg=rio.RefRegion(reg.ctg, "-" if ready.is_rev[j] else "+", ref_st, ref_st + len(seq)),
                                  sig_start=np.int64(start[p] + ready.map0[j]))


def _stack_metrics(rows, metric):
    """np.stack of the rows as the reference's per-read results stack: a read that covers its whole region returns dwell as
    float32, one that does not returns float64 rows (np.full(NaN), src/remora/io.py:2471-2478); everything else is float64."""
    from .metrics import METRIC_KEYS

    if not rows:
        return None
    any_partial = any(partial for _, partial in rows)
    out = {}
    for key, src in METRIC_KEYS[metric]:
        mat = np.stack([vals[key] for vals, _ in rows])
        out[key] = mat.astype(np.float32) if src == "dwell" and not any_partial else mat
    return out


def get_ref_regs_samples_metrics(ref_regs, pod5_bam_pairs, sig_map_refiner=None, skip_sig_map_refine=False, max_reads=None,
                                 reverse_signal=False, metric="dwell_trimmean", missing_ok=False, reads_per_batch=256, device=None, **kwargs):
    """get_ref_reg_samples_metrics for many regions with one pass over every BAM: a list with, per region, what the single call
    returns - or None for a region that some sample has no read on, where the single call raises.  For such a region nothing is
    drawn from `random`, where a sequence of single calls draws for the samples in front of the empty one before it raises: with
    `max_reads`, a seed and a region only some samples cover, the two forms leave the random stream in different states (and the
    regions after it draw other rows)."""
    from .metrics import DEFAULT_END_TRIM, DEFAULT_START_TRIM, METRIC_KEYS

    if metric not in METRIC_KEYS:
        raise RemoraError(f"Unknown per-base metric: {metric}")
    ref_regs = list(ref_regs)
    got = _region_pass(ref_regs, pod5_bam_pairs, False, sig_map_refiner, skip_sig_map_refine, max_reads, reverse_signal, missing_ok,
                       kwargs.get("pa_scaling"), kwargs.get("signal_type", "norm"), metric, kwargs.get("ref_orient", True),
                       kwargs.get("start_trim", DEFAULT_START_TRIM), kwargs.get("end_trim", DEFAULT_END_TRIM), reads_per_batch, device)
    out = []
    for per_sample in got:
        if per_sample is None:
            out.append(None)
            continue
        stacked = [_stack_metrics(rows, metric) for _, rows in per_sample]
        out.append(([m for m in stacked if m is not None], [recs for recs, _ in per_sample]))
    return out


def get_ref_reg_samples_metrics(ref_reg, pod5_bam_pairs, sig_map_refiner=None, skip_sig_map_refine=False, max_reads=None,
                                reverse_signal=False, metric="dwell_trimmean", missing_ok=False, **kwargs):
    """(samples_metrics, all_bam_reads), src/remora/io.py:889-922: per (POD5, BAM) pair the named metric of every read that covers
    `ref_reg`, {key: array [reads, region length]} with NaN where a read does not cover, and the BamRecords of the rows.
    `pod5_bam_pairs`: (POD5 path - a file or a run's directory, io.open_pod5 - or open io.Pod5File / io.Pod5Dataset, BAM path) where the reference takes open handles; no index is needed: the BAM is
    streamed once.  Rows are in file order - fetch order for the coordinate-sorted BAMs the reference requires; an unsorted BAM
    gives its own order - or, with `max_reads`, in the order random.sample draws them, from the same random numbers as the
    reference.  kwargs: ref_orient, signal_type, pa_scaling, start_trim, end_trim as get_ref_reg_sample_metrics takes them, and
    reads_per_batch / device.  Raises RemoraError("No reads covering region")."""
    got = get_ref_regs_samples_metrics([ref_reg], pod5_bam_pairs, sig_map_refiner, skip_sig_map_refine, max_reads, reverse_signal, metric,
                                       missing_ok, **kwargs)[0]
    if got is None:
        raise RemoraError("No reads covering region")
    return got


def get_ref_reg_sample_metrics(ref_reg, pod5, bam_reads, metric, sig_map_refiner, skip_sig_map_refine=False, reverse_signal=False,
                               ref_orient=True, missing_ok=False, pa_scaling=None, signal_type="norm", device=None, **kwargs):
    """The named metric of records the caller chose (src/remora/io.py:840-886): {key: array [reads, region length]}, None without
    reads.  `pod5`: path (a file, or a run's directory of files: io.open_pod5), io.Pod5File or io.Pod5Dataset.  The reads are built and refined one by one and measured in one launch."""
    from . import io as rio
    from .metrics import DEFAULT_END_TRIM, DEFAULT_START_TRIM, METRIC_KEYS

    if metric not in METRIC_KEYS:
        raise RemoraError(f"Unknown per-base metric: {metric}")
    bam_reads = list(bam_reads)
    signals = rio.open_pod5(pod5, device=device)
    io_reads, where = _io_reads_of_records(bam_reads, signals, reverse_signal, pa_scaling, missing_ok, device)
    for io_read in io_reads:  # the reference's errors, before anything runs (:2438-2447)
        mine = io_read.ref_reg
        if mine is None or io_read.ref_to_signal is None:
            raise RemoraError("Missing ref_to_signal (move table)")
        if (mine.ctg, mine.strand) != (ref_reg.ctg, ref_reg.strand):
            raise RemoraError("Region contig/strand do not match read")
        if ref_reg.start >= mine.end or mine.start >= ref_reg.end:
            raise RemoraError("Region does not overlap read.")
    ready = _ready_from_io_reads(io_reads, where, None if skip_sig_map_refine else sig_map_refiner, missing_ok, device)
    if ready is None:
        return None
    wanted, rows = [{int(s): int(s) for s in ready.slot.tolist()}], [dict()]
    _run_ready(ready, [ref_reg], wanted, rows, False, signal_type, metric, ref_orient, kwargs.get("start_trim", DEFAULT_START_TRIM),
               kwargs.get("end_trim", DEFAULT_END_TRIM))
    return _stack_metrics([rows[0][k] for k in sorted(rows[0])], metric)


def get_reads_reference_regions_many(ref_regs, pod5_bam_pairs, sig_map_refiner=None, skip_sig_map_refine=False, max_reads=50,
                                     reverse_signal=False, missing_ok=False, pa_scaling=None, signal_type="norm", reads_per_batch=256,
                                     device=None):
    """get_reads_reference_regions for many regions with one pass over every BAM: per region what the single call returns, or
    None for a region that some sample has no read on (nothing is drawn from `random` for it: see get_ref_regs_samples_metrics)."""
    ref_regs = list(ref_regs)
    if signal_type not in ("norm", "pa", "zc_pa", "dac"):
        raise RemoraError(f"Invalid signal_type: {signal_type}")
    got = _region_pass(ref_regs, pod5_bam_pairs, True, sig_map_refiner, skip_sig_map_refine, max_reads, reverse_signal, missing_ok, pa_scaling,
                       signal_type, None, True, 0, 0, reads_per_batch, device)
    return [None if per_sample is None else ([rows for _, rows in per_sample], [recs for recs, _ in per_sample]) for per_sample in got]


def get_reads_reference_regions(ref_reg, pod5_bam_pairs, sig_map_refiner=None, skip_sig_map_refine=False, max_reads=50,
                                reverse_signal=False, missing_ok=False, pa_scaling=None, signal_type="norm", **kwargs):
    """(samples_read_ref_regs, all_bam_reads), src/remora/io.py:799-837: per (POD5, BAM) pair the ReadRefReg of every read that
    covers `ref_reg` - its samples there, normalised in float64 as Read.get_sig_type does, the region-local mapping and sequence,
    reverse-strand reads turned onto the reference - and the BamRecords.  Pairs, order, sampling and kwargs (reads_per_batch,
    device) as in get_ref_reg_samples_metrics."""
    got = get_reads_reference_regions_many([ref_reg], pod5_bam_pairs, sig_map_refiner, skip_sig_map_refine, max_reads, reverse_signal,
                                           missing_ok, pa_scaling, signal_type, **kwargs)[0]
    if got is None:
        raise RemoraError("No reads covering region")
    return got
