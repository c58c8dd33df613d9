"""Per-base signal metrics (src/remora/metrics.py) and the k-mer level table estimated from them.

Two forms of the same five metrics:
  - METRIC_FUNCS: the reference's names, signatures `f(sig, seq_to_sig, **kwargs)` and returned keys, for ONE read whose
    signal is already a float array (any signal type, a caller's own metric_func beside them) - numpy on the host;
  - base_metrics(): a whole batch of resident reads (data_chunks.DeviceReads) in one launch of rmr_base_metrics
    (csrc/k_metrics.hip), from the int16 samples and each read's shift / scale.  io.Read.compute_per_base_metric and
    DeviceReads.per_base_metrics go through it.
Both sum every base's own samples directly in float64; the reference takes differences of a whole-read cumulative sum
(metrics.py:12-42), whose rounding grows with the read, so the two agree to that rounding and not to the bit.

SiteLevels accumulates the trimmed means of reference-anchored batches on the device and hands them to
rmr_site_kmer_levels: median per reference site, then per k-mer (io.get_region_kmers, src/remora/io.py:930-982)."""
import ctypes

import numpy as np

from . import RemoraError
from . import _lib as L

DEFAULT_START_TRIM = 1
DEFAULT_END_TRIM = 1
MAX_LEVEL_KMER = 8  # RMR_MAX_LEVEL_KMER of include/remora_hip.h


def _range_sums(x, starts, ends):
    """sum(x[s:e]) for every pair, float64, each range summed on its own (0 for an empty or reversed range)."""
    out = np.zeros(starts.size, np.float64)
    if not starts.size:
        return out
    full = ends > starts
    padded = np.append(np.asarray(x, np.float64), 0.0)
    idx = np.stack([np.clip(starts, 0, x.size), np.clip(ends, 0, x.size)], axis=1).ravel()
    out[full] = np.add.reduceat(padded, idx)[::2][full]
    return out


def _mean_and_sd(sig, seq_to_sig, dwells, st_trim, en_trim, want_sd):
    """Mean (and sd) over the samples of every base left after the trims; `dwells` float32 as compute_dwell returns them.  An
    empty base is NaN (metrics.py:21-24: the reference's inf becomes NaN too).  Only the signal the mapping spans counts
    (metrics.py:7-9): a trimmed range is held inside [seq_to_sig[0], seq_to_sig[-1]], in the signal's own indices."""
    sig = np.asarray(sig, np.float64)
    seq_to_sig = np.asarray(seq_to_sig, np.int64)
    first, last = (int(seq_to_sig[0]), int(seq_to_sig[-1])) if seq_to_sig.size else (0, 0)
    starts = np.minimum(last, seq_to_sig[:-1] + st_trim)
    ends = np.maximum(first, seq_to_sig[1:] - en_trim)
    eff = np.maximum(0, dwells - st_trim - en_trim) if (st_trim or en_trim) else dwells
    with np.errstate(divide="ignore", invalid="ignore"):
        means = np.where(eff > 0, _range_sums(sig, starts, ends) / eff, np.nan)
        if not want_sd:
            return means, None
        sds = np.where(eff > 0, np.sqrt(np.maximum(0, _range_sums(np.square(sig), starts, ends) / eff - np.square(means))), np.nan)
    return means, sds


def compute_dwell(sig, seq_to_sig, **kwargs):
    return {"dwell": np.diff(seq_to_sig).astype(np.float32)}


def compute_dwell_mean(sig, seq_to_sig, **kwargs):
    dwells = compute_dwell(sig, seq_to_sig)["dwell"]
    return {"dwell": dwells, "mean": _mean_and_sd(sig, seq_to_sig, dwells, 0, 0, False)[0]}


def compute_dwell_mean_sd(sig, seq_to_sig, **kwargs):
    dwells = compute_dwell(sig, seq_to_sig)["dwell"]
    means, sds = _mean_and_sd(sig, seq_to_sig, dwells, 0, 0, True)
    return {"dwell": dwells, "mean": means, "sd": sds}


def compute_trimmean(sig, seq_to_sig, **kwargs):
    st, en = kwargs.get("start_trim", DEFAULT_START_TRIM), kwargs.get("end_trim", DEFAULT_END_TRIM)
    dwells = compute_dwell(sig, seq_to_sig)["dwell"]
    # ("dwells": the reference's key for this one function, metrics.py:81)
    return {"dwells": dwells, "trimmean": _mean_and_sd(sig, seq_to_sig, dwells, st, en, False)[0]}


def compute_trimmean_trimsd(sig, seq_to_sig, **kwargs):
    st, en = kwargs.get("start_trim", DEFAULT_START_TRIM), kwargs.get("end_trim", DEFAULT_END_TRIM)
    dwells = compute_dwell(sig, seq_to_sig)["dwell"]
    means, sds = _mean_and_sd(sig, seq_to_sig, dwells, st, en, True)
    return {"dwell": dwells, "trimmean": means, "trimsd": sds}


# returned key -> output of rmr_base_metrics, per named metric (the keys METRIC_FUNCS return, in their order)
METRIC_KEYS = {
    "dwell": (("dwell", "dwell"),),
    "dwell_mean": (("dwell", "dwell"), ("mean", "mean")),
    "dwell_mean_sd": (("dwell", "dwell"), ("mean", "mean"), ("sd", "sd")),
    "dwell_trimmean": (("dwells", "dwell"), ("trimmean", "trimmean")),
    "dwell_trimmean_trimsd": (("dwell", "dwell"), ("trimmean", "trimmean"), ("trimsd", "trimsd")),
}
_OUTPUTS = ("dwell", "mean", "sd", "trimmean", "trimsd")
# the host form of each, under the reference's names (metrics.py:111-117)
METRIC_FUNCS = dict(zip(METRIC_KEYS, (compute_dwell, compute_dwell_mean, compute_dwell_mean_sd, compute_trimmean, compute_trimmean_trimsd)))


def base_metrics(dr, metric, start_trim=DEFAULT_START_TRIM, end_trim=DEFAULT_END_TRIM):
    """The named metric for every base of a resident batch: {key: tensor[n_bases] on the device} with METRIC_FUNCS' keys (dwell
    float32, the rest float64), bases concatenated as in `dr.seq_off`.  One launch; the caller synchronises (`dr.engine`) or
    copies the tensors back, which waits."""
    import torch

    if metric not in METRIC_KEYS:
        raise RemoraError(f"Unknown per-base metric: {metric}")
    if int(start_trim) < 0 or int(end_trim) < 0:
        raise RemoraError("Signal trims must not be negative")
    dr.wait_ready()
    dev = dr.engine.torch_device
    n = int(dr.seq_off[-1])
    wanted = {src for _, src in METRIC_KEYS[metric]}
    out = {name: torch.empty(max(n, 1), dtype=torch.float32 if name == "dwell" else torch.float64, device=dev) for name in wanted}
    ptr = lambda name: ctypes.c_void_p(out[name].data_ptr()) if name in out else None  # noqa: E731
    longest = int(np.diff(dr.seq_off).max()) if dr.n_reads else 0
    # the outputs are blocks of torch's allocator, which may hand out one whose last use on torch's stream is still in flight;
    # the kernel runs on the engine's stream: wait for torch's first
    torch.cuda.current_stream(dev).synchronize()
    L.check(L.lib().rmr_base_metrics(dr.engine.handle, dr.n_reads, dr.dacs.data_ptr(), dr.d_sig_off.data_ptr(), dr.s2s.data_ptr(),
                                     dr.d_seq_off.data_ptr(), dr.shift.data_ptr(), dr.scale.data_ptr(), longest, int(start_trim),
                                     int(end_trim), *(ptr(name) for name in _OUTPUTS)))
    dr.engine.synchronize()
    return {key: out[src][:n] for key, src in METRIC_KEYS[metric]}


def read_base_metrics(dacs, shift, scale, seq_to_sig, metric, start_trim=DEFAULT_START_TRIM, end_trim=DEFAULT_END_TRIM, engine=None):
    """The same for one read given as host arrays: {key: numpy array}.  `seq_to_sig` indexes `dacs` (it need not start at 0
    or end at the last sample: the signal outside is clipped as clip_sig does)."""
    from types import SimpleNamespace

    from .data_chunks import DeviceReads

    seq_to_sig = np.ascontiguousarray(seq_to_sig, np.int64)
    one = SimpleNamespace(dacs=np.ascontiguousarray(dacs), shift=float(shift), scale=float(scale), seq_to_sig_map=seq_to_sig,
                          int_seq=np.zeros(max(seq_to_sig.size - 1, 0), np.int8), read_id=None)
    dr = DeviceReads([one], engine)
    return {k: v.cpu().numpy() for k, v in base_metrics(dr, metric, start_trim, end_trim).items()}


# site key, 63 bits: sample (8) | contig (20) | strand (1) | u (34), u < 2^32 the read-oriented coordinate.  u leaves the two top
# bits of its field empty, so the last site of one (sample, contig, strand) and the first of the next are > 2^33 apart
_U_BITS, _CONTIG_BITS, _SAMPLE_BITS = 34, 20, 8
_STRAND_BIT = _U_BITS
_CONTIG_SHIFT = _STRAND_BIT + 1
_SAMPLE_SHIFT = _CONTIG_SHIFT + _CONTIG_BITS
_REV_ORIGIN = (1 << 32) - 1
MAX_LEVEL_CONTIGS, MAX_LEVEL_SAMPLES = 1 << _CONTIG_BITS, 1 << _SAMPLE_BITS


def site_key0(sample, ref_id, is_reverse, ref_start, ref_len):
    """Site keys of the first bases of reference-anchored reads (numpy arrays): the key grows by one per base in read
    orientation - reference position on the forward strand, 2^32 - 1 - position on the reverse strand.  Sample, contig and
    strand each have a field of their own; a value that does not fit its field is refused, never folded into a neighbour's."""
    ref_id, ref_start, ref_len = (np.asarray(x, np.int64) for x in (ref_id, ref_start, ref_len))
    rev = np.asarray(is_reverse, bool)
    if not 0 <= int(sample) < MAX_LEVEL_SAMPLES:
        raise RemoraError(f"k-mer levels take up to {MAX_LEVEL_SAMPLES} pod5/BAM pairs, got pair {int(sample)}")
    if ref_id.size and (ref_id.min() < 0 or ref_id.max() >= MAX_LEVEL_CONTIGS):
        raise RemoraError(f"k-mer levels take references of up to {MAX_LEVEL_CONTIGS} contigs, got contig index {int(ref_id.max())}"
                          if ref_id.min() >= 0 else "k-mer levels need mapped reads (negative contig index)")
    if ref_id.size and (ref_start.min() < 0 or ref_len.min() < 0 or (ref_start + ref_len).max() > _REV_ORIGIN):
        raise RemoraError("k-mer levels take reference positions in [0, 2^32 - 1)")
    u = np.where(rev, _REV_ORIGIN - (ref_start + ref_len - 1), ref_start)
    return (np.int64(int(sample)) << _SAMPLE_SHIFT) | (ref_id << _CONTIG_SHIFT) | (rev.astype(np.int64) << _STRAND_BIT) | u


def describe_site_key(key):
    """'sample S, contig index C, strand +/-, position P' of a site key (the inverse of site_key0)."""
    key = int(key)
    u, rev = key & ((1 << _U_BITS) - 1), (key >> _STRAND_BIT) & 1
    return (f"sample {key >> _SAMPLE_SHIFT}, contig index {(key >> _CONTIG_SHIFT) & (MAX_LEVEL_CONTIGS - 1)}, strand {'-' if rev else '+'}, "
            f"position {_REV_ORIGIN - u if rev else u}")


class LevelObservations:
    """The observations of a set of reads as key intervals [key0, key0 + len): how many lie below a key, in closed form.
    F(x) = sum_i clip(x - key0_i, 0, len_i) = sum_{key0 < x} (x - key0) - sum_{end < x} (x - end): two searchsorted calls and two
    prefix sums.  The sums run modulo 2^64 (keys have 63 bits, so the partial sums wrap); F itself is a number of bases and
    comes out exact."""

    def __init__(self, key0, lens):
        key0, lens = np.asarray(key0, np.int64).ravel(), np.asarray(lens, np.int64).ravel()
        if key0.shape != lens.shape or (lens.size and lens.min() < 0):
            raise RemoraError("k-mer level ranges: one non-negative base count per read")
        key0, lens = key0[lens > 0], lens[lens > 0]
        self.n_bases = int(lens.sum())
        self.starts, self.ends = np.sort(key0), np.sort(key0 + lens)
        with np.errstate(over="ignore"):
            zero = np.zeros(1, np.uint64)
            self._start_sum = np.concatenate([zero, np.cumsum(self.starts.view(np.uint64), dtype=np.uint64)])
            self._end_sum = np.concatenate([zero, np.cumsum(self.ends.view(np.uint64), dtype=np.uint64)])
        # F is linear between the sorted distinct starts and ends; cover[j] reads lie on every key of [points[j], points[j + 1])
        self.points = np.unique(np.concatenate([self.starts, self.ends]))
        self.cover = np.searchsorted(self.starts, self.points, "right") - np.searchsorted(self.ends, self.points, "right")
        self.below_points = self.below(self.points)

    def below(self, x):
        """F(x): observations with a key < x, for an int or an array of keys."""
        xs = np.atleast_1d(np.asarray(x, np.int64))
        i, j = np.searchsorted(self.starts, xs, "left"), np.searchsorted(self.ends, xs, "left")
        with np.errstate(over="ignore"):
            xu = xs.view(np.uint64)
            out = ((i.astype(np.uint64) * xu - self._start_sum[i]) - (j.astype(np.uint64) * xu - self._end_sum[j])).view(np.int64)
        return out if np.ndim(x) else int(out[0])

    def last_key_within(self, total):
        """The largest x with F(x) <= total; None when every x has."""
        j = int(np.searchsorted(self.below_points, total, "right")) - 1
        if j >= self.points.size - 1:
            return None
        return int(self.points[j]) + (int(total) - int(self.below_points[j])) // int(self.cover[j])

    def window(self, key, kb, ka):
        """Observations that aggregating the single site `key` keeps resident: those of [key - kb, key + ka]."""
        return self.below(int(key) + 1 + ka) - self.below(int(key) - kb)

    def largest_window(self, kb, ka):
        """(observations, key) of the site whose window holds the most: the smallest budget plan_level_ranges can work with.
        The window count is linear between the keys at which one of its two ends meets a start or an end of a read."""
        if not self.points.size:
            return 0, 0
        lo, hi = int(self.points[0]), int(self.points[-1])
        cand = np.unique(np.clip(np.concatenate([self.points + kb, self.points - 1 - ka]), lo, hi - 1))
        w = self.below(cand + 1 + ka) - self.below(cand - kb)
        at = int(np.argmax(w))
        return int(w[at]), int(cand[at])


def plan_level_ranges(key0, lens, max_resident_bases, kb, ka):
    """Cut keys int64[n_ranges + 1], from the smallest key0 to the largest key0 + len, of the ranges [a, b) that k-mer levels are
    aggregated in one after the other: the observations a range keeps on the device - those with keys in [a - kb, b + ka), the
    margins being the bases its first and last sites' k-mers reach for - number at most `max_resident_bases`, and every range is
    as long as that allows.  Cuts fall anywhere, inside reads too.  A site whose own window of kb + 1 + ka keys holds more than
    the budget cannot be cut: RemoraError that names it."""
    kb, ka, budget = int(kb), int(ka), int(max_resident_bases)
    obs = LevelObservations(key0, lens)
    if not obs.points.size:
        return np.zeros(1, np.int64)
    a, hi = int(obs.points[0]), int(obs.points[-1])
    cuts = [a]
    while a < hi:
        x = obs.last_key_within(budget + obs.below(a - kb))
        b = hi if x is None else min(hi, x - ka)
        if b <= a:
            need, worst = obs.largest_window(kb, ka)
            raise RemoraError(f"k-mer levels: the site at {describe_site_key(a)} is covered by {obs.window(a, 0, 0)} reads and the "
                              f"{kb + ka + 1} sites its k-mer spans hold {obs.window(a, kb, ka)} bases, more than the {budget} that may be resident "
                              f"at once; this input needs room for {need} (the site at {describe_site_key(worst)})")
        cuts.append(b)
        a = b
    return np.asarray(cuts, np.int64)


def clip_to_key_range(trimmean, int_seq, key0, seq_len, lo, hi):
    """The part of a batch (as SiteLevels.add takes it) that lies on the keys [lo, hi): read i keeps its bases
    [max(0, lo - key0), min(len, hi - key0)), its key0 moves with the first of them, a read that keeps none leaves.  The values
    stay on the device (one gather).  -> trimmean, int_seq, key0, seq_len."""
    import torch

    key0, seq_len = np.asarray(key0, np.int64), np.asarray(seq_len, np.int64)
    first = np.clip(lo - key0, 0, seq_len)
    last = np.clip(hi - key0, first, seq_len)
    if not first.any() and np.array_equal(last, seq_len):
        return trimmean, int_seq, key0, seq_len
    keep = last > first
    src = (np.concatenate([[0], np.cumsum(seq_len)[:-1]]) + first)[keep]
    new_len = (last - first)[keep]
    dst = np.concatenate([[0], np.cumsum(new_len)[:-1]]) if new_len.size else np.zeros(0, np.int64)
    n = int(new_len.sum())
    dev = trimmean.device
    # base k of the clipped batch is base k + (src - dst)[its read] of the batch
    shift = torch.repeat_interleave(torch.from_numpy(src - dst).to(dev), torch.from_numpy(new_len).to(dev), output_size=n)
    idx = torch.arange(n, dtype=torch.int64, device=dev) + shift
    return trimmean[idx], int_seq[idx], (key0 + first)[keep], new_len


# device bytes per observation (one base of one read): 9 kept from batch to batch (trimmed mean f64, base i8), and in levels() the
# four 8-byte key / payload arrays of the radix sorts beside them, plus the sorts' own scratch (a small fraction)
LEVEL_BYTES_PER_BASE = 9 + 4 * 8 + 1


LEVEL_SORT_BYTES = 4 * 8  # of them, the sort buffers of one observation (stage 1) or one site (stage 2)


class SiteLevels:
    """Trimmed means of reference-anchored reads, batch by batch, resident on one device; `levels()` runs the two-stage
    median there (rmr_site_kmer_levels).
    `max_resident_bases`: the input is aggregated one range of site keys after the other (plan_level_ranges cuts them) with at
    most that many observations on the device at a time: begin_range(a, b), add(...) for every batch that meets the range -
    add keeps what lies on [a - kb, b + ka) -, end_range() (rmr_site_medians: the sites of [a, b) join a list of 12 bytes per
    site that stays resident), and after the last range levels() (rmr_kmer_levels_from_sites, whose sort buffers keep to
    max_resident_bases * LEVEL_SORT_BYTES: k-mers in groups).  Same bytes out as the one pass, whatever the cuts."""

    def __init__(self, engine, kmer_context_bases, min_cov=10, max_resident_bases=None):
        self.engine = engine
        self.kb, self.ka = int(kmer_context_bases[0]), int(kmer_context_bases[1])
        if self.kb < 0 or self.ka < 0 or self.kb + self.ka + 1 > MAX_LEVEL_KMER:
            raise RemoraError(f"k-mer levels are estimated for k-mers of up to {MAX_LEVEL_KMER} bases")
        self.min_cov = int(min_cov)
        self._vals, self._seq, self._key0, self._lens = [], [], [], []
        self._n = 0
        self.max_resident_bases = None if max_resident_bases is None else int(max_resident_bases)
        if self.max_resident_bases is not None and self.max_resident_bases < 1:
            raise RemoraError("k-mer levels: max_resident_bases must be positive")
        self._range = None
        self._list_kmer = self._list_level = self._site_counts = None
        self.n_sites = 0  # entries of the lists
        self.range_sites = []  # how many every finished range appended
        self.n_kmer_groups = None  # of the last levels() over the lists

    @property
    def kmer_len(self):
        return self.kb + self.ka + 1

    def add(self, trimmean, int_seq, key0, seq_len):
        """One batch: trimmean f64[n_bases] and int_seq i8[n_bases] (device tensors, read orientation, reads back to back),
        key0 / seq_len int64[n_reads] (host: site_key0 and the reads' base counts)."""
        import torch

        if self.max_resident_bases is not None:
            if self._range is None:
                raise RemoraError("k-mer levels in ranges: begin_range() comes before add()")
            a, b = self._range
            trimmean, int_seq, key0, seq_len = clip_to_key_range(trimmean, int_seq, key0, seq_len, a - self.kb, b + self.ka)
            if not int(np.sum(seq_len)):
                return
            self._n += int(np.sum(seq_len))
            if self._n > self.max_resident_bases:
                raise RemoraError(f"k-mer levels: the range [{a}, {b}) was planned for at most {self.max_resident_bases} bases and holds "
                                  f"{self._n}: the reads are not the ones the ranges were planned from")
        else:
            self._n += int(np.sum(seq_len))
            need, have = self._n * LEVEL_BYTES_PER_BASE, torch.cuda.mem_get_info(self.engine.torch_device)[1]
            if need > have:  # said while the pass can still be stopped cheaply, not by a failed allocation after it
                raise RemoraError(f"k-mer levels keep every base of the input on the device ({LEVEL_BYTES_PER_BASE} B per base): {self._n} bases so "
                                  f"far need {need / 2**30:.1f} GiB, the device has {have / 2**30:.1f} GiB; estimate from a subset of the reads")
        self._vals.append(trimmean)
        self._seq.append(int_seq)
        self._key0.append(np.asarray(key0, np.int64))
        self._lens.append(np.asarray(seq_len, np.int64))

    def _observations(self):
        """The batches held as one: n_reads, d_seq_off, d_key0, n, vals, seq (device tensors)."""
        import torch

        dev = self.engine.torch_device
        lens = np.concatenate(self._lens) if self._lens else np.zeros(0, np.int64)
        seq_off = np.zeros(lens.size + 1, np.int64)
        np.cumsum(lens, out=seq_off[1:])
        n = int(seq_off[-1])
        vals = torch.cat(self._vals) if n else torch.zeros(1, dtype=torch.float64, device=dev)
        seq = torch.cat(self._seq) if n else torch.zeros(1, dtype=torch.int8, device=dev)
        self._vals, self._seq = ([vals], [seq]) if n else ([], [])  # one copy stays; the batches' blocks go back to the allocator
        free, _ = torch.cuda.mem_get_info(dev)
        if n * 33 > free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev):
            raise RemoraError(f"k-mer levels: sorting {n} bases needs {n * 33 / 2**30:.1f} GiB more device memory, {free / 2**30:.1f} GiB are free")
        torch.cuda.empty_cache()  # the sort buffers are the library's own allocations, not the caching allocator's
        d_off = torch.from_numpy(seq_off).to(dev)
        d_key0 = torch.from_numpy(np.concatenate(self._key0) if self._key0 else np.zeros(1, np.int64)).to(dev)
        return int(lens.size), d_off, d_key0, n, vals, seq

    def begin_range(self, a, b):
        """The next range of site keys [a, b); the ranges of a run do not overlap."""
        if self.max_resident_bases is None:
            raise RemoraError("k-mer levels: ranges need a SiteLevels made with max_resident_bases")
        if self._range is not None:
            raise RemoraError("k-mer levels in ranges: end_range() comes before the next begin_range()")
        if not 0 <= int(a) < int(b):
            raise RemoraError(f"k-mer levels: [{a}, {b}) is no range of site keys")
        self._range = (int(a), int(b))

    def end_range(self):
        """Stage 1 over what add() kept for the range.  -> number of sites the range reported."""
        import torch

        if self._range is None:
            raise RemoraError("k-mer levels in ranges: begin_range() comes before end_range()")
        a, b = self._range
        dev = self.engine.torch_device
        if self._site_counts is None:
            self._site_counts = torch.zeros(4**self.kmer_len, dtype=torch.int64, device=dev)
        took = ctypes.c_int64(0)
        if self._n:
            n_reads, d_off, d_key0, n, vals, seq = self._observations()
            room = self.n_sites + min(n, b - a)
            if self._list_kmer is None or room > self._list_kmer.numel():
                cap = max(room, 2 * self.n_sites)
                kmer, level = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.float64, device=dev)
                if self.n_sites:
                    kmer[: self.n_sites], level[: self.n_sites] = self._list_kmer[: self.n_sites], self._list_level[: self.n_sites]
                self._list_kmer, self._list_level = kmer, level
            torch.cuda.current_stream(dev).synchronize()  # the inputs were made on torch's stream, the kernels run on the engine's
            L.check(L.lib().rmr_site_medians(self.engine.handle, n_reads, d_off.data_ptr(), d_key0.data_ptr(), n, vals.data_ptr(), seq.data_ptr(),
                                             self.kb, self.ka, self.min_cov, a, b, self._list_kmer.data_ptr(), self._list_level.data_ptr(),
                                             self.n_sites, self._list_kmer.numel(), self._site_counts.data_ptr(), ctypes.byref(took)))
        self.n_sites += took.value
        self.range_sites.append(took.value)
        self._vals, self._seq, self._key0, self._lens, self._n, self._range = [], [], [], [], 0, None
        return took.value

    def levels(self, want_sites=False):
        """-> levels f64[4^k] (NaN: k-mer without a site), sites per k-mer i64[4^k]; with `want_sites` also the reported sites'
        k-mer index i32[n] and level f64[n], ordered by (k-mer, level).  numpy arrays."""
        import torch

        dev = self.engine.torch_device
        nk = 4**self.kmer_len
        levels = torch.empty(nk, dtype=torch.float64, device=dev)
        counts = torch.empty(nk, dtype=torch.int64, device=dev)
        if self.max_resident_bases is not None:
            if self._range is not None:
                raise RemoraError("k-mer levels in ranges: end_range() comes before levels()")
            n = self.n_sites
            site_counts = self._site_counts if self._site_counts is not None else torch.zeros(nk, dtype=torch.int64, device=dev)
            site_kmer = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_sites else None
            site_level = torch.empty(max(n, 1), dtype=torch.float64, device=dev) if want_sites else None
            groups = ctypes.c_int64(0)
            torch.cuda.empty_cache()
            torch.cuda.current_stream(dev).synchronize()
            L.check(L.lib().rmr_kmer_levels_from_sites(self.engine.handle, n, self._list_kmer.data_ptr() if n else None,
                                                       self._list_level.data_ptr() if n else None, self.kmer_len, site_counts.data_ptr(),
                                                       self.max_resident_bases * LEVEL_SORT_BYTES, levels.data_ptr(), counts.data_ptr(),
                                                       site_kmer.data_ptr() if want_sites else None,
                                                       site_level.data_ptr() if want_sites else None, ctypes.byref(groups)))
            self.n_kmer_groups = groups.value
            n_sites = ctypes.c_int64(n)
        else:
            n_reads, d_off, d_key0, n, vals, seq = self._observations()
            site_kmer = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_sites else None
            site_level = torch.empty(max(n, 1), dtype=torch.float64, device=dev) if want_sites else None
            n_sites = ctypes.c_int64(0)
            torch.cuda.current_stream(dev).synchronize()  # the inputs were made on torch's stream, the kernels run on the engine's
            L.check(L.lib().rmr_site_kmer_levels(self.engine.handle, n_reads, d_off.data_ptr(), d_key0.data_ptr(), n, vals.data_ptr(),
                                                 seq.data_ptr(), self.kb, self.ka, self.min_cov, levels.data_ptr(), counts.data_ptr(),
                                                 site_kmer.data_ptr() if want_sites else None,
                                                 site_level.data_ptr() if want_sites else None, ctypes.byref(n_sites)))
        out = (levels.cpu().numpy(), counts.cpu().numpy())
        if want_sites:
            out += (site_kmer[: n_sites.value].cpu().numpy(), site_level[: n_sites.value].cpu().numpy())
        return out


def kmer_strings(kmer_len):
    """All k-mers over ACGT in the order of the table's index (and of sorted())."""
    from itertools import product

    return ["".join(bs) for bs in product("ACGT", repeat=kmer_len)]
