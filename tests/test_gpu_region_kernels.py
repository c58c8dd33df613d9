"""base_metrics_kernel, region_metrics_kernel and region_signals_kernel (csrc/k_metrics.hip) driven through the C ABI
(rmr_base_metrics, rmr_region_base_metrics, rmr_region_signals) on the synthetic reads of tests/metric_cases.py - not through
DeviceReads.region_metrics / region_signals, whose checks and NaN pre-fill hide what the kernels do themselves: their NaN fill,
their group geometry past blockIdx.y == 1, their own refusals (status 1 and 2) and what they leave untouched.  Every output is
filled with a sentinel before the launch and has guard entries on both sides."""
import ctypes

import numpy as np
import pytest

import metric_cases as mc
from metrics_exact import mean_bound, var_bound

pytestmark = pytest.mark.gpu

SEED = 20
SENT = -7.25                       # no value and no NaN the kernels write
SENT_I64 = 0x7EAD_BEEF_0BAD_F00D
SENT_I16 = 12345                   # no sample of the synthetic reads (-600 .. 1599, -32768, 32767)
SENT_STATUS = 77
OUTPUTS = ("dwell", "mean", "sd", "trimmean", "trimsd")
WHOLE_TRIMS = ((0, 0), (1, 1), (0, 3), (6000, 6000))
REGION_TRIMS = ((0, 0), (1, 1), (0, 3))
SLACK = 64  # entries of mapping and samples on either side of the padded copies (one entry for the per-read arrays)


class _R:
    """What DeviceReads gathers from."""

    def __init__(self, dacs, seq_to_sig, shift, scale):
        self.dacs, self.seq_to_sig_map, self.shift, self.scale = dacs, np.asarray(seq_to_sig, np.int64), float(shift), float(scale)
        self.int_seq, self.read_id = np.zeros(self.seq_to_sig_map.size - 1, np.int8), None


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


class _Batch:
    """The synthetic reads and their dirty twins resident as one batch, the device pointers of its arrays (`plain`), and a second
    copy of every array with slack on both sides (`padded`): a read in front of the batch and one behind it, of 10 bases each,
    whose mapping (zeros) and samples lie in the slack, so that a pair a guard wrongly lets through stays inside the allocations
    and shows as a written sentinel."""

    def __init__(self, torch):
        from remora_amd.data_chunks import DeviceReads

        self.torch = torch
        self.clean, self.twins = mc.synthetic_reads(SEED)
        self.reads = self.clean + [t[1] for t in self.twins]
        self.twin_at = [len(self.clean) + j for j in range(len(self.twins))]
        self.dr = dr = DeviceReads([_R(*r) for r in self.reads])
        dr.wait_ready()
        self.eng, self.dev, self.n = dr.engine, dr.engine.torch_device, dr.n_reads
        self.nb = np.diff(dr.seq_off)
        self.plain = tuple(t.data_ptr() for t in (dr.dacs, dr.d_sig_off, dr.s2s, dr.d_seq_off, dr.shift, dr.scale))
        s2s = np.concatenate([r[1] for r in self.reads])
        assert np.array_equal(dr.s2s.cpu().numpy(), s2s) and np.array_equal(dr.dacs.cpu().numpy(), np.concatenate([r[0] for r in self.reads]))
        z = lambda k, dt: np.zeros(k, dt)  # noqa: E731
        host = (np.concatenate([z(SLACK, np.int16)] + [r[0] for r in self.reads] + [z(SLACK, np.int16)]),
                np.concatenate([[-SLACK], dr.sig_off, [dr.sig_off[-1] + SLACK]]).astype(np.int64),
                np.concatenate([z(SLACK, np.int64), s2s, z(SLACK, np.int64)]),
                np.concatenate([[-10], dr.seq_off, [dr.seq_off[-1] + 10]]).astype(np.int64),
                np.array([0.0] + [r[2] for r in self.reads] + [0.0]), np.array([1.0] + [r[3] for r in self.reads] + [1.0]))
        self._padded = [torch.from_numpy(h).to(self.dev) for h in host]
        self.padded = tuple(t.data_ptr() + lead * t.element_size() for t, lead in zip(self._padded, (SLACK, 1, SLACK, 1, 1, 1)))
        self._whole, self._region = {}, {}

    # ---- rmr_base_metrics -------------------------------------------------------------------------------------------------
    def whole(self, trim):
        """All five outputs of rmr_base_metrics for the batch at `trim`: {name: [per-read arrays]}; computed once."""
        from remora_amd import _lib as L

        if trim not in self._whole:
            torch, n = self.torch, int(self.dr.seq_off[-1])
            out = {k: torch.full((n + 1,), SENT, dtype=torch.float32 if k == "dwell" else torch.float64, device=self.dev) for k in OUTPUTS}
            torch.cuda.current_stream(self.dev).synchronize()
            L.check(L.lib().rmr_base_metrics(self.eng.handle, self.n, *self.plain, int(self.nb.max()), trim[0], trim[1],
                                             *(out[k].data_ptr() for k in OUTPUTS)))
            self.eng.synchronize()
            got = {k: v.cpu().numpy() for k, v in out.items()}
            for k, v in got.items():
                assert v[n] == SENT and not (v[:n] == SENT).any(), k  # every base written, nothing behind the last
            off = self.dr.seq_off
            self._whole[trim] = {k: [v[off[i] : off[i + 1]] for i in range(self.n)] for k, v in got.items()}
        return self._whole[trim]

    # ---- rmr_region_base_metrics --------------------------------------------------------------------------------------------
    def region(self, src, pairs, trim, rows, width, names=OUTPUTS, split=None):
        """One launch over `pairs` (or, `split`: one launch per pair in that order, each with its own max_pair_bases) into
        sentinel-filled outputs.  -> ({name: float64 [1 + rows + 1, width], a slack row on either side}, status int32 [1 + n + 1])."""
        from remora_amd import _lib as L

        torch = self.torch
        full = np.zeros((len(pairs), 8), np.int64)
        full[:, :7] = pairs
        d_pairs = torch.from_numpy(full).to(self.dev)
        out = {k: torch.full((rows + 2, width), SENT, dtype=torch.float64, device=self.dev) for k in names}
        status = torch.full((len(pairs) + 2,), SENT_STATUS, dtype=torch.int32, device=self.dev)
        ptr = lambda k: ctypes.c_void_p(out[k].data_ptr() + width * 8) if k in out else None  # noqa: E731
        torch.cuda.current_stream(self.dev).synchronize()
        span = full[:, 2] - full[:, 1]
        for sel in ([slice(None)] if split is None else [slice(p, p + 1) for p in split]):
            first = 0 if split is None else sel.start
            L.check(L.lib().rmr_region_base_metrics(self.eng.handle, self.n, *src, len(full[sel]), d_pairs.data_ptr() + first * 64,
                                                    int(max(span[sel].max(), 1)), trim[0], trim[1], rows, width, *(ptr(k) for k in OUTPUTS),
                                                    status.data_ptr() + 4 * (1 + first)))
        self.eng.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}, status.cpu().numpy()

    def region_all(self, trim):
        """Every pair of mc.region_pairs in one launch, all five outputs; computed once per trim."""
        if trim not in self._region:
            pairs, rows, width = mc.region_pairs(self.clean)
            self._region[trim] = self.region(self.plain, pairs, trim, rows, width)
        return self._region[trim]


@pytest.fixture(scope="module")
def batch():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _Batch(torch)


@pytest.fixture(scope="module")
def exact(batch):
    """{trim: [per read: (dwell, base list)]} of mc.per_base_exact; the all-trimming trim has no base."""
    return {trim: [mc.per_base_exact(r, *trim) for r in batch.reads] for trim in WHOLE_TRIMS}


# ---- 1. whole reads ---------------------------------------------------------------------------------------------------------------
def test_whole_reads_against_the_exact_sums(batch, exact):
    """rmr_base_metrics on the synthetic batch at four trims: dwell equal, NaN exactly where a base has no samples of its own,
    |gpu - exact| <= mean_bound for mean and trimmean, |gpu^2 - var| <= var_bound for sd and trimsd (tests/metrics_exact.py), for
    every base; and the dirty twins base by base against their clean reads."""
    worst = {"mean": 0.0, "var": 0.0}
    checked = 0
    for trim in WHOLE_TRIMS:
        got = batch.whole(trim)
        for i in range(batch.n):
            dwell, _ = exact[trim][i]
            assert got["dwell"][i].dtype == np.float32 and np.array_equal(got["dwell"][i], dwell), (trim, i)
            for mname, sname, key in (("mean", "sd", (0, 0)), ("trimmean", "trimsd", trim)):
                bases = exact[key][i][1]
                has = np.zeros(dwell.size, bool)
                has[np.array([b[0] for b in bases], np.int64)] = True
                g_m, g_s = got[mname][i], got[sname][i]
                assert np.array_equal(~np.isnan(g_m), has) and np.array_equal(~np.isnan(g_s), has), (trim, i, mname)
                assert not np.isinf(g_m).any() and not np.isinf(g_s).any()
                for base, n, mean, var, sabs, ssq in bases:
                    bm, bv = mean_bound(n, sabs), var_bound(n, ssq, mean)
                    em, ev = abs(g_m[base] - mean), abs(g_s[base] ** 2 - var)
                    worst["mean"], worst["var"] = max(worst["mean"], em / bm), max(worst["var"], ev / bv)
                    assert em <= bm and ev <= bv, (trim, i, mname, base, em, bm, ev, bv)
                    checked += 1
        assert np.isnan(np.concatenate(got["trimmean"])).all() == (trim == (6000, 6000))
    print("bases checked:", checked, "worst error / bound:", worst)
    assert checked > 10000 and max(worst.values()) <= 1.0, worst
    # the 5000-sample base is one of them, and untrimmed means do not depend on the trims
    assert np.isfinite(batch.whole((1, 1))["trimsd"][mc.LONG_BASE_READ][mc.LONG_BASE])
    for trim in WHOLE_TRIMS[1:]:
        for k in ("mean", "sd"):
            assert np.array_equal(_bits(np.concatenate(batch.whole(trim)[k])), _bits(np.concatenate(batch.whole((0, 0))[k])))
    # the dirty twins
    for at, (of, dirty, changed) in zip(batch.twin_at, batch.twins):
        mp = dirty[1]
        touched = sorted({b for e in changed for b in (e - 1, e) if 0 <= b < mp.size - 1})
        same = np.ones(mp.size - 1, bool)
        same[touched] = False
        for trim in WHOLE_TRIMS[:3]:
            got = batch.whole(trim)
            for k in OUTPUTS:
                assert np.array_equal(_bits(got[k][at][same]), _bits(got[k][of][same])), (at, trim, k)
            for k in OUTPUTS[1:]:
                assert np.isnan(got[k][at][touched]).all(), (at, trim, k)
            assert np.array_equal(got["dwell"][at][touched], (mp[1:] - mp[:-1])[touched].astype(np.float32))
    back = batch.whole((1, 1))["dwell"][batch.twin_at[1]]
    assert (back[[mc.BACK_AT, mc.BACK_AT + 1]] < 0).all()


# ---- 2. every region pair in one launch ---------------------------------------------------------------------------------------------
def _region_expected(batch, trim, pairs, rows, width):
    """{name: float64 [1 + rows + 1, width]}: the whole-read arrays of rmr_base_metrics placed by numpy, sentinel rows around."""
    want = {}
    for k in OUTPUTS:
        body = mc.region_rows_expected(batch.whole(trim)[k], pairs, rows, width)
        used = np.zeros(rows, bool)
        used[np.asarray(pairs)[:, 4]] = True
        body[~used] = SENT
        want[k] = np.concatenate([np.full((1, width), SENT), body, np.full((1, width), SENT)])
    return want


@pytest.mark.parametrize("trim", REGION_TRIMS, ids=lambda t: f"trim{t[0]}_{t[1]}")
def test_every_pair_in_one_launch_equals_the_whole_read_bits(batch, trim):
    """All pairs of mc.region_pairs, from 1 to 513 bases, in one launch sized by the longest: every entry of every row is the
    bit pattern rmr_base_metrics gives that base (dwell widened), every other column up to `width` is the kernel's own NaN - the
    outputs start as a sentinel -, the rows in front of and behind the output stay sentinel, every status is 0; and the same for
    each output alone with the other four pointers NULL."""
    pairs, rows, width = mc.region_pairs(batch.clean)
    got, status = batch.region_all(trim)
    want = _region_expected(batch, trim, pairs, rows, width)
    assert status[0] == status[-1] == SENT_STATUS and not status[1:-1].any()
    for k in OUTPUTS:
        assert not (got[k][1:-1] == SENT).any(), k  # the NaN fill of block y == 0 reached every column the read does not cover
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:5])
    assert np.isfinite(got["trimmean"]).sum() > 5000
    for k in OUTPUTS:
        alone, status = batch.region(batch.plain, pairs, trim, rows, width, names=(k,))
        assert list(alone) == [k] and not status[1:-1].any()
        assert np.array_equal(_bits(alone[k]), _bits(want[k])), k


# ---- 3. launch splitting ----------------------------------------------------------------------------------------------------------------
def test_one_launch_per_pair_gives_the_same_bytes(batch):
    """The same pairs one per launch, each with its own max_pair_bases (the launch grid as tight as the call allows: a span of n
    bases gets (n + 62) / 64 + 1 groups), forwards and in reverse order."""
    trim = (1, 1)
    pairs, rows, width = mc.region_pairs(batch.clean)
    want, _ = batch.region_all(trim)
    for order in (range(len(pairs)), range(len(pairs) - 1, -1, -1)):
        got, status = batch.region(batch.plain, pairs, trim, rows, width, split=list(order))
        assert status[0] == status[-1] == SENT_STATUS and not status[1:-1].any()
        for k in OUTPUTS:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (k, np.argwhere(_bits(got[k]) != _bits(want[k]))[:5])


# ---- 4. the kernel's own refusals ---------------------------------------------------------------------------------------------------------
def test_bad_pairs_get_status_one_and_write_nothing(batch):
    """include/remora_hip.h: "a pair is used only if 0 <= first < last <= bases of its read, lead + (last - first) <= region
    length <= width and 0 <= row < rows; otherwise nothing is written for it and status[pair] = 1".  Pairs that are off by exactly
    one, among good ones, over the padded arrays: a guard that let one through would write into a sentinel row (or into the slack
    rows around the output) and report 0."""
    trim = (1, 1)
    pairs, rows, width = mc.region_pairs(batch.clean)
    good = pairs[np.r_[0:14, np.nonzero(pairs[:, 2] - pairs[:, 1] == 513)[0][1:2]]]  # (the first 513-base pair is among the 14)
    free = [r for r in range(rows) if r not in set(good[:, 4].tolist())]
    n, nb = batch.n, batch.nb
    last_read = n - 1
    bad = {
        "read = n_reads": [n, 0, 5, 0, free[0], 5, 0],
        "read = -1": [-1, 0, 5, 0, free[1], 5, 0],
        "last = nb + 1": [4, nb[4] - 3, nb[4] + 1, 0, free[2], 8, 0],
        "last = nb + 1 on the last read": [last_read, nb[last_read] - 3, nb[last_read] + 1, 0, free[3], 8, 1],
        "first = last": [4, 10, 10, 0, free[4], 5, 0],
        "first = -1": [0, -1, 1, 0, free[5], 5, 0],
        "lead = rlen - covered + 1": [4, 3, 9, 5, free[6], 10, 0],
        "lead = rlen - covered + 1, flipped": [4, 3, 9, 5, free[7], 10, 1],
        "lead = -1": [4, 3, 9, -1, free[8], 10, 0],
        "row = rows": [4, 3, 9, 0, rows, 10, 0],
        "row = -1": [4, 3, 9, 0, -1, 10, 1],
        "rlen = width + 1": [4, 3, 9, 0, free[9], width + 1, 0],
        "rlen = 0": [4, 3, 4, 0, free[10], 0, 0],
    }
    mixed = np.concatenate([good[:7], np.asarray(list(bad.values()), np.int64), good[7:]])
    is_bad = np.r_[np.zeros(7, bool), np.ones(len(bad), bool), np.zeros(len(good) - 7, bool)]
    got, status = batch.region(batch.padded, mixed, trim, rows, width)
    assert status[0] == status[-1] == SENT_STATUS
    assert status[1:-1].tolist() == is_bad.astype(int).tolist(), dict(zip(bad, status[8 : 8 + len(bad)].tolist()))
    all_rows, _ = batch.region_all(trim)
    for k in OUTPUTS:
        want = np.full_like(all_rows[k], SENT)
        want[1 + good[:, 4]] = all_rows[k][1 + good[:, 4]]
        assert np.array_equal(_bits(got[k]), _bits(want)), (k, np.argwhere(_bits(got[k]) != _bits(want))[:5])


# ---- 5. rmr_region_signals ----------------------------------------------------------------------------------------------------------------
def _signals(batch, src, entries, raw, short_sig=0, short_map=0):
    """One launch of rmr_region_signals.  entries: (pair, samples of its slot, mapping entries of its slot).  The outputs have
    one guard entry behind their capacity (`short_*`: the capacity handed over is that much less than the slots need).
    -> (sig, sig_off, map, map_off, sig_start, status), the first and third with their guard."""
    from remora_amd import _lib as L

    torch, dev = batch.torch, batch.dev
    full = np.zeros((len(entries), 8), np.int64)
    full[:, :7] = [e[0] for e in entries]
    sig_off, map_off = (np.concatenate([[0], np.cumsum([e[j] for e in entries])]).astype(np.int64) for j in (1, 2))
    sig = torch.full((int(sig_off[-1]) + 1,), SENT_I16 if raw else SENT, dtype=torch.int16 if raw else torch.float64, device=dev)
    smap = torch.full((int(map_off[-1]) + 1,), SENT_I64, dtype=torch.int64, device=dev)
    start = torch.full((len(entries) + 1,), SENT_I64, dtype=torch.int64, device=dev)
    status = torch.full((len(entries) + 1,), SENT_STATUS, dtype=torch.int32, device=dev)
    d_pairs, d_so, d_mo = (torch.from_numpy(x).to(dev) for x in (full, sig_off, map_off))
    torch.cuda.current_stream(dev).synchronize()
    L.check(L.lib().rmr_region_signals(batch.eng.handle, batch.n, *src, len(entries), d_pairs.data_ptr(), d_so.data_ptr(), d_mo.data_ptr(),
                                       int(raw), sig.data_ptr(), int(sig_off[-1]) - short_sig, smap.data_ptr(), int(map_off[-1]) - short_map,
                                       start.data_ptr(), status.data_ptr()))
    batch.eng.synchronize()
    return sig.cpu().numpy(), sig_off, smap.cpu().numpy(), map_off, start.cpu().numpy(), status.cpu().numpy()


def _check_signals(batch, entries, want_status, got, raw):
    sig, sig_off, smap, map_off, start, status = got
    sent = SENT_I16 if raw else SENT
    assert sig[-1] == sent and smap[-1] == SENT_I64 and start[-1] == SENT_I64 and status[-1] == SENT_STATUS
    assert status[:-1].tolist() == list(want_status)
    for p, ((pair, _, _), st) in enumerate(zip(entries, want_status)):
        s, m = sig[sig_off[p] : sig_off[p + 1]], smap[map_off[p] : map_off[p + 1]]
        if st:  # a refused pair writes nothing
            assert (s == sent).all() and (m == SENT_I64).all() and start[p] == SENT_I64, (p, pair)
            continue
        w_sig, w_map, w_start = mc.signals_expected(batch.reads[pair[0]], pair, raw)
        assert s.dtype == w_sig.dtype and np.array_equal(s, w_sig) and np.array_equal(m, w_map) and start[p] == w_start, (p, pair)


def _slot(batch, pair):
    mp = batch.reads[pair[0]][1]
    return (list(pair), int(mp[pair[2]] - mp[pair[1]]), int(pair[2] - pair[1] + 1))


@pytest.mark.parametrize("raw", [False, True], ids=["normalised", "raw"])
def test_region_signals_of_every_planned_size(batch, raw):
    """Spans of 0, 1, 255, 256, 2047, 2048, 2049 and more than 5000 samples and of 2, 256, 257 and more than 2048 mapping entries
    (the 8 x 256 threads of a pair take a second trip above 2048), forward and flipped: samples, mapping entries and sig_start
    equal the header's rule exactly, the entry behind either capacity is still the guard.  lead, row and region length are not
    looked at."""
    pairs = mc.signal_pairs(batch.clean).tolist() + [[1, 3, 9, -4, -1, 0, 0]]
    entries = [_slot(batch, p) for p in pairs]
    got = _signals(batch, batch.plain, entries, raw)
    _check_signals(batch, entries, [0] * len(entries), got, raw)
    assert got[1][-1] > 30000 and got[3][-1] > 5000


@pytest.mark.parametrize("raw", [False, True], ids=["normalised", "raw"])
def test_region_signals_refusals_write_nothing(batch, raw):
    """Status 2 where the mapping leaves the read's signal at either end of the span or runs backwards over it (the dirty twins),
    status 1 for a span that does not fit its read, for a slot of either output that is one entry too long or too short, and for
    a slot that ends beyond either capacity; a refused pair leaves its slots and its sig_start untouched and its neighbours
    are what they are without it.  Over the padded arrays."""
    ends, back = batch.twin_at
    nb, j = batch.nb, mc.BACK_AT
    sp = mc.signal_pairs(batch.clean)
    good = [_slot(batch, p) for p in sp[[2, 3, 8, 9, 20, 21]].tolist()]
    g0 = good[3]
    refused = [
        (([ends, 0, 3, 0, 0, 0, 0], 4, 4), 2),                       # map[first] = -3
        (([ends, nb[ends] - 3, nb[ends], 0, 0, 0, 1], 4, 4), 2),     # map[last] = sig_len + 5
        (([back, j, j + 2, 0, 0, 0, 0], 4, 3), 2),                   # backwards across both bases
        (([back, j, j + 1, 0, 0, 0, 1], 4, 2), 2),
        (([batch.n, 0, 5, 0, 0, 0, 0], 4, 6), 1),                    # the checks of the span, each off by one
        (([-1, 0, 5, 0, 0, 0, 0], 4, 6), 1),
        (([4, nb[4] - 3, nb[4] + 1, 0, 0, 0, 0], 4, 5), 1),
        (([0, -1, 1, 0, 0, 0, 0], 4, 3), 1),
        (([4, 10, 10, 0, 0, 0, 0], 4, 1), 1),
        ((g0[0], g0[1] + 1, g0[2]), 1),                              # sig_out_off[p + 1] - sig_out_off[p] off by one
        ((g0[0], g0[1] - 1, g0[2]), 1),
        ((g0[0], g0[1], g0[2] + 1), 1),                              # map_out_off off by one
        ((g0[0], g0[1], g0[2] - 1), 1),
    ]
    assert g0[1] > 1
    entries, want = [], []
    for k, (e, st) in enumerate(refused):
        entries += [good[k % len(good)], e]
        want += [0, st]
    entries.append(good[0])
    want.append(0)
    assert entries[-1][1] >= 1
    _check_signals(batch, entries, want, _signals(batch, batch.padded, entries, raw), raw)
    # the last pair's slots end one entry beyond the capacity of the samples, then of the mapping
    _check_signals(batch, entries, want[:-1] + [1], _signals(batch, batch.padded, entries, raw, short_sig=1), raw)
    _check_signals(batch, entries, want[:-1] + [1], _signals(batch, batch.padded, entries, raw, short_map=1), raw)


# ---- 6. the profiler slots ----------------------------------------------------------------------------------------------------------------------
def test_each_call_is_one_launch_and_no_pairs_none(batch):
    from remora_amd import _lib as L

    pairs, rows, width = mc.region_pairs(batch.clean)
    eng = batch.eng
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        batch.region(batch.plain, pairs, (1, 1), rows, width)
        _signals(batch, batch.plain, [_slot(batch, p) for p in mc.signal_pairs(batch.clean).tolist()], False)
        prof = eng.profile()
        assert prof["region_metrics"][1] == 1 and prof["region_signals"][1] == 1, prof
        assert L.lib().rmr_region_base_metrics(eng.handle, batch.n, *batch.plain, 0, None, 1, 1, 1, rows, width, None, None, None, None, None, None) == 0
        assert L.lib().rmr_region_signals(eng.handle, batch.n, *batch.plain, 0, None, None, None, 0, None, 0, None, 0, None, None) == 0
        eng.synchronize()
        prof = eng.profile()
        assert prof["region_metrics"][1] == 1 and prof["region_signals"][1] == 1, prof
    finally:
        eng.profile_enable(False)
