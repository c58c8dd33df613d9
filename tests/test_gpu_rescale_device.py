"""Iterative signal-mapping refiners (scale_iters > 0) on a resident batch: the two kernels behind
SigMapRefiner.rescale_device (rmr_rescale_points, rmr_theil_sen_fit; csrc/k_refine.hip) against the host functions they
restate (SigMapRefiner.rescale, theil_sen), refine_device_reads against refine_reads, and the commands that used to send such
a refiner read by read against that path.  Every comparison is equality of bits."""
import ctypes
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")
TABLE = os.path.join(DATA, "levels_4mer.txt")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _refiner(**kw):
    from remora_amd.refine_signal_map import SigMapRefiner

    return SigMapRefiner(kmer_model_filename=TABLE, do_fix_guage=True, **kw)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    """Equal float64 bits, any NaN standing for any NaN."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


def _synth(ref, seed, nb, zero_frac=0.0, stalls=0, jitter=True, idx=0, noise=0.2):
    """A read whose samples follow the table's levels (dwells 2..15) and whose mapping is off by a few samples per base."""
    from remora_amd.data_chunks import RemoraRead

    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 4, nb)
    dwell = rng.integers(2, 16, nb)
    if zero_frac:
        dwell[rng.random(nb) < zero_frac] = 0
        dwell[0], dwell[-1] = max(dwell[0], 1), max(dwell[-1], 1)
    if stalls:
        dwell[rng.choice(np.arange(12, nb - 12), stalls, replace=False)] = 200 + 37 * np.arange(stalls)
    m = np.concatenate([[0], np.cumsum(dwell)]).astype(np.int64)
    norm = np.repeat(ref.extract_levels(seq).astype(np.float64), dwell) + noise * rng.standard_normal(m[-1])
    dacs = np.round(500 + 80 * norm).astype(np.int16)
    if jitter:
        j = m.copy()
        j[1:-1] += rng.integers(-3, 4, nb - 1)
        j = np.maximum.accumulate(np.clip(j, m[0], m[-1] - 1))  # (the last base keeps a sample: the rough re-scale reads its centre)
        j[0], j[-1] = m[0], m[-1]
        m = j
    return RemoraRead(dacs=dacs, shift=497.0 + (idx % 5), scale=83.5 - (idx % 3), seq_to_sig_map=m, int_seq=seq, read_id=f"s{nb}_{idx}")


# ---- 1. rmr_theil_sen_fit ------------------------------------------------------------------------------------------------
def _host_medians(x, y):
    """The first two statements of theil_sen (remora_amd/refine_signal_map.py)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # the median of nothing
        dx = x[:, np.newaxis] - x
        dy = y[:, np.newaxis] - y
        keep = dx > 0
        slope = np.median(dy[keep] / dx[keep])
        inter = np.median(y - slope * x)
    return slope, inter, int(keep.sum())


def _fit_cases():
    rng = np.random.default_rng(20)
    cases = []
    for m in (2, 3, 4, 11, 999):
        x = rng.standard_normal(m)
        cases.append((f"m{m}", x, (0.9 * x + 0.1 + 0.3 * rng.standard_normal(m)).astype(np.float32), None))
        if m == 11:  # the read that is not live stands here, with points of its own
            cases.append(("dead", x + 1.0, cases[-1][2] * 2, None))
    x = rng.standard_normal(1500)
    cases.append(("sampled", x, (1.1 * x - 0.2 + 0.3 * rng.standard_normal(1500)).astype(np.float32),
                  np.random.RandomState(4).choice(1500, 1000, replace=False).astype(np.int32)))
    x = np.array([0.5, 0.5, -1.25, 2.0])  # 6 pairs, one of them tied: 5 slopes
    cases.append(("one tie", x, np.array([0.1, 0.4, -1.0, 2.5], np.float32), None))
    x = rng.integers(0, 7, 60) / 4.0
    cases.append(("many ties", x, (x + 0.4 * rng.standard_normal(60)).astype(np.float32), None))
    cases.append(("all x equal", np.full(12, 0.25), np.linspace(-1, 1, 12).astype(np.float32), None))
    cases.append(("y constant", rng.standard_normal(15), np.full(15, 0.75, np.float32), None))
    return cases


def test_theil_sen_fit_equals_the_host_medians(torch_cuda):
    """Odd and even pair counts, 999 points, 1000 of 1500 through a drawn sample, ties that drop pairs, no pair at all, a zero
    slope, and a read that is not live between two that are: slope and intercept are np.median's bits."""
    from remora_amd import _lib as L

    torch = torch_cuda
    ref = _refiner(scale_iters=1)
    dev = ref._device_refiner(0)
    tdev = dev.engine.torch_device
    cases = _fit_cases()
    dead = [c[0] for c in cases].index("dead")
    assert 0 < dead < len(cases) - 1
    room = [c[1].size + 3 for c in cases]  # bases of the read: more than its points
    seq_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    n = len(cases)
    x, y = np.full(seq_off[-1], np.nan), np.full(seq_off[-1], np.nan, np.float32)
    count, live = np.zeros(n, np.int32), np.ones(n, np.uint8)
    samp, samp_off = [np.full(1000, -1, np.int32)], np.full(n, -1, np.int64)  # (a leading block nobody points to)
    for i, (_, cx, cy, pick) in enumerate(cases):
        x[seq_off[i] : seq_off[i] + cx.size], y[seq_off[i] : seq_off[i] + cx.size] = cx, cy
        count[i] = cx.size
        if pick is not None:
            samp_off[i] = 1000 * len(samp)
            samp.append(pick)
    live[dead] = 0
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(tdev)  # noqa: E731
    d_x, d_y, d_count, d_off, d_samp, d_samp_off, d_live = (up(a) for a in (x, y, count, seq_off, np.concatenate(samp), samp_off, live))
    slope = torch.full((n,), -123.5, dtype=torch.float64, device=tdev)
    inter = torch.full((n,), -321.5, dtype=torch.float64, device=tdev)
    status = torch.full((n,), -9, dtype=torch.int32, device=tdev)
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    L.check(dev._lib.rmr_theil_sen_fit(dev._h, n, p(d_x), p(d_y), p(d_count), p(d_off), p(d_samp), p(d_samp_off), d_samp.numel(), p(d_live),
                                       p(slope), p(inter), p(status)))
    dev.engine.synchronize()
    slope, inter, status = slope.cpu().numpy(), inter.cpu().numpy(), status.cpu().numpy()
    parities = set()
    for i, (name, cx, cy, pick) in enumerate(cases):
        if i == dead:
            assert (slope[i], inter[i], status[i]) == (-123.5, -321.5, -9), "a read that is not live was written"
            continue
        if pick is not None:
            cx, cy = cx[pick], cy[pick]
        want_slope, want_inter, pairs = _host_medians(cx, cy)
        print(name, "pairs", pairs, "slope", slope[i], want_slope, "inter", inter[i], want_inter, "status", status[i])
        parities.add((name, pairs % 2))
        assert status[i] == (1 if pairs == 0 else 2 if want_slope == 0 else 0), name
        assert _same(slope[i], want_slope) and _same(inter[i], want_inter), name
    assert status[[c[0] for c in cases].index("all x equal")] == 1 and status[[c[0] for c in cases].index("y constant")] == 2
    assert ("one tie", 1) in parities and {p for _, p in parities} == {0, 1}
    # without the sample, or with one that does not lie inside `samp`, a read above 1000 points is refused, not fitted through
    # something else
    slope2, inter2 = torch.zeros(n, dtype=torch.float64, device=tdev), torch.zeros(n, dtype=torch.float64, device=tdev)
    for sample in ((None, None, 0), (p(d_samp), p(d_samp_off), d_samp.numel() - 1)):
        status = torch.full((n,), -9, dtype=torch.int32, device=tdev)
        torch.cuda.synchronize()
        L.check(dev._lib.rmr_theil_sen_fit(dev._h, n, p(d_x), p(d_y), p(d_count), p(d_off), *sample, p(d_live), p(slope2), p(inter2), p(status)))
        dev.engine.synchronize()
        assert status.cpu().numpy()[[c[0] for c in cases].index("sampled")] == 3


# ---- 2. rmr_rescale_points -----------------------------------------------------------------------------------------------
def _host_points(ref, r):
    """(count, norm_sig, levels) of the valid bases of the host `rescale` for the read as it stands: what it hands to
    rescale_theil_sen, or the count alone where it raises "Too few positions"."""
    import remora_amd.refine_signal_map as rsm

    class Got(Exception):
        pass

    def grab(dacs, levels, shift, scale):
        raise Got((dacs - shift) / scale, levels)

    seen = []
    real_ts, real_reduce = rsm.rescale_theil_sen, np.logical_and.reduce

    class Spy:
        def __getattr__(self, name):
            return getattr(np, name)

        class logical_and:  # noqa: N801
            @staticmethod
            def reduce(terms):
                seen.append(real_reduce(terms))
                return seen[-1]

    rsm.rescale_theil_sen, real_np, rsm.np = grab, rsm.np, Spy()
    try:
        s0 = r.seq_to_sig_map[0]
        ref.rescale(ref.extract_levels(r.int_seq), r.dacs[s0 : r.seq_to_sig_map[-1]], r.shift, r.scale, r.seq_to_sig_map - s0)
    except Got as g:
        return int(seen[0].sum()), g.args[0], g.args[1]
    except rsm.RemoraError:
        return int(seen[0].sum()), None, None
    finally:
        rsm.rescale_theil_sen, rsm.np = real_ts, real_np
    raise AssertionError("rescale returned")


def _golden_reads(ref_anchored=False):
    from remora_amd import io as rio

    out = []
    for read, err in rio.iter_reads_from_pod5_and_bam(os.path.join(DATA, "can_reads.pod5"), os.path.join(DATA, "can_mappings.bam"),
                                                      parse_ref_align=ref_anchored):
        if err is None:
            out.append(read.into_remora_read(ref_anchored))
    return out


def test_rescale_points_equal_the_host_rescale(torch_cuda):
    """count, x and y of every read against what the host `rescale` hands to rescale_theil_sen: real reads, reads shorter than
    the edge filter, reads with bases without samples, and a read whose 90th dwell percentile falls between 8 and a stall."""
    from remora_amd.data_chunks import DeviceReads

    ref = _refiner(scale_iters=1)
    reads = _golden_reads()[:4]
    reads += [_synth(ref, 30 + nb, nb, jitter=False, idx=k) for k, nb in enumerate((9, 15, 25, 60, 3000))]
    reads.append(_synth(ref, 41, 300, zero_frac=0.15, jitter=False, idx=7))
    stall = _synth(ref, 42, 60, stalls=6, jitter=False, idx=8)
    reads.append(stall)
    dwell = np.diff(stall.seq_to_sig_map)
    assert (dwell == 0).sum() == 0 and (np.diff(reads[-2].seq_to_sig_map) == 0).sum() >= 20
    p90 = np.percentile(dwell, 90)
    assert p90 != np.floor(p90) and np.sort(dwell)[53] < 16 and np.sort(dwell)[54] >= 200
    want = [_host_points(ref, r) for r in reads]
    counts = [w[0] for w in want]
    assert max(counts) > 1000 and any(10 <= c <= 1000 for c in counts) and any(c < 10 for c in counts)
    assert counts[4] == 0 and counts[5] == 0 and counts[6] <= 5  # 9 and 15 bases: nothing inside the edges; 25 bases: five
    dr = DeviceReads(reads)
    live = np.ones(len(reads), bool)
    live[1] = False
    ctx = ref._rescale_context(dr)
    ctx["count"].fill_(-4)
    got_counts = ref._rescale_points(dr, live, 10)
    x, y = ctx["x"].cpu().numpy(), ctx["y"].cpu().numpy()
    for i, (r, (cnt, norm_sig, levels)) in enumerate(zip(reads, want)):
        print(r.read_id, r.int_seq.size, "count", got_counts[i], cnt)
        if not live[i]:
            assert got_counts[i] == -4
            continue
        assert got_counts[i] == cnt, r.read_id
        if norm_sig is not None:
            q0 = int(dr.seq_off[i])
            assert norm_sig.dtype == np.float64 and levels.dtype == np.float32
            assert np.array_equal(_bits(x[q0 : q0 + cnt]), _bits(norm_sig)), r.read_id
            assert np.array_equal(y[q0 : q0 + cnt].view(np.uint32), levels.view(np.uint32)), r.read_id


def test_the_two_kernels_return_the_same_bits_with_jittered_barriers():
    """The LDS hand-offs of the radix select (histogram, scan, the bin that is chosen) go through the block barrier of
    rmr_math.h: in the jitter build (`make jitter`: a pseudo-random per-wave sleep around every barrier) the two kernel tests
    above pass as they stand.  A child process, because a process loads one build of the library."""
    import subprocess
    import sys

    lib = os.path.join(os.path.dirname(HERE), "remora_amd", "libremora_hip_jitter.so")
    assert os.path.exists(lib), "make -C remora_amd/csrc jitter (build() does)"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                          "theil_sen_fit_equals or rescale_points_equal"], env=dict(os.environ, REMORA_HIP_LIB=lib), capture_output=True,
                         text=True, timeout=300, cwd=os.path.dirname(HERE))
    assert out.returncode == 0 and "2 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-1500:]


# ---- 3. refine_device_reads against refine_reads -------------------------------------------------------------------------
def _flow_batch(ref, big=True):
    """Reads of 40 .. 3000 bases, one that leaves after round 1 with "Too few positions" (25 bases: 5 inside the edges) and
    one whose band is refused (no signal assigned)."""
    sizes = [150, 40, 25, 400] + ([3000] if big else []) + [90, 64]
    reads = [_synth(ref, 50 + i, nb, idx=i) for i, nb in enumerate(sizes)]
    bad = _synth(ref, 70, 80, idx=9)
    bad.seq_to_sig_map = np.full_like(bad.seq_to_sig_map, bad.seq_to_sig_map[0])
    reads.insert(3, bad)
    return reads


def _assert_same_flow(got, got_errs, want, want_errs, dr=None):
    assert [(type(e), str(e)) for e in got_errs] == [(type(e), str(e)) for e in want_errs]
    for g, w in zip(got, want):
        assert np.array_equal(g.seq_to_sig_map, w.seq_to_sig_map) and g.seq_to_sig_map.dtype == w.seq_to_sig_map.dtype, g.read_id
        assert _same(g.shift, w.shift) and _same(g.scale, w.scale), (g.read_id, g.shift, w.shift, g.scale, w.scale)
    if dr is not None:
        assert np.array_equal(dr.s2s.cpu().numpy(), np.concatenate([g.seq_to_sig_map for g in got]))
        assert _same(dr.shift.cpu().numpy(), [float(g.shift) for g in got]) and _same(dr.scale.cpu().numpy(), [float(g.scale) for g in got])


@pytest.mark.parametrize("algo", ["dwell_penalty", "Viterbi"])
@pytest.mark.parametrize("rough", [False, True], ids=["plain", "rough"])
@pytest.mark.parametrize("iters", [1, 3])
def test_refine_device_reads_equal_refine_reads(torch_cuda, iters, rough, algo):
    """Mappings, shift, scale and per-read errors (type and text) of the resident rounds against refine_reads under the same
    seed, with a read above 1000 points (drawn sub-samples), a read that leaves with "Too few positions" and a band error; the
    device arrays end up holding what the read objects hold."""
    from remora_amd import RemoraError
    from remora_amd.data_chunks import DeviceReads

    ref = _refiner(scale_iters=iters, do_rough_rescale=rough, algo=algo)
    want = _flow_batch(ref)
    np.random.seed(7)
    want_errs = ref.refine_reads(want)
    want_next = np.random.random()  # where the host rounds leave the generator
    assert [e is not None for e in want_errs] == [i == 3 for i in range(len(want))] and isinstance(want_errs[3], RemoraError)
    got = _flow_batch(ref)
    before = [(r.shift, r.scale) for r in got]
    dr = DeviceReads(got)
    np.random.seed(7)
    if rough:
        ref.rough_rescale_device(dr, got)
    got_errs = ref.refine_device_reads(dr, got, errors="collect")
    _assert_same_flow(got, got_errs, want, want_errs, dr)
    moved = [(r.shift, r.scale) != b for r, b in zip(got, before)]
    assert moved[0] and moved[5] and (rough or not moved[2]), "which reads were re-scaled"  # (25 bases: too few positions)
    assert np.random.random() == want_next, "the generator's state"
    # errors="raise": the same work, then the first error in read order, the generator back where the call found it
    again = _flow_batch(ref)
    dr = DeviceReads(again)
    np.random.seed(9)
    state = np.random.get_state()
    if rough:
        ref.rough_rescale_device(dr, again)
    with pytest.raises(RemoraError) as ei:
        ref.refine_device_reads(dr, again)
    assert str(ei.value) == str(want_errs[3])
    now = np.random.get_state()
    assert np.array_equal(now[1], state[1]) and now[2] == state[2]


def test_the_result_does_not_depend_on_the_place_in_the_batch(torch_cuda):
    """Without a read above 1000 points nothing is drawn: every read's result is its own, wherever it stands."""
    from remora_amd.data_chunks import DeviceReads

    ref = _refiner(scale_iters=3, do_rough_rescale=True)
    base = _flow_batch(ref, big=False)
    dr = DeviceReads(base)
    ref.rough_rescale_device(dr, base)
    base_errs = ref.refine_device_reads(dr, base, errors="collect")
    state = np.random.get_state()
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(base))
        reads = _flow_batch(ref, big=False)
        reads = [reads[k] for k in order]
        dr = DeviceReads(reads)
        ref.rough_rescale_device(dr, reads)
        errs = ref.refine_device_reads(dr, reads, errors="collect")
        _assert_same_flow(reads, errs, [base[k] for k in order], [base_errs[k] for k in order], dr)
    assert np.array_equal(np.random.get_state()[1], state[1]), "something was drawn"


def test_scale_iters_zero_keeps_its_behaviour_and_collects_on_request(torch_cuda):
    from remora_amd import RemoraError
    from remora_amd.data_chunks import DeviceReads

    ref = _refiner(scale_iters=0)
    want = _flow_batch(ref)
    want_errs = ref.refine_reads(want)
    got = _flow_batch(ref)
    dr = DeviceReads(got)
    s2s = dr.s2s.clone()
    with pytest.raises(RemoraError):
        ref.refine_device_reads(dr, got)
    assert np.array_equal(dr.s2s.cpu().numpy(), s2s.cpu().numpy())  # raised before anything was written back
    _assert_same_flow(got, ref.refine_device_reads(dr, got, errors="collect"), want, want_errs, dr)
    with pytest.raises(ValueError):
        ref.refine_device_reads(dr, got, errors="ignore")


# ---- 4. the commands ------------------------------------------------------------------------------------------------------
def _cmd_refiner():
    return _refiner(do_rough_rescale=True, scale_iters=2)


def _no_refine_reads(monkeypatch):
    from remora_amd.refine_signal_map import SigMapRefiner

    def refused(self, *a, **k):
        raise AssertionError("refine_reads was called: the read-by-read fallback is still there")

    monkeypatch.setattr(SigMapRefiner, "refine_reads", refused)


def _host_refinement(monkeypatch):
    """The comparand of the two commands that have a switch: their per-read paths with the refinement the parent of this
    change gave an iterative refiner - refine_reads on the read objects (host re-scaling), the batch uploaded afterwards."""
    from remora_amd.data_chunks import DeviceReads
    from remora_amd.refine_signal_map import SigMapRefiner

    host_refine_reads = SigMapRefiner.refine_reads

    def rough(self, dr, reads, *a, **k):
        pass  # (refine_reads does it)

    def refine(self, dr, reads, errors="raise"):
        assert all(hasattr(r, "dacs") for r in reads), "the per-read path works on read objects"
        errs = host_refine_reads(self, reads)
        fresh = DeviceReads(reads, dr.engine)
        dr.__dict__.update(fresh.__dict__)
        if errors == "raise":
            for e in errs:
                if e is not None:
                    raise e
            return None
        return errs

    monkeypatch.setattr(SigMapRefiner, "rough_rescale_device", rough)
    monkeypatch.setattr(SigMapRefiner, "refine_device_reads", refine)


def test_infer_output_is_the_same_file_with_and_without_the_batch_ingest(torch_cuda, tmp_path, monkeypatch):
    """`infer from_pod5_and_bam` with a model whose refiner iterates (scale_iters = 2, rough re-scale first), both anchors: the
    default run takes the batch ingest (counted) and never calls refine_reads; RMR_INFER_BATCH_INGEST=0 with the host
    refinement writes the same bytes."""
    from oracle import oracle as O
    from remora_amd import io as rio
    from remora_amd.inference import infer_from_pod5_and_bam
    from remora_amd.model_util import load_model, model_from_state
    from test_gpu_parity import _mint_pt, _real_reads_golden

    g = _real_reads_golden("can")
    _, md = load_model(_mint_pt(tmp_path, g, O), device=0)
    md = dict(md, sig_map_refiner=_cmd_refiner())
    model = model_from_state(O.state_from_npz(g), md, device=0)
    batches = []
    real = rio.iter_ingest_batches

    def counted(*a, **k):
        for ib in real(*a, **k):
            batches.append(isinstance(ib, rio.IngestBatch))
            yield ib

    pod5, bam = os.path.join(DATA, "can_reads.pod5"), os.path.join(DATA, "can_mappings.bam")
    plain = str(tmp_path / "plain.bam")
    for ref_anchored in (False, True):
        outs, stats = [], []
        for mode in ("1", "0"):
            with monkeypatch.context() as mp:
                mp.setattr(rio, "iter_ingest_batches", counted)
                mp.setenv("RMR_INFER_BATCH_INGEST", mode)
                if mode == "1":
                    _no_refine_reads(mp)
                else:
                    _host_refinement(mp)
                del batches[:]
                out = str(tmp_path / f"o{mode}.bam")
                np.random.seed(7)
                stats.append(infer_from_pod5_and_bam(pod5, bam, model, md, out, reads_per_batch=5, ref_anchored=ref_anchored))
                outs.append(open(out, "rb").read())
                assert (len(batches) >= 2 and all(batches)) if mode == "1" else not batches, "which ingest ran"
        assert stats[0] == stats[1] and stats[0][None] >= 10 and outs[0] == outs[1]
        # and the iterations are in it: not the file of the single-pass refiner
        infer_from_pod5_and_bam(pod5, bam, model, dict(md, sig_map_refiner=_refiner(do_rough_rescale=True, scale_iters=0)), plain,
                                reads_per_batch=5, ref_anchored=ref_anchored)
        assert open(plain, "rb").read() != outs[0]


def test_dataset_prepare_writes_the_same_directory_on_either_path(torch_cuda, tmp_path, monkeypatch):
    """extract_chunk_dataset with --refine-scale-iters 2 on the batch ingest (counted, refine_reads refused) and with
    RMR_PREPARE_BATCH_INGEST=0 and the host refinement: every file of the dataset directory byte for byte."""
    import remora_amd.prepare_train_data as ptd
    from remora_amd.util import Motif
    from test_gpu_parity import _prep_args

    _, which, mod_base, kw = _prep_args("can_refine")
    assert not kw["basecall_anchor"] and kw["bed"] is None

    def run(out_dir):
        np.random.seed(11)
        ptd.extract_chunk_dataset(
            bam_path=os.path.join(DATA, f"{which}_mappings.bam"), pod5_path=os.path.join(DATA, f"{which}_reads.pod5"), out_path=out_dir,
            mod_base=mod_base, mod_base_control=mod_base is None, motifs=[Motif(*m) for m in kw["motifs"]], focus_ref_pos=None,
            chunk_context=kw["chunk_context"], min_samps_per_base=kw["min_samps_per_base"], max_chunks_per_read=kw["max_chunks_per_read"],
            pa_scaling=None, sig_map_refiner=_cmd_refiner(), kmer_context_bases=kw["kmer_context_bases"],
            base_start_justify=kw["base_start_justify"], offset=kw["offset"], num_reads=None, basecall_anchor=False, reads_per_batch=5)

    calls = []
    real = ptd.extract_chunk_arrays_from_ingest

    def counted(*a, **k):
        got = real(*a, **k)
        calls.append(got is not None)
        return got

    with monkeypatch.context() as mp:
        mp.setattr(ptd, "extract_chunk_arrays_from_ingest", counted)
        _no_refine_reads(mp)
        run(str(tmp_path / "batch"))
    assert len(calls) >= 2 and all(calls), "the batch ingest did not run, or handed a batch back"
    with monkeypatch.context() as mp:
        mp.setenv("RMR_PREPARE_BATCH_INGEST", "0")
        _host_refinement(mp)
        run(str(tmp_path / "reads"))
    files = sorted(os.listdir(tmp_path / "batch"))
    assert files == sorted(os.listdir(tmp_path / "reads")) and "metadata.jsn" in files and len(files) >= 5
    for f in files:
        assert open(tmp_path / "batch" / f, "rb").read() == open(tmp_path / "reads" / f, "rb").read(), f
    assert os.path.getsize(tmp_path / "batch" / "signal.npy") > 1000


def test_site_kmer_levels_equal_the_per_read_path(torch_cuda, monkeypatch):
    """io.get_site_kmer_levels with the iterating refiner on the batch ingest (refine_reads refused) against the same call with
    every batch handed over as io.Read objects, which are refined by refine_reads: the same arrays."""
    from remora_amd import io as rio

    pod5, bam = os.path.join(DATA, "can_reads.pod5"), os.path.join(DATA, "can_mappings.bam")
    with monkeypatch.context() as mp:
        _no_refine_reads(mp)
        np.random.seed(3)
        got = rio.get_site_kmer_levels(pod5, bam, _cmd_refiner(), (2, 2), min_cov=3)
    real = rio.iter_ingest_batches
    handed = []

    def read_by_read(*a, **k):
        for ib in real(*a, **k):
            handed.append(1)
            yield ib.per_read() if isinstance(ib, rio.IngestBatch) else ib

    with monkeypatch.context() as mp:
        mp.setattr(rio, "iter_ingest_batches", read_by_read)
        np.random.seed(3)
        want = rio.get_site_kmer_levels(pod5, bam, _cmd_refiner(), (2, 2), min_cov=3)
    assert handed and sorted(got) == sorted(want) and sum(v.size for v in want.values()) >= 50
    for kmer in want:
        assert np.array_equal(_bits(got[kmer]), _bits(want[kmer])), kmer
    plain = rio.get_site_kmer_levels(pod5, bam, _refiner(do_rough_rescale=True, scale_iters=0), (2, 2), min_cov=3)
    assert any(not np.array_equal(plain[k], got[k]) for k in got)


def test_region_metrics_equal_the_per_read_path(torch_cuda, monkeypatch):
    """get_ref_reg_samples_metrics with the iterating refiner: the batch path (refine_reads refused, no io.Read built) against
    reads refined one by one as Read.set_refine_signal_mapping does, same seed, one read per batch on both sides (the
    sub-samples of a batch are drawn round by round, those of a single read round by round as well)."""
    from conftest import golden
    from remora_amd import io as rio

    fx = golden("region_metrics.npz")
    ctg, strand, start, end = fx["regions"][list(fx["region_names"]).index("b_rev")]
    reg = rio.RefRegion(str(ctg), str(strand), int(start), int(end))
    pod5, bam = os.path.join(DATA, "can_reads.pod5"), os.path.join(DATA, "can_mappings.bam")

    def no_reads(*a, **k):
        raise AssertionError("the per-read path was taken")

    with monkeypatch.context() as mp:
        _no_refine_reads(mp)
        mp.setattr(rio, "_reads_of_records", no_reads)
        np.random.seed(5)
        (mets,), (recs,) = rio.get_ref_reg_samples_metrics(reg, [(pod5, bam)], sig_map_refiner=_cmd_refiner(), metric="dwell_mean_sd",
                                                           reads_per_batch=1)
    assert len(recs) >= 3
    by_name = {}
    for read, err in rio.iter_reads_from_pod5_and_bam(pod5, bam):
        if err is None and read.ref_to_signal is not None:
            by_name[read.record.query_name] = read
    np.random.seed(5)
    for row, rec in enumerate(recs):
        read = by_name[rec.query_name]
        read.set_refine_signal_mapping(_cmd_refiner(), ref_mapping=True)
        want = read.compute_per_base_metric("dwell_mean_sd", region=reg)
        for key in mets:
            w = np.ascontiguousarray(want[key][::-1], np.float64)
            assert mets[key][row].shape == w.shape and np.array_equal(np.ascontiguousarray(mets[key][row], np.float64).view(np.uint8),
                                                                      w.view(np.uint8)), (row, key)
