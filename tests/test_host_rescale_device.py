"""The host half of the iterative refiner on a resident batch (SigMapRefiner.rescale_device / refine_device_reads): the two
entry points are declared, exported and bound; the per-base `level_ok` bytes a batch uploads once are the level term of
`rescale`'s mask; and the sub-samples of reads above 1000 points are drawn from numpy's global generator exactly where
`refine_reads` draws them.  The two native calls are replaced by the host function's own values here; the kernels
themselves are held to the host functions in tests/test_gpu_rescale_device.py."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TABLE = os.path.join(HERE, "golden", "data", "levels_4mer.txt")


def _refiner(**kw):
    from remora_amd.refine_signal_map import SigMapRefiner

    return SigMapRefiner(kmer_model_filename=TABLE, do_fix_guage=True, **kw)


def _read(ref, rng, nb, idx=0, noise=0.15):
    """A read whose signal follows the table's levels (so that a re-scale has something to fit), dwells 3..16."""
    from remora_amd.data_chunks import RemoraRead

    seq = rng.integers(0, 4, nb)
    dwell = rng.integers(3, 17, nb)
    m = np.concatenate([[0], np.cumsum(dwell)]).astype(np.int64)
    norm = np.repeat(ref.extract_levels(seq).astype(np.float64), dwell) + noise * rng.standard_normal(m[-1])
    return RemoraRead(dacs=np.round(500 + 80 * norm).astype(np.int16), shift=497.0 + idx, scale=83.5, seq_to_sig_map=m, int_seq=seq,
                      read_id=f"r{nb}_{idx}")


def test_the_new_entry_points_are_declared_exported_and_bound():
    from remora_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "remora_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, n_args in (("rmr_rescale_points", 15), ("rmr_theil_sen_fit", 13)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert decl, f"{name} is not declared in include/remora_hip.h"
        assert len(decl.group(1).split(",")) == n_args
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n_args
        assert getattr(_lib.lib(), name).argtypes == argtypes


@pytest.mark.parametrize("nb", [5, 15, 25, 3000])
def test_level_ok_is_the_level_term_of_rescale(nb, monkeypatch):
    """`rescale` hands np.logical_and.reduce its five mask terms; the third is the level term.  The helper's bytes are that
    term, for reads `rescale` turns away as well (5, 15 and 25 bases: "Too few positions" after the mask is built)."""
    import remora_amd.refine_signal_map as rsm
    from remora_amd import RemoraError

    ref = _refiner(scale_iters=1)
    r = _read(ref, np.random.default_rng(nb), nb)
    levels = ref.extract_levels(r.int_seq)
    seen = []

    class Spy:
        def __getattr__(self, name):
            return getattr(np, name)

        class logical_and:  # noqa: N801 - stands in for the ufunc
            @staticmethod
            def reduce(terms):
                seen.append(terms)
                return np.logical_and.reduce(terms)

    monkeypatch.setattr(rsm, "np", Spy())
    np.random.seed(0)
    try:
        ref.rescale(levels, r.dacs, r.shift, r.scale, r.seq_to_sig_map)
    except RemoraError as e:
        assert nb <= 25 and str(e) == "Too few positions"  # (25 bases: 5 inside the edges, fewer than min_levels)
    monkeypatch.undo()
    (terms,) = seen
    assert len(terms) == 5 and terms[2].dtype == np.bool_ and terms[2].shape == (nb,)
    got = ref.level_ok(levels)
    assert got.dtype == np.uint8 and np.array_equal(got.astype(bool), terms[2])
    if nb >= 25:
        assert 0 < int(got.sum()) < nb


def test_no_pair_of_increasing_x_gives_nan_scaling_and_no_error_on_the_host():
    """What rescale_device restates for the kernel's "no pair" status: the host's median of nothing is NaN, NaN is not 0, so
    theil_sen raises nothing and the read goes on with NaN shift and scale."""
    from remora_amd.refine_signal_map import theil_sen

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sh, sc = theil_sen(np.full(12, 0.25), np.linspace(-1, 1, 12).astype(np.float32), 500.0, 80.0)
    assert np.isnan(sh) and np.isnan(sc)


class _FakeDeviceReads:
    def __init__(self, reads):
        self.n_reads = len(reads)
        self.scalings = []

    def set_scaling(self, shift, scale):
        self.scalings.append((np.array(shift), np.array(scale)))


def _host_points(ref, r):
    """(dac means, levels) of the valid bases of `rescale` for the read as it stands, or None where it raises."""
    import remora_amd.refine_signal_map as rsm
    from remora_amd import RemoraError

    class Got(Exception):
        pass

    def grab(dacs, levels, shift, scale):
        raise Got(dacs, levels)

    real, rsm.rescale_theil_sen = rsm.rescale_theil_sen, grab
    try:
        ref.rescale(ref.extract_levels(r.int_seq), r.dacs, r.shift, r.scale, r.seq_to_sig_map)
    except Got as g:
        return g.args
    except RemoraError:
        return None
    finally:
        rsm.rescale_theil_sen = real


def test_sub_samples_are_drawn_where_refine_reads_draws_them(monkeypatch):
    """A batch of reads below and above 1000 points with a "too few" read between them, three rounds.  The DP is replaced by
    the identity on both sides and the two native calls by the host function's own count, slope and intercept: the calls of
    np.random.choice (arguments and results), the scalings and the reads that leave are those of refine_reads."""
    import remora_amd.refine_signal_map as rsm

    ref = _refiner(scale_iters=3)
    sizes = [400, 6000, 15, 5200, 90, 4800]
    make = lambda: [_read(ref, np.random.default_rng(100 + i), nb, i) for i, nb in enumerate(sizes)]  # noqa: E731
    calls = []
    real_choice = np.random.choice

    def choice(a, size=None, replace=True, p=None):
        out = real_choice(a, size, replace, p)
        calls.append((a, size, replace, out.copy()))
        return out

    monkeypatch.setattr(np.random, "choice", choice)

    # the host side: refine_reads with an identity DP
    def identity_dp(self, dacs_list, shifts, scales, maps, int_seqs, device=None):
        class Dev:
            status_message = staticmethod(lambda st: "ok")

        return [np.asarray(m).copy() for m in maps], np.zeros(len(maps), np.int32), Dev()

    monkeypatch.setattr(rsm.SigMapRefiner, "_refine_batch", identity_dp)
    want = make()
    np.random.seed(7)
    assert ref.refine_reads(want) == [None] * len(sizes)
    want_calls = list(calls)
    del calls[:]
    n_big = sum(_host_points(ref, r) is not None and _host_points(ref, r)[0].size > 1000 for r in make())
    assert n_big == 3 and len(want_calls) == 3 * n_big
    assert [c[0] for c in want_calls[:3]] == [_host_points(ref, r)[0].size for r in make() if r.int_seq.size > 4000]

    # the device side: rescale_device round by round, the natives answered by the host function
    got = make()
    points = {}

    def fake_points(self, dr, live, edge_filter_bases):
        assert edge_filter_bases == 10
        counts = np.full(len(got), -77, np.int32)
        for i in np.flatnonzero(live):
            points[i] = _host_points(ref, got[i])
            counts[i] = 0 if points[i] is None else points[i][0].size
        return counts

    def fake_fit(self, dr, fit, samp, samp_off):
        slope, inter, status = np.full(len(got), np.nan), np.full(len(got), np.nan), np.full(len(got), -5, np.int32)
        flat = np.concatenate(samp) if samp else np.zeros(0, np.int32)
        for i in np.flatnonzero(fit):
            dacs, levels = points[i]
            x = (dacs - got[i].shift) / got[i].scale
            assert (samp_off[i] >= 0) == (x.size > 1000)
            if samp_off[i] >= 0:
                pick = flat[samp_off[i] : samp_off[i] + 1000]
                assert pick.dtype == np.int32
                x, levels = x[pick], levels[pick]
            dx, dy = x[:, None] - x, levels[:, None] - levels
            slope[i] = np.median(dy[dx > 0] / dx[dx > 0])
            inter[i] = np.median(levels - slope[i] * x)
            status[i] = 0
        return slope, inter, status

    monkeypatch.setattr(rsm.SigMapRefiner, "_rescale_points", fake_points)
    monkeypatch.setattr(rsm.SigMapRefiner, "_theil_sen_fit", fake_fit)
    dr = _FakeDeviceReads(got)
    live = np.ones(len(got), bool)
    np.random.seed(7)
    left = []
    for _ in range(3):
        errs = ref.rescale_device(dr, got, live)
        for i, e in enumerate(errs):
            if e is not None:
                assert live[i] and str(e) == "Too few positions"
                live[i] = False
                left.append(i)
    assert left == [2]
    assert len(calls) == len(want_calls)
    for (a, size, replace, out), (wa, wsize, wreplace, wout) in zip(calls, want_calls):
        assert (a, size, replace) == (wa, wsize, wreplace) and np.array_equal(out, wout)
    for g, w in zip(got, want):
        assert np.float64(g.shift).tobytes() == np.float64(w.shift).tobytes(), g.read_id
        assert np.float64(g.scale).tobytes() == np.float64(w.scale).tobytes(), g.read_id
    assert any(g.shift != r.shift for g, r in zip(got, make()))
    sh, sc = dr.scalings[-1]
    assert np.array_equal(sh, [float(r.shift) for r in got]) and np.array_equal(sc, [float(r.scale) for r in got])
