"""The refinement DP of remora_amd/csrc/k_refine.hip on every route its waves can take, each against the CPU oracle (maps
with integer equality, statuses by their text) and each with the launch counts of refine_band / refine_dp / refine_dp_rowwise
that prove the route ran: persistent waves that draw further reads from the work counter (RMR_REFINE_GRID), every penalty
length of the register path and the first one past it, signal lengths at the block, ring and checkpoint edges, the two width
classes at their edges, rows on both sides of 32767 samples, a hand-back in the middle of a wave after a replay out of
checkpoint reach, traceback lookups outside their row in all three kernels, and one call with every route and status in it.

The reads come from tests/refine_cases.py; tests/test_host_refine_cases.py shows on the CPU that each has the property it is
used for here."""
import numpy as np
import pytest

import refine_cases as C

pytestmark = pytest.mark.gpu

ALGOS = ("Viterbi", "dwell_penalty")
_want_cache = {}


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def _want(read, rs, algo, sd):
    key = (id(read), id(rs.table), rs.center, rs.hbw, algo, sd.tobytes())
    if key not in _want_cache:
        _want_cache[key] = (read, C.expect(read, rs.table, rs.center, rs.hbw, algo, sd))   # (the read is kept: ids stay unique)
    return _want_cache[key][1]


def _run(monkeypatch, rs, reads, algo, sd=C.DEFAULT_SD, grid=None, force_w=None, rowwise=False):
    """One rmr_refine_signal_maps call under the given switches -> (maps, statuses, launches of the three refine kernels).
    Every read's map and status is compared with the oracle before the function returns."""
    from remora_amd.engine import get_engine
    from remora_amd.refine_signal_map import SigMapRefiner

    for name, val in (("RMR_REFINE_GRID", grid), ("RMR_REFINE_W", force_w), ("RMR_REFINE_ROWWISE", 1 if rowwise else None)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    ref = SigMapRefiner(_levels_array=rs.table, center_idx=rs.center, scale_iters=0, algo=algo, half_bandwidth=rs.hbw, sd_arr=sd)
    eng = get_engine(0)
    eng.profile_reset()
    eng.profile_enable(True)
    try:
        outs, status, dev = ref._refine_batch([r[0] for r in reads], [C.SHIFT] * len(reads), [C.SCALE] * len(reads),
                                              [r[1] for r in reads], [r[2] for r in reads])
    finally:
        eng.profile_enable(False)
    prof = eng.profile()
    launches = {k: prof.get(k, (0.0, 0))[1] for k in ("refine_band", "refine_dp", "refine_dp_rowwise")}
    assert launches["refine_band"] == 1
    for i, r in enumerate(reads):
        want, err = _want(r, rs, algo, sd)
        if err is None:
            assert status[i] == 0, (i, dev.status_message(status[i]))
            np.testing.assert_array_equal(outs[i], want, err_msg=f"{algo} read {i} ({r[2].size} bases)")
        else:
            assert status[i] != 0 and dev.status_message(status[i]) == err, (i, status[i], err)
            outs[i] = outs[i][:0]   # a refused read has no map: nothing of its slot is compared between runs
    return outs, status, launches


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def batch37():
    return C.mixed_batch()


@pytest.mark.parametrize("force_w", [None, 64], ids=["w16", "w64"])
@pytest.mark.parametrize("algo", ALGOS)
def test_persistent_waves_take_further_reads(monkeypatch, batch37, algo, force_w):
    """37 reads, so a last group of one: with the launch capped at 1, 2 and 3 waves every wave goes round its loop again and
    again (ten rounds of four reads for one 16-lane wave, 37 for one 64-lane wave), re-initialising its tables of learnt
    terms, reusing its traceback slots and checkpoints, after reads that replayed; the results are the oracle's and, byte for
    byte, those of the uncapped launch (ten waves / 37 waves, one round each)."""
    rs = batch37
    free, st_free, n = _run(monkeypatch, rs, rs.reads, algo, force_w=force_w)
    assert (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0)
    assert _same([free[0]], [free[-1]])   # the largest read, first and last in input order
    for grid in (1, 2, 3):
        outs, status, n = _run(monkeypatch, rs, rs.reads, algo, grid=grid, force_w=force_w)
        assert (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0), grid
        assert _same(outs, free) and np.array_equal(status, st_free), grid
    # a value of 0 or below is "unset"
    outs, status, n = _run(monkeypatch, rs, rs.reads, algo, grid=0, force_w=force_w)
    assert _same(outs, free) and (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0)


@pytest.mark.parametrize("force_w", [None, 64], ids=["w16", "w64"])
@pytest.mark.parametrize("sd_len", [1, 2, 3, 4, 5, 6, 7])
def test_every_penalty_length(monkeypatch, batch37, sd_len, force_w):
    """refine_dp_kernel<W, D, 1> for D = 1..6 (replays among the reads, so the checkpoints of 13 + 4 D dwords are written and
    read back), and the first length past kMaxD, which the row-wise kernel takes whole."""
    rs = batch37
    _, _, n = _run(monkeypatch, rs, rs.reads[:14], "dwell_penalty", sd=C.default_sd(sd_len), force_w=force_w)
    assert (n["refine_dp"], n["refine_dp_rowwise"]) == ((1, 0) if sd_len <= C.K_MAX_D else (0, 1))


@pytest.mark.parametrize("force_w", [None, 64], ids=["w16", "w64"])
@pytest.mark.parametrize("algo", ALGOS)
def test_lengths_at_block_and_ring_edges(monkeypatch, algo, force_w):
    rs = C.LENGTHS
    _, status, n = _run(monkeypatch, rs, rs.reads, algo, force_w=force_w)
    assert not status.any() and (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("e", C.WIDTH_EDGES, ids=lambda e: f"edge{e.edge}")
def test_width_classes_at_their_edges(monkeypatch, e, algo):
    """16 rows per sample: the 16-lane kernel; 17: the 64-lane kernel; 64: still that; 65: the row-wise kernel.  Dropping
    the reads one past the edge removes exactly that launch."""
    rs = C.ReadSet(None, e.table, e.k, e.center, e.hbw)
    mixed = [r for pair in zip(e.below, e.above) for r in pair]
    _, status, n_all = _run(monkeypatch, rs, mixed, algo)
    _, _, n_below = _run(monkeypatch, rs, e.below, algo)
    assert not status.any()
    if e.edge == 16:
        assert (n_all["refine_dp"], n_all["refine_dp_rowwise"]) == (2, 0)
    else:
        assert (n_all["refine_dp"], n_all["refine_dp_rowwise"]) == (1, 1)
    assert (n_below["refine_dp"], n_below["refine_dp_rowwise"]) == (1, 0)


@pytest.mark.parametrize("algo", ALGOS)
def test_rows_wider_than_the_int16_traceback(monkeypatch, algo):
    """Widest rows of 32767, 32770 and 33079 samples: the first is the column kernel's (stay counts up to 32766 in int16),
    the other two go row-wise."""
    rs = C.WIDE_ROWS
    _, _, n = _run(monkeypatch, rs, rs.reads[:1], algo)
    assert (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0)
    _, status, n = _run(monkeypatch, rs, rs.reads, algo)
    assert not status.any() and (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 1)


@pytest.mark.parametrize("which", range(len(C.OUT_OF_REACH.reads)))
def test_hand_back_in_the_middle_of_a_wave(monkeypatch, which):
    """One wave of four reads.  With the control read (replays in reach) nothing leaves the column kernel; with the stalled
    read one lane group learns a large-score term more than kCk blocks after the row began, stops, and its read goes
    row-wise, while the three neighbours carry on, replay, and return what they returned in the control run."""
    rs = C.OUT_OF_REACH
    ctl = [C.OUT_OF_REACH_CONTROL.reads[which]] + C.NEIGHBOURS
    full = [rs.reads[which]] + C.NEIGHBOURS
    outs_c, st_c, n = _run(monkeypatch, rs, ctl, "dwell_penalty", grid=1)
    assert not st_c.any() and (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0)
    outs_f, st_f, n = _run(monkeypatch, rs, full, "dwell_penalty", grid=1)
    assert not st_f.any() and (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 1)
    assert _same(outs_f[1:], outs_c[1:])
    # under Viterbi nothing is speculated: the same reads stay in the column kernel
    _, _, n = _run(monkeypatch, rs, full, "Viterbi", grid=1)
    assert (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0)


def test_hand_back_from_the_64_lane_kernel(monkeypatch):
    """At half_bandwidth 31 rows are wide enough for a replay to be nine blocks behind without a stall: two reads of 64 rows
    per sample, one with such a row, one without, through one persistent wave."""
    rs = C.FAR_REPLAY_W64
    _, status, n = _run(monkeypatch, rs, rs.reads[1:], "dwell_penalty", grid=1)
    assert not status.any() and (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 0)
    _, status, n = _run(monkeypatch, rs, rs.reads, "dwell_penalty", grid=1)
    assert not status.any() and (n["refine_dp"], n["refine_dp_rowwise"]) == (1, 1)


@pytest.mark.parametrize("route", ["w16", "w64", "w64-forced", "rowwise"])
def test_traceback_lookups_outside_their_row(monkeypatch, route):
    """Paths that leave their row through large-score cells, mapped through the reference's flat band layout by the
    traceback of the 16-lane kernel, of the 64-lane kernel (by band width, and forced) and of the row-wise kernel."""
    rs = C.OUTSIDE_ROW[64 if route == "w64" else 16]
    outs, status, n = _run(monkeypatch, rs, rs.reads, "dwell_penalty", force_w=64 if route == "w64-forced" else None,
                           rowwise=route == "rowwise")
    assert not status.any()
    assert (n["refine_dp"], n["refine_dp_rowwise"]) == ((0, 1) if route == "rowwise" else (1, 0))


@pytest.mark.parametrize("algo", ALGOS)
def test_one_call_with_every_route_and_status(monkeypatch, algo):
    """Reads of both width classes, a row-wise read and one read of every reachable status in one call under two persistent
    waves: every slot as the oracle says, and the same call in reversed order gives the reversed results."""
    rs, routes = C.mixed_call()
    outs, status, n = _run(monkeypatch, rs, rs.reads, algo, grid=2)
    assert (n["refine_dp"], n["refine_dp_rowwise"]) == (2, 1)
    assert [bool(s) for s in status] == [r in C.STATUSES for r in routes]
    outs_r, status_r, n = _run(monkeypatch, rs, rs.reads[::-1], algo, grid=2)
    assert (n["refine_dp"], n["refine_dp_rowwise"]) == (2, 1)
    assert np.array_equal(status_r[::-1], status)
    ok = [i for i, s in enumerate(status) if s == 0]
    assert _same([outs_r[::-1][i] for i in ok], [outs[i] for i in ok])
