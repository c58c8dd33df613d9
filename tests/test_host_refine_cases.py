"""CPU checks of tests/refine_cases.py, which tests/test_gpu_refine_paths.py relies on: with the oracle alone, every case list
has the property it is there for (signal lengths at the block edges, rows per sample on both sides of 16 and 64, rows on
both sides of 32767 samples, large-score rows out of checkpoint reach and their controls in reach, traceback lookups outside
their row in both width classes, a read per reachable status), and the oracle accepts every read that is meant to succeed.  A
GPU test can then never pass on an empty class."""
import numpy as np
import pytest

import refine_cases as C

ALGOS = ("Viterbi", "dwell_penalty")


def _ok(rs, read, algo="dwell_penalty", hbw=None):
    want, err = C.expect(read, rs.table, rs.center, rs.hbw if hbw is None else hbw, algo, C.DEFAULT_SD)
    return err is None and want[0] == read[1][0] and want[-1] == read[1][-1] and bool(np.all(np.diff(want) >= 0))


def test_random_read_keeps_the_suites_stream():
    """random_read is the generator test_gpu_refine.py has always used (moved here): `stalls` draws nothing, so reads made
    without it are the reads of before, and a read with it has its twin's bases and one longer dwell."""
    a = C.random_read(np.random.default_rng(3), C.CALM, 3, 1, 40, zero_frac=0.15, stall=True, trim=True)
    b = C.random_read(np.random.default_rng(3), C.CALM, 3, 1, 40, zero_frac=0.15, stall=True, trim=True, stalls=())
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = C.random_read(np.random.default_rng(3), C.CALM, 3, 1, 40, stalls=((20, 500),))
    d = C.random_read(np.random.default_rng(3), C.CALM, 3, 1, 40)
    assert np.array_equal(c[2], d[2]) and 500 - 13 <= c[1][-1] - d[1][-1] <= 500 - 1   # one dwell of 1..13 became 500
    assert c[0].size == c[1][-1]


def test_lengths():
    rs = C.LENGTHS
    assert tuple(sorted({r[2].size for r in rs.reads})) == C.LENGTH_BASES
    nsig = [int(r[1][-1] - r[1][0]) for r in rs.reads]
    assert nsig == [n for _, _, n in C.LENGTH_SEEDS]
    assert {n % 64 for n in nsig} >= {63, 0, 1}
    for mod in (63, 0, 1):  # each residue at short, medium and long reads
        assert sum(n % 64 == mod for n in nsig) >= 3, mod
    assert any(abs(n - 512) <= 1 for n in nsig) and {512, 513} <= set(nsig)
    for r in rs.reads:
        b = C.band(r, rs.hbw)
        assert C.band_is_regular(b) and C.width_class(b) == 16
        for algo in ALGOS:
            assert _ok(rs, r, algo), r[2].size   # the reference's validation refuses none of these lengths


@pytest.mark.parametrize("e", C.WIDTH_EDGES, ids=lambda e: f"edge{e.edge}")
def test_width_edges(e):
    rs = C.ReadSet(e.below + e.above, e.table, e.k, e.center, e.hbw)
    assert len(e.below) >= 2 and len(e.above) >= 2
    assert [C.maxwin(C.band(r, e.hbw)) for r in e.below] == [e.edge] * len(e.below)
    assert [C.maxwin(C.band(r, e.hbw)) for r in e.above] == [e.edge + 1] * len(e.above)
    nxt = {16: 64, 64: 0}[e.edge]
    assert {C.width_class(C.band(r, e.hbw)) for r in e.below} == {e.edge}
    assert {C.width_class(C.band(r, e.hbw)) for r in e.above} == {nxt}
    for r in rs.reads:
        assert C.band_is_regular(C.band(r, e.hbw)) and C.widest_row(C.band(r, e.hbw)) <= C.MAX_ROW
        assert all(_ok(rs, r, algo) for algo in ALGOS)
    for r in e.below + (e.above if e.edge == 16 else []):   # what the column kernel takes, it keeps: no hand-back but the width's
        assert C.replay_blocks(r, e.table, e.center, e.hbw, C.DEFAULT_SD) < C.K_CK


def test_far_replay_in_the_64_lane_kernel():
    rs = C.FAR_REPLAY_W64
    far, near = rs.reads
    assert [C.maxwin(C.band(r, rs.hbw)) for r in rs.reads] == [64, 64] and _ok(rs, far) and _ok(rs, near)
    assert C.replay_blocks(far, rs.table, rs.center, rs.hbw, C.DEFAULT_SD) == C.K_CK
    assert 0 <= C.replay_blocks(near, rs.table, rs.center, rs.hbw, C.DEFAULT_SD) < C.K_CK


def test_wide_rows():
    rs = C.WIDE_ROWS
    widths = [C.widest_row(C.band(r, rs.hbw)) for r in rs.reads]
    assert widths == [w for _, w in C.WIDE_STALLS]
    assert widths[0] == C.MAX_ROW and C.MAX_ROW + 1 <= widths[1] <= C.MAX_ROW + 4 and widths[2] > C.MAX_ROW + 256
    assert [C.width_class(C.band(r, rs.hbw)) for r in rs.reads] == [16, 0, 0]
    for r in rs.reads:
        b = C.band(r, rs.hbw)
        assert r[2].size == 60 and C.maxwin(b) <= 16 and C.band_is_regular(b)   # but for the row width, the 16-lane kernel's
        assert int((b[1] - b[0]).sum()) < 400_000                              # the longest input of the GPU tests
        assert _ok(rs, r, "Viterbi")
    assert _ok(rs, rs.reads[0], "dwell_penalty")


def test_out_of_reach_and_its_control():
    rs, ctl = C.OUT_OF_REACH, C.OUT_OF_REACH_CONTROL
    assert len(rs.reads) == len(ctl.reads) >= 3
    for r, c in zip(rs.reads, ctl.reads):
        assert np.array_equal(r[2], c[2])   # the same bases
        args = (rs.table, rs.center, rs.hbw, "dwell_penalty", C.DEFAULT_SD)
        assert C.far_replay_rows(r, *args), "no large-score row out of checkpoint reach"
        assert C.has_large_score_cells(c, *args) and not C.far_replay_rows(c, *args)
        # the control's replays are in reach whatever the scores: no row i starts 8 blocks before row i - 1 ends
        b = C.band(c, ctl.hbw)
        assert int((b[1, :-1] // 64 - b[0, 1:] // 64).max()) < C.K_CK
        for x in (r, c):
            bx = C.band(x, rs.hbw)
            assert C.width_class(bx) == 16 and C.band_is_regular(bx) and _ok(rs, x)
        assert not C.has_large_score_cells(r, rs.table, rs.center, rs.hbw, "Viterbi", C.DEFAULT_SD)


def test_outside_row():
    assert C.OUTSIDE_ROW[16].hbw != C.OUTSIDE_ROW[64].hbw
    for cls, rs in C.OUTSIDE_ROW.items():
        assert len(rs.reads) >= 2
        for r in rs.reads:
            b = C.band(r, rs.hbw)
            assert C.width_class(b) == cls and (C.maxwin(b) <= 16 if cls == 16 else 17 <= C.maxwin(b) <= 64)
            assert C.outside_row_lookups(r, rs.table, rs.center, rs.hbw, "dwell_penalty", C.DEFAULT_SD) > 0
            assert C.outside_row_lookups(r, rs.table, rs.center, rs.hbw, "Viterbi", C.DEFAULT_SD) == 0   # never under Viterbi
            assert C.band_is_regular(b) and _ok(rs, r)


def test_statuses():
    texts = {t for _, t in C.STATUSES.values()}
    assert texts == {"Read without bases", "Band contains 0-length region", "Invalid sig_band length"}
    for name, (read, text) in C.STATUSES.items():
        assert read[1].size == read[2].size + 1 and read[0].size >= read[1][-1]
        for hbw in C.STATUS_HBWS:
            for algo in ALGOS:
                assert C.expect(read, C.CALM, 1, hbw, algo, C.DEFAULT_SD) == (None, text), (name, hbw)
    # the two reads the oracle's band code cannot take are the ones expect() answers itself
    assert C.STATUSES["no-bases"][0][2].size == 0
    m = C.STATUSES["no-signal"][0][1]
    assert m[0] == m[-1] and m.size > 1


def test_no_oracle_accepted_band_is_irregular():
    """The column kernel's guards against rows that do not start at strictly increasing samples, gaps and nested rows have no
    case: adjust_seq_band rules the shapes out (refine_cases.py gives the argument).  480 random reads, with and without
    zero-dwell bases, at five half widths: every band the oracle accepts is regular, and only reachable statuses occur."""
    from oracle import oracle as O

    reachable = {t for _, t in C.STATUSES.values()}
    n_ok = n_err = 0
    for seed in range(480):
        rng = np.random.default_rng(10_000 + seed)
        r = C.random_read(rng, C.CALM, 3, 1, int(rng.integers(12, 120)), zero_frac=(0.0, 0.3, 0.6)[seed % 3], trim=seed % 2 == 0,
                          stall=seed % 16 == 5)
        hbw = (1, 2, 5, 7, 31)[seed % 5]
        b = C.band(r, hbw)
        err = O.validate_seq_band(b, int(r[1][-1] - r[1][0]), r[2].size)
        if err is None:
            n_ok += 1
            assert C.band_is_regular(b), (seed, hbw)
        else:
            n_err += 1
            assert err in reachable, (seed, hbw, err)
    assert n_ok > 300 and n_err > 10


def test_mixed_batch():
    rs = C.mixed_batch()
    assert len(rs.reads) == 37 and len(rs.reads) % 4 == 1   # a ragged last group of four
    size = [int((C.band(r, rs.hbw)[1] - C.band(r, rs.hbw)[0]).sum()) for r in rs.reads]
    assert size[0] == size[-1] == max(size) and all(np.array_equal(x, y) for x, y in zip(rs.reads[0], rs.reads[-1]))
    assert sum(any(r is c for c in C.OUT_OF_REACH_CONTROL.reads) for r in rs.reads) == 2
    assert len({r[2].size for r in rs.reads}) > 25   # mixed lengths
    n_ok = 0
    for r in rs.reads:
        b = C.band(r, rs.hbw)
        err = C.expect(r, rs.table, rs.center, rs.hbw, "dwell_penalty", C.DEFAULT_SD)[1]
        n_ok += err is None
        if err is None:
            assert C.width_class(b) == 16 and C.band_is_regular(b)
            assert not C.far_replay_rows(r, rs.table, rs.center, rs.hbw, "dwell_penalty", C.DEFAULT_SD)
            # and no replay can be out of reach, whatever the penalties: no row i starts 8 blocks before row i - 1 ends
            assert int((b[1, :-1] // 64 - b[0, 1:] // 64).max(initial=0)) < C.K_CK
    assert n_ok >= 33


def test_neighbours_outlast_the_hand_back():
    args = (C.LOUD, 1, C.OUT_OF_REACH.hbw, "dwell_penalty", C.DEFAULT_SD)
    handed_back_by = max(int(C.band(r, C.OUT_OF_REACH.hbw)[1, i - 1]) for r in C.OUT_OF_REACH.reads for i in C.far_replay_rows(r, *args))
    for r in C.NEIGHBOURS:
        b = C.band(r, C.OUT_OF_REACH.hbw)
        assert r[1][-1] - r[1][0] > handed_back_by + 128 and C.width_class(b) == 16 and C.band_is_regular(b)
        assert C.expect(r, *args)[1] is None and not C.far_replay_rows(r, *args)
        assert int((b[1, :-1] // 64 - b[0, 1:] // 64).max()) < C.K_CK
    assert all(C.has_large_score_cells(r, *args) for r in C.NEIGHBOURS)   # they replay too, within reach


def test_mixed_call():
    rs, routes = C.mixed_call()
    assert routes != sorted(routes) and set(routes) == {"w16", "w64", "rowwise"} | set(C.STATUSES)
    assert routes.count("w16") >= 2 and routes.count("w64") >= 2 and routes.count("rowwise") == 1
    for r, route in zip(rs.reads, routes):
        for algo in ALGOS:
            want, err = C.expect(r, rs.table, rs.center, rs.hbw, algo, C.DEFAULT_SD)
            if route in C.STATUSES:
                assert err == C.STATUSES[route][1]
            else:
                assert err is None and C.width_class(C.band(r, rs.hbw)) == {"w16": 16, "w64": 64, "rowwise": 0}[route]
