"""CPU checks of the case table of tests/test_gpu_stream_shapes.py (tests/stream_cases.py): every case takes, by the restated
launch plans, the path of the streamed-weight kernels it is there for; and the fp32 gate has teeth on the long-chunk cases - one
wrong 16-channel tile at one position of merge_conv1's output moves the logits by three gates or more."""
import numpy as np
import pytest

import stream_cases as S

KCB = (4, 4)
GATE_FP32 = 1e-4  # GATE["fp32"] of tests/test_gpu_lstm_heads.py (a GPU module; restated, and compared below)


def plans(size, L):
    return {name: (S.conv_stream_plan(*spec), spec) for name, spec in S.conv_layers(size, L).items()}


def test_gate_is_the_projects():
    import test_gpu_lstm_heads as H
    import test_gpu_split_shapes as P

    assert H.GATE["fp32"] == GATE_FP32
    assert S.SUB_BATCHES == P.SUB_BATCHES[:5]
    assert (S.N, S.N_BIG) == (H.N, H.N_BIG)


@pytest.mark.parametrize("case", S.FP32_CASES, ids=lambda c: f"{c.group}-{c.size}-{c.L}-{c.batches[-1]}")
def test_every_fp32_launch_fits_and_is_a_streamed_one(case):
    assert case.size > 64 and case.size % 16 == 0
    for name, (p, spec) in plans(case.size, case.L).items():
        assert p.lds <= S.LDS_LIMIT, (case, name, p)
        assert 1 <= p.nw <= 8 and (p.nwin == 1 or p.cb == 1), (case, name, p)
    lp = S.lstm_stream_plan(case.size)
    assert lp.lds <= S.LDS_LIMIT and lp.threads <= (512 if lp.nt == 4 else 1024), (case, lp)


def test_widths_cover_every_wave_count_and_both_lstm_kernels():
    cases = [c for c in S.FP32_CASES if c.group == "widths"]
    assert [c.size for c in cases] == list(range(80, 257, 16)) and set(S.NEW_WIDTHS) < set(S.SIZES)
    nw = {c.size: S.waves(c.size) for c in cases}
    assert nw == {80: 5, 96: 6, 112: 7, 128: 8, 144: 8, 160: 5, 176: 8, 192: 6, 208: 8, 224: 7, 240: 5, 256: 8}
    # eight waves over 9, 11 and 13 output tiles: an uneven share; 144 and 208 are the two that had never run
    assert [c.size for c in cases if S.conv_stream_plan(*S.conv_layers(c.size, 100)["merge_conv1"]).uneven] == [144, 176, 208]
    for c in cases:
        lp = S.lstm_stream_plan(c.size)
        assert lp.nt == (4 if c.size <= 128 else 2) and c.batches == (37, 16 * lp.nt + 1)  # a ragged group; one group and a chunk
        p, spec = plans(c.size, 100)["merge_conv1"]
        assert p.nwin == 1 and S.conv_ntv(p, spec[5], c.batches[0]) >= {2}


def test_step_count_cases_reach_the_small_tiles():
    cases = [c for c in S.FP32_CASES if c.group == "steps"]
    assert len(cases) == 15 and {S.layer_rows(c.L)[3] for c in cases} == {1, 2, 3}
    sig3_ntv, merge_cb = {}, set()
    for c in cases:
        pl = plans(c.size, c.L)
        p, spec = pl["merge_conv1"]
        for n in c.batches:  # merge_conv1: every iteration, full or ragged, is ONE column tile - cb T <= 16 columns of cb 4 .. 8 chunks
            its, cols = S.conv_iterations(p, spec[5], n)
            assert max(cols) <= 16 and S.conv_ntv(p, spec[5], n) == {1} and 4 <= p.cb <= 8, (c, p)
            assert its > 1
        merge_cb.add(p.cb)
        p3, spec3 = pl["sig_conv3"]
        assert p3.nwin == 1
        sig3_ntv[c.L] = S.conv_ntv(p3, spec3[5], c.batches[1]) | S.conv_ntv(p3, spec3[5], c.batches[0])
    assert merge_cb == {4, 5, 6, 7, 8}
    assert sig3_ntv == {29: {1, 2}, 32: {2, 3}, 35: {3, 4}}  # full iterations: 2, 3 and 4 tiles (30, 48 and 56 columns)


def test_window_switch_cases_sit_on_both_sides_of_it():
    for size, L, windows in S.WINDOW_SWITCH:
        p, spec = plans(size, L)["merge_conv1"]
        staged = spec[4] * p.rs * 16 + 64
        assert (staged > S.WINDOW_ABOVE) == windows == (p.nwin > 1), (size, L, p)
        if windows:
            assert 0 < p.last_cols < p.pout_w and p.cb == 1  # the last window is partial
            assert p.pin_w == p.pout_w + 4
        else:  # one row more would not fit
            assert (spec[4] + 1) * p.rs * 16 + 64 > S.WINDOW_ABOVE and p.lds > 150_000
    got = {(size, L): (p.nwin, p.pout_w, p.last_cols, p.lds) for size, L, _ in S.WINDOW_SWITCH for p in [plans(size, L)["merge_conv1"][0]]}
    assert got == {(256, 230): (1, 68, 68, 152640), (256, 233): (5, 16, 5, 43072), (224, 260): (1, 78, 78, 152640),
                   (224, 263): (5, 16, 15, 37952), (128, 437): (1, 137, 137, 153664), (128, 440): (3, 48, 42, 57408)}
    assert max(v[3] for v in got.values()) == 153664  # the largest image the kernel ever takes
    # 260 chunks x 5 windows: more iterations than the 4 x 256 blocks of an MI355X - 276 blocks restage after their first window
    p, spec = plans(256, 233)["merge_conv1"]
    assert S.conv_iterations(p, spec[5], S.MANY_WINDOWS)[0] == 1300 > 4 * 256


def test_window_remainder_cases():
    full, one = plans(256, 266)["merge_conv1"][0], plans(256, 269)["merge_conv1"][0]
    assert (full.nwin, full.pout_w, full.last_cols) == (5, 16, 16)  # pout 80
    assert (one.nwin, one.pout_w, one.last_cols) == (6, 16, 1)      # pout 81: the sixth window stages rows == KW
    assert S.layer_rows(266)[3] == 80 and S.layer_rows(269)[3] == 81


def test_second_trip_cases():
    for c in (c for c in S.FP32_CASES if c.group == "trips"):
        lp = S.lstm_stream_plan(c.size)
        groups = (c.batches[0] + 16 * lp.nt - 1) // (16 * lp.nt)
        assert groups == 1024 + (1 if lp.nt == 4 else 2) and groups > 4 * 256, (c, lp, groups)  # the grid of an MI355X: 1024 blocks
    assert {S.lstm_stream_plan(c.size).nt for c in S.FP32_CASES if c.group == "trips"} == {2, 4}


@pytest.mark.parametrize("cus", [256, 304])
def test_16bit_cases(cus):
    for c in S.CASES16:
        assert c.size % 32 == 0
        n = c.n if c.n is not None else 8 * cus + 37
        cbs = {}
        for name, (ic, oc, kw, _, pin, pout) in S.conv_layers(c.size, c.L).items():
            p = S.conv16_plan(ic, oc, kw, pin, pout, n, cus)
            assert p.lds <= S.LDS_LIMIT, (c, name, p)
            cbs[name] = p.cb
            assert S.conv16_plan(ic, oc, kw, pin, pout, 64, cus).cb == 1  # the groupings of the bit-equality check: cb 1
        lp = S.lstm_stream16_plan(c.size)
        assert lp.lds <= S.LDS_LIMIT and c.size * 16 * lp.nt * 4 <= lp.lds // 2
        if c.group == "cb8":
            assert cbs["sig_conv3"] == 8 and cbs["seq_conv2"] == 8
            assert S.conv16_plan(*[S.conv_layers(96, 100)["sig_conv3"][i] for i in (0, 1, 2, 4, 5)], 300, cus).cb <= 2
        else:
            assert max(cbs.values()) >= 2 and cbs["sig_conv3"] < 8  # the batch is in blocks of several chunks, never of 8
    size, fits, refused = S.LDS_EDGE16
    for L, ok, lds in ((fits, True, 163280), (refused, False, 164320)):
        ic, oc, kw, _, pin, pout = S.conv_layers(size, L)["merge_conv1"]
        p = S.conv16_plan(ic, oc, kw, pin, pout, 3, cus)
        assert p.lds == lds and (p.lds <= S.LDS_LIMIT) == ok and p.cb == 1
        assert pin == (150 if ok else 151)


# ---- the restatement is the launch code's ------------------------------------------------------------------------------------------
def test_stream_plans_keep_their_invariants_and_the_restatement_follows_them(tmp_path):
    """rmr_plan.h makes the launch plans of the streamed-weight kernels and of the split convolution; their launchers only fill
    the argument structs from them.  tests/c/stream_plans.cpp (plain g++, no HIP) sweeps ConvLSTM_w_ref at every size 80 .. 256,
    chunk length 29 .. 470, batch 1 .. 8 CUs + 37 and 256 / 304 / 80 CUs: every plan that is ok stays within its kernel's LDS limit
    and its chunk budget, windows tile the chunk, the wave count divides the output tiles or is 8, the LSTM block is 4 H threads
    within its launch bound and the fc partial sums fit (the count's floor: what the program makes, so that the sweep cannot
    shrink unseen).  Then one line per plan, and the plans restated in Python - stream_cases.conv_stream_plan, conv16_plan, waves,
    lstm_stream_plan, lstm_stream16_plan and test_gpu_split_shapes.conv_split_plan, which the GPU tests and the case checks above
    rely on - give the same numbers on every line, the shapes of the case tables among them.  (n and the CU count reach the fp32
    convolutions, the LSTMs and the split convolution through the grid alone, which the restatement does not have: one line per
    shape; the 16-bit convolutions' lines carry both.)"""
    import os
    import shutil
    import subprocess

    import test_gpu_split_shapes as P

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text("#pragma once\n#define __host__\n#define __device__\n")
    exe = str(tmp_path / "plans")
    cc = subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-I", str(tmp_path), "-I", os.path.join(root, "remora_amd", "csrc"),
                         os.path.join(root, "tests", "c", "stream_plans.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[:4000] + run.stderr
    out = run.stdout.splitlines()
    assert out[0].endswith(" 0 violations") and int(out[0].split()[0]) > 6_000_000, out[0]

    specs, seen32, seen16, count = {}, set(), set(), dict.fromkeys(("conv32", "conv16", "lstm32", "lstm16", "split"), 0)
    for line in out[1:]:
        kind, *f = line.split()
        count[kind] += 1
        if kind in ("conv32", "conv16"):
            size, L, layer = int(f[0]), int(f[1]), f[4 if kind == "conv16" else 2]
            if (size, L) not in specs:
                specs = {(size, L): S.conv_layers(size, L)}  # (the lines of a shape follow each other)
            ic, oc, kw, stride, pin, pout = specs[size, L][layer]
        if kind == "conv32":
            ok, nw, cb, nwin, pin_w, pout_w, rs, lds = map(int, f[3:])
            p = S.conv_stream_plan(ic, oc, kw, stride, pin, pout)
            assert (p.nw, p.cb, p.nwin, p.pin_w, p.pout_w, p.rs, p.lds) == (nw, cb, nwin, pin_w, pout_w, rs, lds) and nw == S.waves(oc), line
            assert ok == (lds <= S.LDS_LIMIT) == 1, line
            seen32.add((size, L))
        elif kind == "conv16":
            n, cus, (ok, nw, cb, lds) = int(f[2]), int(f[3]), map(int, f[5:])
            assert S.conv16_plan(ic, oc, kw, pin, pout, n, cus) == (nw, cb, lds) and ok == (lds <= S.LDS_LIMIT), line
            seen16.add((size, L, n, cus))
        elif kind in ("lstm32", "lstm16"):
            size, ok, nt, threads, lds = map(int, f)
            assert (S.lstm_stream_plan if kind == "lstm32" else S.lstm_stream16_plan)(size) == (nt, threads, lds) and ok == 1, line
        else:
            ic, pin, parts, ok, cb, lds = map(int, f)
            assert P.conv_split_plan(ic, pin, parts) == (cb, lds) and ok == (lds <= 160 * 1024), line
    sweep = len(S.SIZES) * len(range(29, 471))
    assert count == {"conv32": 3 * sweep, "conv16": 3 * sweep * 27, "lstm32": 12, "lstm16": 6, "split": 3 * 591 * 3}, count
    # every shape of the case tables was compared: the fp32 cases by (size, L), the 16-bit ones with their batch and both CU counts
    for c in S.FP32_CASES:
        assert (c.size, c.L) in seen32, c
    for size, L, _ in S.WINDOW_SWITCH:
        assert (size, L) in seen32, (size, L)
    for cus in (256, 304):
        for c in S.CASES16:
            for n in (c.n if c.n is not None else 8 * cus + 37, 64, 300):  # the case's batch; what test_16bit_cases asks besides
                assert (c.size, c.L, n, cus) in seen16, (c, n, cus)
        for L in S.LDS_EDGE16[1:]:
            assert (S.LDS_EDGE16[0], L, 3, cus) in seen16, (L, cus)


# ---- the fp32 gate has teeth on the long-chunk cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.LONG_CASES, ids=lambda c: f"{c.size}-{c.L}")
def test_one_wrong_tile_of_merge_conv1_moves_the_logits_by_three_gates(case):
    """The float64 network of the case, on the case's own five chunks, with ONE 16-channel tile of merge_conv1's output (before the
    swish; a forward hook on merge_bn) at ONE position of ONE chunk replaced by the neighbouring column - what a window that
    stages one row off, or a wave that stores a tile to the wrong column, would do.  At positions 0, T / 2 and T - 1 the chunk's
    logits move by 3 x 1e-4 or more, and no other chunk's move at all: the 1e-4 gate of tests/test_gpu_stream_shapes.py sees such
    an error through an LSTM of up to 138 steps.  A condition on the inputs (synth_state(seed=stream_cases.weights_seed(size)) - another seed than
    `size`, see there - and synth_chunks(shard=L)), not a measurement of any kernel.  Smallest move with these inputs: 7.0e-4
    (size 128, L 440, position T / 2); each case prints its three."""
    import torch

    from oracle import oracle as O
    from oracle import torch_ref
    from remora_amd import synth

    T = S.layer_rows(case.L)[3]
    d = synth.synth_chunks(5, case.L, min(20, case.L // 4), KCB, 3, True, shard=case.L)
    enc = O.compute_encoded_kmer_batch(*KCB, d["sequence"], d["sequence_to_signal_mapping"], d["sequence_lengths"])
    net = torch_ref.from_state(synth.synth_state("conv_lstm", case.size, 9, 3, seed=S.weights_seed(case.size), amplify=True)).double()
    sig, enc = torch.tensor(d["signal"]).double(), torch.tensor(enc).double()
    ch = slice(16 * S.TEETH_TILE, 16 * S.TEETH_TILE + 16)
    with torch.no_grad():
        ref = net(sig, enc).numpy()
        moves = {}
        for pos in (0, T // 2, T - 1):
            def swap(_mod, _inp, out, pos=pos):
                assert out.shape == (5, case.size, T)
                out = out.clone()
                out[S.TEETH_CHUNK, ch, pos] = out[S.TEETH_CHUNK, ch, pos + 1 if pos + 1 < T else pos - 1]
                return out

            handle = net.merge_bn.register_forward_hook(swap)
            try:
                moved = np.abs(net(sig, enc).numpy() - ref)
            finally:
                handle.remove()
            moves[pos] = float(moved[S.TEETH_CHUNK].max())
            others = np.delete(moved, S.TEETH_CHUNK, axis=0)
            assert others.max() == 0.0, (case, pos)
    print(f"size {case.size} L {case.L} T {T}: logit moves {moves}")
    assert min(moves.values()) >= 3 * GATE_FP32, (case, moves)
