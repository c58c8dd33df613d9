"""CPU checks of the case table of tests/test_gpu_train_shapes.py (tests/train_cases.py): every case takes, by the restated launch
arithmetic of api_train.hip / k_train.hip, the path it is there for; every named path is taken by some case and not taken by
another; the restated layer geometry is the reference network's; and every case is well enough conditioned for the gradient gate
of tests/test_gpu_train_grads.py - torch fp32 stays within 5e-6 of torch float64 on the case's own inputs and initial state, so
max(2e-5, 4 x torch fp32's) is the 2e-5 floor in every case."""
import numpy as np
import pytest
import torch

import train_cases as C

CONDITION = 5e-6
IDS = [C.case_id(c.shape) for c in C.CASES]


def group(name):
    return [c for c in C.CASES if c.group == name]


def test_the_table_is_the_one_the_issue_asks_for():
    assert len(set(IDS)) == len(IDS)
    assert [c.shape for c in group("sizes")] == [(s, 41, 18, 9, 2, "seeded") for s in range(16, 257, 16)]
    assert [c.shape for c in group("kmers")] == [(16, 35, 9, k, 2, "seeded") for k in range(1, 22)]
    assert [c.shape for c in group("classes")] == [(16, 33, 21, 9, o, "seeded") for o in range(2, 17)] + [(16, 33, 21, 9, 16, "absent2")]
    assert [c.shape for c in group("lengths")] == [(32, L, 7, 9, 2, "seeded") for L in range(29, 44)]
    assert [c.shape for c in group("batches")] == [(16, 35, n, 9, 2, "seeded") for n in (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129)]
    assert [c.shape for c in group("reductions")] == [(16, 100, 700, 1, 2, "seeded"), (16, 32, 18800, 1, 2, "centre")]
    assert [c.shape for c in group("inside")] == [(64, 100, 37, 9, 2, "seeded", 300)]
    assert {c.shape[5] for c in group("masks")} == {"keep1", "drop1"}
    for c in C.CASES:  # what rmr_trainer_create and rmr_trainer_forward_backward accept
        size, L, n, K, num_out = c.shape[:5]
        assert 16 <= size <= 256 and size % 16 == 0 and 1 <= K <= 21 and 2 <= num_out <= 16 and 29 <= L <= 200 and n >= 2


def test_absent_classes_are_absent_and_masks_keep_what_they_say():
    _, _, labels, mask = C.case_inputs((16, 33, 21, 9, 16, "absent2"))
    assert mask is None and labels.max() <= 13 and len(set(labels.tolist())) >= 8
    for o in C.CLASS_COUNTS:
        labels = C.case_inputs((16, 33, 21, 9, o, "seeded"))[2]
        assert 0 <= labels.min() and labels.max() <= o - 1
    assert C.case_inputs((16, 35, 17, 9, 2, "keep1"))[3].sum() == 1
    assert C.case_inputs((16, 35, 17, 9, 2, "drop1"))[3].sum() == 16
    assert C.case_inputs(C.RESIDENCY)[3].sum() == 25


# ---- every case named after a path takes it -----------------------------------------------------------------------------------------
def test_reduction_cases_take_their_trips():
    f = C.shape_facts(C.SECOND_TRIP)
    assert f.colsum_second_trip and not f.colsum_capped and f.wgrad_capped and f.wgrad_second_trip
    rows = C.colsum_rows(*C.SECOND_TRIP[:5])
    assert rows["sig_conv1"] == 67200 and C.colsum_plan(67200) == (132, 510)  # lanes 0 .. 3 of the second pass add three partials
    assert rows["lstm1.bias"] == 16800 and C.colsum_plan(16800)[0] == 33
    # n T = 16 800 rows want 66 slices; which products the workspace shortens depends on who sized it.  At size 16 that is
    # seq_conv2 (K x NC = 208 x 16, the largest of the network): cap 64 < want 77.  lstm1's and merge_conv1's K x NC are smaller,
    # so their 66 slices fit (cap 208 and 83) - and take train_wgrad_reduce_kernel's second trip instead; the 18 800-chunk case
    # below is the one that shortens merge_conv1's
    assert f.capped_products == ("seq_conv2",)
    part = C.part_w_floats(16, 100, 1, 2, 700)
    assert part == 208 * 16 * 64
    plans = {p.name: C.wgrad_plan(p, part) for p in C.wgrad_products(*C.SECOND_TRIP[:5])}
    assert (plans["seq_conv2"].want, plans["seq_conv2"].cap, plans["seq_conv2"].rows_per, plans["seq_conv2"].slices) == (77, 64, 308, 64)
    assert (plans["lstm1.weight_ih"].want, plans["lstm1.weight_ih"].cap, plans["lstm1.weight_ih"].slices) == (66, 208, 66)
    assert (plans["merge_conv1"].want, plans["merge_conv1"].cap, plans["merge_conv1"].slices) == (66, 83, 66)
    assert plans["sig_conv1"].slices == 263 and plans["sig_conv2"].slices > 192  # a fourth and fifth trip of the reduction

    f = C.shape_facts(C.CAPPED)
    assert f.colsum_capped and f.colsum_second_trip and f.wgrad_capped
    rows = C.colsum_rows(*C.CAPPED[:5])
    assert rows["sig_conv1"] == rows["seq_conv1"] == 526400 > 1024 * 512 and C.colsum_plan(526400) == (1024, 515)
    assert max(r for name, r in rows.items() if name != "sig_conv1" and name != "seq_conv1") <= 1024 * 512
    assert C.colsum_plan(rows["sig_conv2"]) == (882, 512)  # the most blocks short of the cap
    # every convolution but sig_conv1 is shortened to the workspace: the product that sized it (seq_conv2, cap 64), merge_conv1
    # (n T = 37 600 rows want 147 slices, cap 83); the LSTM products' 16 x 64 partials fit (cap 208) and take a third trip
    assert f.capped_products == ("merge_conv1", "sig_conv3", "sig_conv2", "seq_conv2", "seq_conv1") and f.T == 2
    part = C.part_w_floats(*C.CAPPED[:2], *C.CAPPED[3:5], C.CAPPED[2])
    plans = {p.name: C.wgrad_plan(p, part) for p in C.wgrad_products(*C.CAPPED[:5])}
    assert (plans["merge_conv1"].want, plans["merge_conv1"].cap, plans["merge_conv1"].slices) == (147, 83, 83)
    assert (plans["lstm1.weight_ih"].want, plans["lstm1.weight_ih"].cap, plans["lstm1.weight_ih"].slices) == (147, 208, 147)
    assert plans["sig_conv1"].slices == 2057  # 33 trips of train_wgrad_reduce_kernel


def test_the_batch_inside_a_larger_workspace_plans_by_the_workspace():
    inside, alone = C.shape_facts(C.INSIDE), C.shape_facts(C.INSIDE[:6])
    assert C.part_w_floats(64, 100, 9, 2, 300) > C.part_w_floats(64, 100, 9, 2, 37)
    assert not inside.wgrad_capped and not alone.wgrad_capped
    full = C.shape_facts(C.INSIDE_FULL)
    assert full.wgrad_second_trip and not full.wgrad_capped and not full.colsum_second_trip  # what the old suite reached: 57 blocks
    assert C.colsum_blocks(300 * 96) == 57


def test_sizes_cover_every_column_block_count():
    cases = group("sizes")
    assert [C.shape_facts(c.shape).nc_tail64 for c in cases] == [s % 64 != 0 for s in C.SIZES]
    blocks = {c.shape[0]: max(C.gemm_grid(p)[1] for p in C.gemm_products(*c.shape[:5])) for c in cases}
    assert blocks == {s: (4 * s + 63) // 64 for s in C.SIZES} and blocks[256] == 16
    merge = {p.name: p for p in C.wgrad_products(*C.WIDEST[:5])}["merge_conv1"]
    assert (merge.K, merge.NC) == (2560, 256)
    for c in cases:
        assert C.shape_facts(c.shape).T == 5 and C.lstm_grid(c.shape[0], c.shape[2]) == (1, c.shape[0] // 16)


def test_kmer_lengths_cover_every_k_tail():
    cases = group("kmers")
    ks = [{p.name: p for p in C.gemm_products(*c.shape[:5])}["seq_conv1"].K for c in cases]
    assert ks == [20 * k for k in range(1, 22)] and ks[0] == 20 and ks[-1] == 420
    assert {k % 16 for k in ks} == {0, 4, 8, 12}       # every tail train_gemm_kernel's loads of four can leave
    assert {k % 64 for k in ks} == set(range(0, 64, 4))  # and every tail of train_wgrad_kernel's 64 rows of K
    for c, k in zip(cases, ks):
        f = C.shape_facts(c.shape)
        assert f.k_tail16 == (k % 16 != 0) and f.k_tail64 == (k % 64 != 0)
    assert [c.shape[3] for c in cases if not C.shape_facts(c.shape).k_tail16] == [4, 8, 12, 16, 20]
    assert [c.shape[3] for c in cases if not C.shape_facts(c.shape).k_tail64] == [16]


def test_lengths_cover_every_remainder_and_step_count():
    cases = group("lengths")
    assert [C.shape_facts(c.shape).T for c in cases] == [1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5]
    for name in ("sig_conv3", "seq_conv2"):  # rows of the data-gradient product: ceil(Lin / 3) with every remainder of Lin
        lin = [C.conv_layers(32, c.shape[1], 9)[name][4] for c in cases]
        assert {x % 3 for x in lin} == {0, 1, 2}
    whh = [{p.name: p for p in C.wgrad_products(*c.shape[:5])}["lstm1.weight_hh"].R for c in cases]
    assert whh[:3] == [0, 0, 0] and all(r > 0 for r in whh[3:])  # exactly zero where and only where T = 1


def test_batch_edges_sit_on_both_sides_of_the_tiles():
    cases = group("batches")
    assert [C.shape_facts(c.shape).rows_partial_tile for c in cases] == [True, True, True, True, True, True, False, True, True, False, True]
    assert [C.lstm_grid(16, c.shape[2])[0] for c in cases] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 3]
    part = lambda n: C.part_w_floats(16, 35, 9, 2, n)
    for c in cases:
        n = c.shape[2]
        for p in C.wgrad_products(*c.shape[:5]):
            pl = C.wgrad_plan(p, part(n))
            assert pl.rows_per % 4 == 0 and (pl.slices - 1) * pl.rows_per < p.R <= pl.slices * pl.rows_per or p.R == 0
    # rows_per is rounded up to 4: a last group of 1, 2 and 3 rows occurs (fc and lstm2.weight_ih: R = n)
    assert {c.shape[2] % 4 for c in cases} == {0, 1, 2, 3}


def test_each_flag_is_true_in_one_case_and_false_in_another():
    seen = {flag: set() for flag in C.FLAGS}
    for c in C.CASES:
        f = C.shape_facts(c.shape)
        for flag in C.FLAGS:
            seen[flag].add(bool(getattr(f, flag)))
    assert all(v == {True, False} for v in seen.values()), seen
    assert {C.shape_facts(c.shape).T for c in C.CASES} >= {1, 2, 3, 4, 5, 24}


# ---- the geometry is the network's --------------------------------------------------------------------------------------------------
def test_geometry_is_the_reference_networks():
    from oracle import torch_ref

    for size, L in sorted({(c.shape[0], c.shape[1]) for c in C.CASES}):
        net = torch_ref.ConvLSTMRef(size=size, kmer_len=1, num_out=2).eval()
        shapes = {}
        hooks = [getattr(net, name).register_forward_hook(lambda m, i, o, name=name: shapes.__setitem__(name, tuple(o.shape)))
                 for name in ("sig_conv1", "sig_conv2", "sig_conv3", "seq_conv1", "seq_conv2", "merge_conv1")]
        with torch.no_grad():
            out = net(torch.zeros(2, 1, L), torch.zeros(2, 4, L))
        for h in hooks:
            h.remove()
        assert tuple(out.shape) == (2, 2)
        g = C.geometry(L)
        assert shapes == {"sig_conv1": (2, 4, g.P1), "sig_conv2": (2, 16, g.P2), "sig_conv3": (2, size, g.P3), "seq_conv1": (2, 16, g.P1),
                          "seq_conv2": (2, size, g.P3), "merge_conv1": (2, size, g.T)}, (size, L)
        assert {name: spec[5] for name, spec in C.conv_layers(size, L, 1).items()} == {name: s[2] for name, s in shapes.items()}


# ---- conditioning -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_torch_fp32_is_within_5e6_of_float64(case):
    """torch fp32 against torch float64, the case's own inputs and initial state (the one seed the GPU test uses): the worst
    per-tensor gradient error relative to the tensor's largest entry is <= 5e-6.  A case that misses is replaced in the table by
    another length or seed, never given a tolerance of its own: kmer_len 16 (train_cases.INPUT_SEED) and the colsum_capped case
    (train_cases.CAPPED, with the figures of what it replaces).  torch's fp32 convolution gradients add per-thread partials, so
    the figure of the largest case moves with torch's thread count: 4.4e-6 at 8 threads, 3.9e-6 at 12, 3.3e-6 at 16, 3.8e-6 at 32
    (and 7.3e-6 at 4, 1.6e-5 at 1 or 2: on fewer than 8 threads that one case misses)."""
    from test_gpu_train_grads import CONV_BIASES, rel, torch_step

    size, L, n, K, num_out = case.shape[:5]
    sigs, enc, labels, mask = C.case_inputs(case.shape)
    state = C.case_state(case.shape)
    _, g64, _, _ = torch_step(state, size, K, num_out, sigs, enc, labels, mask, torch.float64)
    _, g32, _, _ = torch_step(state, size, K, num_out, sigs, enc, labels, mask, torch.float32)
    errs = {name: rel(g32[name], g64[name]) for name in g64 if name not in CONV_BIASES and np.any(g64[name])}
    worst = max(errs, key=errs.get)
    print(f"{C.case_id(case.shape)}: worst {worst} {errs[worst]:.2e}")
    assert errs[worst] <= CONDITION, (worst, errs[worst])
