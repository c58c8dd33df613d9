"""One forward_backward of the HIP trainer at every size, k-mer length, class count, short chunk length and batch edge the
trainer accepts, at the batches that take the second trips and the caps of its fixed-order reductions, and inside a workspace
larger than the batch - the cases of tests/train_cases.py, which tests/test_host_train_cases.py shows to take the paths they are
named after - against torch autograd on the CPU in float64, with torch fp32 as the yardstick.

The gates are those of tests/test_gpu_train_grads.py, applied unchanged (`gates`): loss <= 1e-6, logits <= 1e-5, per-tensor
gradients max(2e-5, 4 x torch fp32's), convolution biases <= 1e-6 x the largest gradient entry, running statistics <= 2e-6,
lstm2.weight_hh_l0 exactly zero, lstm1.weight_hh_l0 exactly zero where and only where T = 1, num_batches_tracked == 1, parameters
untouched; and nothing in the gradients is non-finite.  Then: history independence of a batch inside a larger workspace, the
two residencies of the inputs, repeatability where the reductions have the most partials, the refusals (labels outside
0..num_out-1 among them), and one optimiser step further into the inference kernels."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import train_cases as C
from test_gpu_train_grads import CONV_BIASES, make_inputs, rel, torch_step

pytestmark = pytest.mark.gpu

IDS = [C.case_id(c.shape) for c in C.CASES]
REPEATED = (C.SECOND_TRIP, C.WIDEST)  # a second call from the same state: the paths with the most partials


def trainer_for(shape, **kw):
    from remora_amd.train_model import Trainer

    size, L, n, K, num_out = shape[:5]
    return Trainer(size, K, num_out, L, max_batch=shape[6] if len(shape) > 6 else n, seed=C.STATE_SEED, **kw)


def refs(shape, state0):
    size, L, n, K, num_out = shape[:5]
    sigs, enc, labels, mask = C.case_inputs(shape)
    return (torch_step(state0, size, K, num_out, sigs, enc, labels, mask, torch.float64),
            torch_step(state0, size, K, num_out, sigs, enc, labels, mask, torch.float32))


def one_call(tr, shape):
    sigs, enc, labels, mask = C.case_inputs(shape)
    loss, logits = tr.forward_backward(sigs, enc, labels, mask=mask, return_logits=True)
    return dict(loss=loss, logits=logits, grads=tr.grads(), after=tr.state_dict())


@functools.lru_cache(maxsize=None)
def run_case(shape):
    tr = trainer_for(shape)
    state0 = tr.state_dict()
    c = one_call(tr, shape)
    if shape in REPEATED:
        tr.load_state_dict(state0)
        c["second"] = one_call(tr, shape)
    c["ref64"], c["ref32"] = refs(shape, state0)
    c["T"] = C.shape_facts(shape).T
    return c


def same_bytes(a, b):
    assert np.float32(a["loss"]).tobytes() == np.float32(b["loss"]).tobytes()
    assert np.asarray(a["logits"]).tobytes() == np.asarray(b["logits"]).tobytes()
    assert list(a["grads"]) == list(b["grads"]) and list(a["after"]) == list(b["after"])
    for name, g in a["grads"].items():
        assert g.tobytes() == b["grads"][name].tobytes(), name
    for name, v in a["after"].items():
        assert v.numpy().tobytes() == b["after"][name].numpy().tobytes(), name


def gates(c, tag):
    """Every gate of tests/test_gpu_train_grads.py on one call's results; returns (worst gradient error, torch fp32's worst)."""
    loss64, g64, after64, logits64 = c["ref64"]
    loss32, g32, after32, _ = c["ref32"]
    # test_loss_and_logits
    print(f"{tag}: loss hip {c['loss']:.9f} f64 {loss64:.9f} |d| {abs(c['loss'] - loss64):.2e}; torch fp32 |d| {abs(loss32 - loss64):.2e}; "
          f"logits max|d| {np.abs(c['logits'] - logits64).max():.2e}")
    assert np.isfinite(c["loss"]) and np.isfinite(c["logits"]).all()
    assert abs(c["loss"] - loss64) <= 1e-6
    assert np.abs(c["logits"] - logits64).max() <= 1e-5
    # rows must not leak: nothing non-finite in any gradient
    for name, g in c["grads"].items():
        assert np.isfinite(g).all(), name
    # test_gradients
    assert list(c["grads"]) == list(g64)
    bad, worst, worst32 = [], (0.0, ""), 0.0
    for name, g in c["grads"].items():
        if name in CONV_BIASES or not np.any(g64[name]):
            continue
        assert g.shape == g64[name].shape
        mine, yard = rel(g, g64[name]), rel(g32[name], g64[name])
        print(f"{name:24s} hip {mine:.2e}  torch fp32 {yard:.2e}")
        worst, worst32 = max(worst, (mine, name)), max(worst32, yard)
        if not mine <= max(2e-5, 4 * yard):
            bad.append((name, mine, yard))
    print(f"GRAD {tag}: hip {worst[0]:.2e} ({worst[1]})  torch fp32 {worst32:.2e}")
    assert not bad, bad
    # test_zero_gradients
    g = c["grads"]
    assert not np.any(g["lstm2.weight_hh_l0"])
    assert np.any(g["lstm1.weight_hh_l0"]) == (c["T"] != 1)
    top = max(float(np.abs(v).max()) for v in g.values())
    for name in sorted(CONV_BIASES):
        assert np.abs(g[name]).max() <= 1e-6 * top, (name, float(np.abs(g[name]).max()), top)
    # test_running_statistics
    seen, worst_stat = 0, 0.0
    for name, v in c["after"].items():
        if name.endswith("num_batches_tracked"):
            assert int(v) == 1 == int(after64[name])
        elif "running_" in name:
            mine = rel(v.numpy(), after64[name])
            worst_stat = max(worst_stat, mine)
            assert mine <= 2e-6, (name, mine, rel(after32[name], after64[name]))
            seen += 1
        else:
            assert np.array_equal(v.numpy(), after64[name].astype(np.float32)), name
    assert seen == 12
    print(f"{tag}: running statistics hip {worst_stat:.2e}")
    return worst[0], worst32


@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_every_gate_at_every_case(case):
    print(f"{case.group}: {case.path}; {C.shape_facts(case.shape)}")
    gates(run_case(case.shape), C.case_id(case.shape))


@pytest.mark.parametrize("shape", REPEATED, ids=[C.case_id(s) for s in REPEATED])
def test_repeatable_where_the_partials_are_most(shape):
    c = run_case(shape)
    same_bytes(c, c["second"])


def test_a_batch_inside_a_larger_workspace_does_not_depend_on_history():
    """37 chunks on a trainer of max_batch 300, from a saved state; then 300 chunks; then the state again and the same 37: equal
    bytes, and both runs pass the float64 gates.  (Not compared with a trainer of max_batch 37: train_wgrad's cap follows the
    workspace, so the summation order may differ.)"""
    tr = trainer_for(C.INSIDE)
    state0 = tr.state_dict()
    first = one_call(tr, C.INSIDE)
    tr.load_state_dict(state0)
    full = one_call(tr, C.INSIDE_FULL)
    tr.load_state_dict(state0)
    again = one_call(tr, C.INSIDE)
    same_bytes(first, again)
    ref64, ref32 = refs(C.INSIDE, state0)
    for c, tag in ((first, "first"), (again, "after 300")):
        c.update(ref64=ref64, ref32=ref32, T=24)
        gates(c, "inside " + tag)
    full["ref64"], full["ref32"] = refs(C.INSIDE_FULL, state0)
    full["T"] = 24
    gates(full, "the 300 between")


def test_device_inputs_give_the_bytes_of_host_inputs():
    """(64, 100, 37, mask): numpy inputs; the same arrays as device tensors (a torch.bool mask) through Trainer.forward_backward;
    and the same device tensors through rmr_trainer_forward_backward itself with the caller's logits filled with NaN before the
    call - every entry is written, and loss, logits and gradients have equal bytes in all three."""
    from remora_amd import _lib as L

    tr = trainer_for(C.RESIDENCY)
    state0 = tr.state_dict()
    sigs, enc, labels, mask = C.case_inputs(C.RESIDENCY)
    host = one_call(tr, C.RESIDENCY)
    dev = tr.engine.torch_device
    d_sigs, d_enc, d_labels, d_mask = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sigs, enc, labels, mask))
    assert d_mask.dtype == torch.bool
    tr.load_state_dict(state0)
    loss, logits = tr.forward_backward(d_sigs, d_enc, d_labels, mask=d_mask, return_logits=True)
    assert logits.is_cuda
    same_bytes(host, dict(loss=loss, logits=logits.cpu().numpy(), grads=tr.grads(), after=tr.state_dict()))
    tr.load_state_dict(state0)
    own = torch.full((37, 2), float("nan"), dtype=torch.float32, device=dev)
    m8 = d_mask.to(torch.uint8).contiguous()
    out = ctypes.c_float(float("nan"))
    L.check(tr._lib.rmr_trainer_forward_backward(tr._h, d_sigs.data_ptr(), d_enc.data_ptr(), d_labels.data_ptr(), m8.data_ptr(), 37, ctypes.byref(out),
                                                 own.data_ptr(), L.MEM_DEVICE))
    own = own.cpu().numpy()
    assert np.isfinite(own).all()
    raw = dict(loss=out.value, logits=own, grads=tr.grads(), after=tr.state_dict())
    same_bytes(host, raw)
    raw["ref64"], raw["ref32"] = refs(C.RESIDENCY, state0)
    raw["T"] = 24
    gates(raw, "device inputs")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_shape_refusals_name_the_reason_and_launch_nothing():
    from remora_amd import RemoraError
    from remora_amd.train_model import Trainer

    tr = Trainer(16, 9, 2, 100, max_batch=8, seed=1)
    eng = tr.engine
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        for size in (272, 8):
            with pytest.raises(RemoraError, match=f"multiple of 16 from 16 to 256, got {size}"):
                Trainer(size, 9, 2, 100, max_batch=8, seed=1)
        for k in (0, 22):
            with pytest.raises(RemoraError, match=f"k-mer length of 1..21, got {k}"):
                Trainer(16, k, 2, 100, max_batch=8, seed=1)
        for o in (1, 17):
            with pytest.raises(RemoraError, match=f"num_out of 2..16, got {o}"):
                Trainer(16, 9, o, 100, max_batch=8, seed=1)
        with pytest.raises(RemoraError, match="chunk length of at least 29, got 28"):
            Trainer(16, 9, 2, 28, max_batch=8, seed=1)
        assert not any(k.startswith("train_") for k in eng.profile()), eng.profile()
    finally:
        eng.profile_enable(False)


LABEL_SHAPE = (16, 35, 17, 9, 3, "seeded")


@pytest.mark.parametrize("bad", [-1, 3], ids=["minus1", "num_out"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_a_label_out_of_range_is_refused_and_moves_nothing(where, bad):
    """A label of -1 or num_out in a row of the loss: refused by name ("label ... outside 0..num_out-1"), with the gradients of
    the call before, the running statistics and num_batches_tracked left as they were - in both residencies.  Host labels are
    refused before anything is launched.  Device labels are found by the step's first kernel, and every later store to a
    gradient or a running statistic is held; the host learns of it with the loss.  The same label in a row that the mask drops
    is no reason to refuse (torch's loss does not see it either), and the call after a refusal is an ordinary one."""
    from remora_amd import RemoraError

    tr = trainer_for(LABEL_SHAPE)
    eng, dev = tr.engine, tr.engine.torch_device
    sigs, enc, labels, _ = C.case_inputs(LABEL_SHAPE)
    to = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)) if where == "device" else (lambda a: a)
    loss0 = tr.forward_backward(to(sigs), to(enc), to(labels))
    grads0, state1 = tr.grads(), tr.state_dict()
    assert int(state1["sig_bn1.num_batches_tracked"]) == 1 and any(np.any(g) for g in grads0.values())
    wrong = labels.copy()
    wrong[5] = bad
    sigs2 = sigs + np.float32(0.5)  # another batch: a step that went through would move every gradient and statistic
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        with pytest.raises(RemoraError, match=rf"label {bad} of chunk 5 is outside 0\.\.num_out-1"):
            tr.forward_backward(to(sigs2), to(enc), to(wrong))
        launched = [k for k in eng.profile() if k.startswith("train_")]
    finally:
        eng.profile_enable(False)
    assert bool(launched) == (where == "device"), launched
    grads1, state2 = tr.grads(), tr.state_dict()
    for name, g in grads0.items():
        assert g.tobytes() == grads1[name].tobytes(), name
    assert list(state1) == list(state2)
    for name, v in state1.items():
        assert v.numpy().tobytes() == state2[name].numpy().tobytes(), name
    # the mask takes the row out of the loss: accepted, and the loss is that of any other label there
    mask = np.arange(len(labels)) != 5
    tr.load_state_dict(state1)
    masked_bad = tr.forward_backward(to(sigs), to(enc), to(wrong), mask=to(mask))
    tr.load_state_dict(state1)
    masked_ok = tr.forward_backward(to(sigs), to(enc), to(labels), mask=to(mask))
    assert np.float32(masked_bad).tobytes() == np.float32(masked_ok).tobytes()
    # the call after the refusal: the first call's bytes from the first call's state
    nets_state = C.case_state(LABEL_SHAPE)
    tr.load_state_dict(nets_state)
    assert np.float32(tr.forward_backward(to(sigs), to(enc), to(labels))).tobytes() == np.float32(loss0).tobytes()
    for name, g in tr.grads().items():
        assert g.tobytes() == grads0[name].tobytes(), name
    assert int(tr.state_dict()["sig_bn1.num_batches_tracked"]) == 1


# ---- one step further ---------------------------------------------------------------------------------------------------------------
STEPPED = (C.WIDEST, (16, 35, 9, 1, 2, "seeded"), (16, 35, 9, 21, 2, "seeded"), (16, 33, 21, 9, 16, "seeded"))


@pytest.mark.parametrize("shape", STEPPED, ids=[C.case_id(s) for s in STEPPED])
def test_one_step_further_into_the_inference_kernels(shape):
    """forward_backward and one optimizer_step, then eval_model() (the inference kernels on the stepped weights and the moved
    running statistics) on 16 fresh chunks beside the float64 network, stepped by torch.optim.AdamW with the trainer's settings, in
    eval mode: <= 1e-4, the gate of test_five_training_steps_beside_torch_float64."""
    from oracle import torch_ref
    from remora_amd.train_model import ADAMW_DEFAULTS

    size, L, n, K, num_out = shape[:5]
    assert shape in [c.shape for c in C.CASES]
    tr = trainer_for(shape)
    net = torch_ref.ConvLSTMRef(size=size, kmer_len=K, num_out=num_out)
    net.load_state_dict(tr.state_dict(), strict=True)
    net = net.double().train()
    o = ADAMW_DEFAULTS
    opt = torch.optim.AdamW(net.parameters(), lr=o["lr"], betas=o["betas"], eps=o["eps"], weight_decay=o["weight_decay"])
    sigs, enc, labels, mask = C.case_inputs(shape)
    assert mask is None
    loss = tr.step(sigs, enc, labels)
    loss64 = torch.nn.functional.cross_entropy(net(torch.from_numpy(sigs).double(), torch.from_numpy(enc).double()), torch.from_numpy(labels))
    loss64.backward()
    opt.step()
    assert abs(loss - float(loss64)) <= 1e-6
    sigs, enc, _ = make_inputs(size, L, 16, K, num_out, seed=999)
    with torch.no_grad():
        want = net.eval()(torch.from_numpy(sigs).double(), torch.from_numpy(enc).double()).numpy()
    got = tr.eval_model()(sigs, enc).numpy()
    print(f"{C.case_id(shape)}: eval logits max|d| {np.abs(got - want).max():.2e} of max {np.abs(want).max():.2e}")
    assert got.shape == want.shape == (16, num_out)
    assert np.abs(got - want).max() <= 1e-4
