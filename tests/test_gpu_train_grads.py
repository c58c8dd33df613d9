"""One forward_backward of the HIP trainer (rmr_trainer_*) against torch autograd on the CPU in float64, with torch in
float32 on the same inputs as the yardstick.

The comparand is oracle/torch_ref.ConvLSTMRef in .train() mode with the trainer's own initial state.  Inputs: randn signals,
one-hot k-mers drawn per position, uniform random labels.  Gates (why they are what they are: torch fp32 measured on the
same shapes):
  loss              |loss - loss64| <= 1e-6                                   (torch fp32 <= 1.1e-7)
  gradients         max |g - g64| / max |g64| <= max(2e-5, 4 x torch fp32's)    (torch fp32 1.2e-6 .. 4.2e-6; 2.3e-5 at a
                    signal offset of 8, hence the yardstick); every parameter tensor but the six convolution biases, whose
                    gradient is mathematically zero under train-mode BatchNorm, and the tensors whose float64 gradient is
                    identically zero
  zero gradients    lstm2.weight_hh_l0 always and lstm1.weight_hh_l0 at T = 1 exactly zero; convolution biases
                    max |g| <= 1e-6 x the largest gradient entry of the network (torch fp32 <= 1.1e-8)
  running stats     max |x - x64| / max |x64| per tensor <= 2e-6              (torch fp32 <= 4.1e-7)
  logits            <= 1e-5 absolute
  repeatability     a second call from the same state gives identical bytes
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CONV_BIASES = {"sig_conv1.bias", "sig_conv2.bias", "sig_conv3.bias", "seq_conv1.bias", "seq_conv2.bias", "merge_conv1.bias"}

# (size, chunk length, N, K, num_out, variant)
SHAPES = [
    (16, 100, 37, 9, 2, "seeded"),    # N no multiple of any tile
    (64, 100, 37, 9, 2, "seeded"),
    (64, 29, 5, 9, 3, "seeded"),      # T = 1
    (32, 31, 16, 5, 2, "seeded"),     # T = 1, stride-3 remainder
    (64, 30, 17, 9, 2, "seeded"),
    (96, 200, 8, 9, 3, "seeded"),
    (128, 100, 33, 9, 3, "seeded"),
    (64, 100, 300, 9, 2, "seeded"),   # several blocks per reduction
    (64, 100, 37, 9, 2, "he"),        # torch_ref.random_model's He-scaled weights
    (64, 100, 37, 9, 2, "mask"),      # a mask that drops a third of the rows
    (64, 100, 300, 9, 2, "offset8"),  # the signal offset by +8: what catches a one-pass variance
]
IDS = ["s%d_l%d_n%d_k%d_o%d_%s" % s for s in SHAPES]


def make_inputs(size, L, n, K, num_out, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    sigs = rng.standard_normal((n, 1, L)).astype(np.float32) + np.float32(offset)
    code = rng.integers(0, 4, (n, K, L))
    enc = (code[:, :, None, :] == np.arange(4)[None, None, :, None]).astype(np.float32).reshape(n, 4 * K, L)
    labels = rng.integers(0, num_out, n).astype(np.int64)
    return sigs, enc, labels


def torch_step(state, size, K, num_out, sigs, enc, labels, mask, dtype):
    """loss, {name: grad}, state after the forward (running statistics moved), logits: torch autograd on the CPU."""
    from oracle import torch_ref

    net = torch_ref.ConvLSTMRef(size=size, kmer_len=K, num_out=num_out)
    net.load_state_dict(state, strict=True)
    net = net.to(dtype).train()
    logits = net(torch.from_numpy(sigs).to(dtype), torch.from_numpy(enc).to(dtype))
    lab = torch.from_numpy(labels)
    keep = torch.ones(len(labels), dtype=torch.bool) if mask is None else torch.from_numpy(mask)
    loss = torch.nn.functional.cross_entropy(logits[keep], lab[keep])
    loss.backward()
    grads = {k: p.grad.detach().numpy().astype(np.float64) for k, p in net.named_parameters()}
    after = {k: v.detach().numpy().astype(np.float64) for k, v in net.state_dict().items()}
    return float(loss), grads, after, logits.detach().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def run_case(shape):
    from oracle import torch_ref
    from remora_amd.train_model import Trainer

    size, L, n, K, num_out, variant = shape
    state = None
    if variant == "he":
        state = {k: v.clone() for k, v in torch_ref.random_model("conv_lstm", size, K, num_out, seed=3).state_dict().items()}
    tr = Trainer(size, K, num_out, L, max_batch=n, state=state, seed=11)
    state0 = tr.state_dict()
    sigs, enc, labels = make_inputs(size, L, n, K, num_out, seed=5, offset=8.0 if variant == "offset8" else 0.0)
    mask = (np.arange(n) % 3 != 1) if variant == "mask" else None
    loss, logits = tr.forward_backward(sigs, enc, labels, mask=mask, return_logits=True)
    grads, after = tr.grads(), tr.state_dict()
    # a second call from the same state
    tr.load_state_dict(state0)
    loss_b, logits_b = tr.forward_backward(sigs, enc, labels, mask=mask, return_logits=True)
    grads_b, after_b = tr.grads(), tr.state_dict()
    ref64 = torch_step(state0, size, K, num_out, sigs, enc, labels, mask, torch.float64)
    ref32 = torch_step(state0, size, K, num_out, sigs, enc, labels, mask, torch.float32)
    return dict(loss=loss, logits=logits, grads=grads, after=after, second=(loss_b, logits_b, grads_b, after_b), ref64=ref64, ref32=ref32,
                T=(L - 17) // 3 + 1 - 4)


def rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_loss_and_logits(shape):
    c = run_case(shape)
    loss64, _, _, logits64 = c["ref64"]
    print(f"loss hip {c['loss']:.9f} f64 {loss64:.9f} |d| {abs(c['loss'] - loss64):.2e}; torch fp32 |d| {abs(c['ref32'][0] - loss64):.2e}; "
          f"logits max|d| {np.abs(c['logits'] - logits64).max():.2e}")
    assert abs(c["loss"] - loss64) <= 1e-6
    assert np.abs(c["logits"] - logits64).max() <= 1e-5


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gradients(shape):
    c = run_case(shape)
    g64, g32 = c["ref64"][1], c["ref32"][1]
    assert list(c["grads"]) == list(g64)  # named_parameters order
    bad = []
    for name, g in c["grads"].items():
        if name in CONV_BIASES or not np.any(g64[name]):
            continue
        assert g.shape == g64[name].shape
        mine, yard = rel(g, g64[name]), rel(g32[name], g64[name])
        print(f"{name:24s} hip {mine:.2e}  torch fp32 {yard:.2e}")
        if not mine <= max(2e-5, 4 * yard):
            bad.append((name, mine, yard))
    assert not bad, bad


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_zero_gradients(shape):
    c = run_case(shape)
    g = c["grads"]
    assert not np.any(g["lstm2.weight_hh_l0"])
    if c["T"] == 1:
        assert not np.any(g["lstm1.weight_hh_l0"])
    else:
        assert np.any(g["lstm1.weight_hh_l0"])
    top = max(float(np.abs(v).max()) for v in g.values())
    for name in sorted(CONV_BIASES):
        print(f"{name:18s} max|g| {np.abs(g[name]).max():.2e} of {top:.2e}")
        assert np.abs(g[name]).max() <= 1e-6 * top, name


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_running_statistics(shape):
    c = run_case(shape)
    after64, after32 = c["ref64"][2], c["ref32"][2]
    seen = 0
    for name, v in c["after"].items():
        if name.endswith("num_batches_tracked"):
            assert int(v) == 1 == int(after64[name])
        elif "running_" in name:
            mine = rel(v.numpy(), after64[name])
            print(f"{name:24s} hip {mine:.2e}  torch fp32 {rel(after32[name], after64[name]):.2e}")
            assert mine <= 2e-6, name
            seen += 1
        else:  # forward_backward leaves the parameters alone
            assert np.array_equal(v.numpy(), after64[name].astype(np.float32)), name
    assert seen == 12


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[7], SHAPES[9]], ids=[IDS[1], IDS[2], IDS[7], IDS[9]])
def test_repeatable_bit_for_bit(shape):
    c = run_case(shape)
    loss_b, logits_b, grads_b, after_b = c["second"]
    assert np.float32(loss_b).tobytes() == np.float32(c["loss"]).tobytes()
    assert logits_b.tobytes() == c["logits"].tobytes()
    for name, g in c["grads"].items():
        assert g.tobytes() == grads_b[name].tobytes(), name
    for name, v in c["after"].items():
        assert v.numpy().tobytes() == after_b[name].numpy().tobytes(), name


def test_refusals_name_the_reason_and_launch_nothing():
    from oracle import torch_ref
    from remora_amd import RemoraError
    from remora_amd.train_model import Trainer

    tr = Trainer(16, 9, 2, 100, max_batch=8, seed=1)
    eng = tr.engine
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        sigs, enc, labels = make_inputs(16, 100, 9, 9, 2, seed=2)
        with pytest.raises(RemoraError, match="max_batch"):
            tr.forward_backward(sigs, enc, labels)
        with pytest.raises(RemoraError, match="at least 2 chunks"):
            tr.forward_backward(sigs[:1], enc[:1], labels[:1])
        with pytest.raises(RemoraError, match="multiple of 16"):
            Trainer(40, 9, 2, 100, max_batch=8, seed=1)
        conv = {k: v.clone() for k, v in torch_ref.random_model("conv_only", 64, 9, 2, seed=0).state_dict().items()}
        with pytest.raises(RemoraError, match="Conv_w_ref"):
            Trainer(64, 9, 2, 100, max_batch=8, state=conv)
        assert not any(k.startswith("train_") for k in eng.profile()), eng.profile()
    finally:
        eng.profile_enable(False)
