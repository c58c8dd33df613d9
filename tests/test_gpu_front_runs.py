"""GPU parity of the shipped Winograd front kernels (k_conv_front.hip: sig3_front_wino_kernel, seq2_front_wino_kernel) on chunks
built to reach the corners of the sequence producer: bases of one to six samples, bases that start before the chunk or end behind
it, signal positions no base owns, lengths of zero and beyond max_seq_len, the last chunk of a partial block iteration, and small
batches.  The Winograd fronts are held to the direct form (RMR_WINOGRAD=0) on every chunk and to the float64 network on the
well-formed ones, and a chunk's bits do not depend on the batch it arrives in."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, KB, KA, MAXLEN = 100, 4, 4, 20
SEQ_W, MAP_W = MAXLEN + KB + KA, MAXLEN + 1


def _direct(fn):
    """fn() with the direct forms selected (RMR_WINOGRAD=0); the variable's earlier state is restored afterwards."""
    old = os.environ.get("RMR_WINOGRAD")
    os.environ["RMR_WINOGRAD"] = "0"
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["RMR_WINOGRAD"]
        else:
            os.environ["RMR_WINOGRAD"] = old


def _chunk(rng, kind):
    """(map row, length, well_formed) of one chunk of the given kind; the map row is MAP_W wide."""
    mp = np.zeros(MAP_W, np.int64)
    if kind == "short":  # bases of 1..6 samples from 0, the rest of the chunk in one base
        n = int(rng.integers(2, MAXLEN + 1))
        cuts = np.cumsum(rng.integers(1, 7, n - 1))
        cuts = cuts[cuts < L]
        n = len(cuts) + 1
        mp[1:n] = cuts
        mp[n] = L
        return mp, n, True
    if kind == "long":  # one base over more than the whole chunk, or two bases, one of them reaching past each end
        if rng.random() < 0.5:
            mp[0], mp[1] = -int(rng.integers(1, 40)), L + int(rng.integers(1, 40))
            return mp, 1, False
        mp[0], mp[1], mp[2] = -int(rng.integers(1, 40)), int(rng.integers(1, L)), L + int(rng.integers(1, 40))
        return mp, 2, False
    if kind == "gaps":  # the bases cover only a window: positions before and behind it belong to no base
        n = int(rng.integers(1, MAXLEN + 1))
        lo, hi = sorted(rng.choice(np.arange(0, L + 1), 2, replace=False))
        inner = np.sort(rng.choice(np.arange(lo + 1, hi), min(n - 1, hi - lo - 1), replace=False)) if hi - lo > 1 else []
        n = len(inner) + 1
        mp[0], mp[1:n], mp[n] = lo, inner, hi
        return mp, n, True
    if kind == "empty":  # length 0
        return mp, 0, True
    if kind == "overlong":  # a length beyond max_seq_len (the kernels take max_seq_len of it)
        cuts = np.sort(rng.choice(np.arange(1, L), MAXLEN - 1, replace=False))
        mp[1:MAXLEN] = cuts
        mp[MAXLEN] = L
        return mp, MAXLEN + int(rng.integers(1, 30)), False
    raise ValueError(kind)


def _edge_chunks(n, seed):
    rng = np.random.default_rng(seed)
    kinds = ("short", "long", "gaps", "empty", "overlong")
    signal = rng.standard_normal((n, 1, L), dtype=np.float32)
    seqs = np.full((n, SEQ_W), -1, np.int8)
    maps = np.zeros((n, MAP_W), np.int16)
    lens = np.zeros(n, np.int16)
    ok = np.zeros(n, bool)
    for i in range(n):
        mp, ln, good = _chunk(rng, kinds[i % len(kinds)] if i % 3 else kinds[int(rng.integers(0, len(kinds)))])
        maps[i], lens[i], ok[i] = mp, ln, good
        nb = min(ln, MAXLEN) + KB + KA
        seqs[i, :nb] = rng.integers(0, 4, nb)
        if rng.random() < 0.2:  # a missing base (-1) inside the k-mer window: its slot contributes nothing
            seqs[i, int(rng.integers(0, nb))] = -1
    return dict(signal=signal, sequence=seqs, sequence_to_signal_mapping=maps, sequence_lengths=lens), ok


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 31, 257, 1023, 1024, 4099])
def test_winograd_fronts_on_edge_chunks(n):
    """Winograd fronts against the direct form (<= 2e-5) on every chunk and against the float64 network (<= 1e-4, and within the
    direct form's rounding) on the well-formed chunks.  Batch sizes: one to a few chunks (one block iteration of one to three
    chunks), up to 1024 (the small-batch plan), and 4099 (a partial last iteration)."""
    import torch

    from oracle import oracle as O
    from oracle import torch_ref
    from remora_amd.model_util import model_from_state

    net = torch_ref.random_model("conv_lstm", 64, 9, 2, seed=3)
    state = {k: v.numpy() for k, v in net.state_dict().items()}
    model = model_from_state(state, dict(chunk_context=(L // 2, L - L // 2), kmer_context_bases=(KB, KA)), device=0, dtype="fp32")
    d, ok = _edge_chunks(n, seed=900 + n)
    args = (d["signal"], d["sequence"], d["sequence_to_signal_mapping"], d["sequence_lengths"], (KB, KA))
    out = model.infer_chunks(*args)
    direct = _direct(lambda: model.infer_chunks(*args))
    assert np.isfinite(out).all()
    assert np.abs(out - direct).max() <= 2e-5, (n, float(np.abs(out - direct).max()))
    assert not np.array_equal(out, direct), (n, "RMR_WINOGRAD=0 did not select another kernel")
    if ok.any():
        idx = np.flatnonzero(ok)
        sub = [a[idx] for a in args[:4]]
        # the encoder takes the signal length from its first chunk's map: lead with one whose bases end at the chunk's end
        a_seq, a_map = np.zeros((1, SEQ_W), np.int8), np.zeros((1, MAP_W), np.int16)
        a_map[0, 1] = L
        enc = O.compute_encoded_kmer_batch(KB, KA, np.concatenate([a_seq, sub[1]]), np.concatenate([a_map, sub[2]]),
                                           np.concatenate([np.ones(1, np.int16), sub[3]]))[1:]
        net64 = torch_ref.build("conv_lstm", 64, 9, 2).double()
        net64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in net.state_dict().items()})
        with torch.no_grad():
            exact = net64(torch.from_numpy(sub[0]).double(), torch.from_numpy(enc).double()).numpy()
        ew, ed = float(np.abs(out[idx] - exact).max()), float(np.abs(direct[idx] - exact).max())
        assert ew <= 1e-4, (n, ew, ed)
        assert ew <= 3.0 * ed + 2e-6, (n, ew, ed)


def test_winograd_fronts_batch_independent():
    """The bits of a chunk do not depend on its neighbours or on how many chunks a block iteration holds (the small-batch plan
    shrinks it): every slice of an edge batch returns the rows of the whole batch."""
    from oracle import torch_ref
    from remora_amd.model_util import model_from_state

    net = torch_ref.random_model("conv_lstm", 64, 9, 2, seed=4)
    state = {k: v.numpy() for k, v in net.state_dict().items()}
    model = model_from_state(state, dict(chunk_context=(L // 2, L - L // 2), kmer_context_bases=(KB, KA)), device=0, dtype="fp32")
    d, _ = _edge_chunks(20000, seed=77)
    args = (d["signal"], d["sequence"], d["sequence_to_signal_mapping"], d["sequence_lengths"])
    out = model.infer_chunks(*args, (KB, KA))
    for start, m in ((0, 1), (3, 2), (10, 3), (100, 5), (1000, 1024), (5000, 4099), (19999, 1)):
        part = model.infer_chunks(*[a[start : start + m] for a in args], (KB, KA))
        assert np.array_equal(part, out[start : start + m]), (start, m)
