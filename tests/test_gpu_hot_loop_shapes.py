"""GPU tests of the shapes at which the fp32 hot loops (k_lstm.hip, k_conv_front.hip) take another path.

The Winograd front kernels choose once per launch between an input transform with zero selects for rows behind a chunk's last
(taken where the last group of four outputs reaches behind the chunk) and one without them; lstm_head_kernel runs its time loop
two steps per trip, with a first step, an odd middle step and a last step outside it.  fp32, size 64, k-mer context (4, 4),
reference-scale weights.  Every case runs a batch of 37 chunks (a ragged last block iteration, a ragged last group of sixteen)
and one of 1024 + 37: only above 1024 chunks does the LSTM run sixteen chunks per block (lstm_head_kernel; below, lstm_small_kernel
returns the same bits), and only with an iteration for every CU do the fronts stage four chunks per iteration, so that a chunk
has neighbours behind its rows at all."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KCB = (4, 4)
N, N_BIG = 37, 1024 + 37
KEYS = ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")
_cache = {}


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


def _case(cc):
    """(model, chunk arrays of N_BIG chunks, float64 logits of all of them) for one chunk context; computed once."""
    if cc not in _cache:
        import torch

        from oracle import oracle as O
        from oracle import torch_ref
        from remora_amd import synth
        from remora_amd.model_util import model_from_state

        state = synth.synth_state("conv_lstm", 64, 9, 2, seed=8, amplify=False)
        net = torch_ref.from_state(state).double()
        model = model_from_state(state, dict(chunk_context=cc, kmer_context_bases=KCB), device=0, dtype="fp32")
        L = sum(cc)
        d = synth.synth_chunks(N_BIG, L, min(20, L // 4), KCB, 2, True, shard=L)
        args = tuple(d[k] for k in KEYS)
        enc = O.compute_encoded_kmer_batch(*KCB, *args[1:])
        with torch.no_grad():
            ref = net(torch.from_numpy(args[0]).double(), torch.from_numpy(enc).double()).numpy()
        ref.setflags(write=False)
        _cache[cc] = (model, args, ref)
    return _cache[cc]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("cc,behind", [((48, 48), True), ((50, 50), False)])
def test_tail_rows_of_the_winograd_input_transforms(cc, behind):
    """(48, 48): L = 96, P1 = 92, P2 = 88, P3 = 27, seven groups of four outputs - the last one reads rows 72 + phase + 3 j, up to
    89 of sig_conv3's 88 rows and up to 95 of seq_conv2's 92: the body with the zero selects.  (50, 50): P1 = 96, P2 = 92, the same
    reach ends on the last row: the select-free body.  Both within 1e-4 of the float64 network and 2e-5 of the direct forms; and
    chunk 0 - whose missing rows, without the selects, are the first rows of chunk 1 in the staged image - returns the same bits
    whatever its three neighbours in the iteration are."""
    L = sum(cc)
    P1 = L - 4
    P2, P3 = P1 - 4, (P1 - 4 - 9) // 3 + 1
    ngrp = (P3 + 3) // 4
    assert (12 * (ngrp - 1) + 2 + 15 > P2 - 1) == behind and (12 * (ngrp - 1) + 2 + 21 > P1 - 1) == behind
    model, args, ref = _case(cc)
    for n in (N, N_BIG):
        sub = [a[:n] for a in args]
        out = model.infer_chunks(*sub, KCB)
        direct = _direct(lambda: model.infer_chunks(*sub, KCB))
        e64, edir = float(np.abs(out - ref[:n]).max()), float(np.abs(out - direct).max())
        print(f"cc={cc} n={n}: max|out - float64| = {e64:.3e}, max|out - direct| = {edir:.3e}")
        assert e64 <= 1e-4, (cc, n, e64)
        assert edir <= 2e-5, (cc, n, edir)
        assert not np.array_equal(out, direct), (cc, n, "RMR_WINOGRAD=0 did not select another kernel")
        # neighbours B: other chunks of the batch, their signal scaled up so that a row leaking into chunk 0 cannot hide
        other = [a[:n].copy() for a in args]
        for k in KEYS[1:]:
            i = KEYS.index(k)
            other[i][1:4] = args[i][N_BIG - 3 : N_BIG]
        other[0][1:4] = 8.0 * args[0][N_BIG - 3 : N_BIG]
        out_b = model.infer_chunks(*other, KCB)
        assert np.array_equal(_bits(out_b[0]), _bits(out[0])), (cc, n, out[0], out_b[0])
        assert np.array_equal(_bits(out_b[4:]), _bits(out[4:])), (cc, n)
        assert not np.array_equal(out_b[1:4], out[1:4])


@pytest.mark.parametrize("cc,T", [((14, 15), 1), ((16, 16), 2), ((17, 18), 3), ((48, 48), 23)])
def test_lstm_step_counts(cc, T):
    """Chunk lengths 29, 32, 35 and 96: one, two, three and 23 LSTM steps - the first step alone, first and last, one odd middle
    step, ten pairs and an odd one.  Within 1e-4 of the float64 network; the same chunks return the same bits in a batch of 5, of
    37 and of 1024 + 37 (sixteen chunks per block, the last group ragged)."""
    L = sum(cc)
    assert (L - 8 - 9) // 3 + 1 - 4 == T
    model, args, ref = _case(cc)
    big = model.infer_chunks(*args, KCB)
    e_big = float(np.abs(big - ref).max())
    print(f"cc={cc} T={T} n={N_BIG}: max|out - float64| = {e_big:.3e}")
    assert e_big <= 1e-4, (cc, N_BIG, e_big)
    assert big.std(axis=0).min() > 1e-6  # the chunks are told apart
    for n in (5, N):
        out = model.infer_chunks(*[a[:n] for a in args], KCB)
        e = float(np.abs(out - ref[:n]).max())
        print(f"cc={cc} T={T} n={n}: max|out - float64| = {e:.3e}")
        assert e <= 1e-4, (cc, n, e)
        assert np.array_equal(_bits(out), _bits(big[:n])), (cc, n, float(np.abs(out - big[:n]).max()))
    tail = model.infer_chunks(*[a[N_BIG - 5 :] for a in args], KCB)  # the chunks of the ragged last group
    assert np.array_equal(_bits(tail), _bits(big[N_BIG - 5 :])), cc
