"""GPU tests of Conv_w_ref (`conv_only`) at every chunk length it admits.

fc is Linear(size * 3, num_out): rmr_pack.cpp admits the chunk lengths that end in three positions, L = 95 ... 106, and
refuses 94 and 107 by name.  The suite's other Conv_w_ref tests run L = 100, whose layer lengths (shared with 98 and 99) are all
multiples of four; the other nine give the tiled kernels a ragged last group of four outputs - Winograd F(4, 5) at 64 input channels (merge_conv2), the polyphase stride-3
Winograd at 32 (seq_conv3), merge_conv1 at T = 1 (mod 4), the 11-tap signal front on the matrix cores at a row count other than
80, the stride-2 layers with and without an input row they do not read, and the streamed convolutions of the sizes above 64.

     L   P1   P2   P3    T   T2   T3      (P1 = L - 10 rows of sig_conv1 / seq_conv1, P2 = P1 - 10 of sig_conv2 / seq_conv2,
    95   85   75   23   19   15    7       P3 = (P2 - 9) // 3 + 1 of sig_conv3 / seq_conv3, T = P3 - 4 of merge_conv1,
    96   86   76   23   19   15    7       T2 = T - 4 of merge_conv2, T3 = (T2 - 3) // 2 + 1 of merge_conv3; merge_conv4
    97   87   77   23   19   15    7       gives (T3 - 3) // 2 + 1 = 3 at every one of them.  T2 even: merge_conv3 does not read
    98   88   78   24   20   16    7       the last row of its input; T3 even: merge_conv4 does not.)
    99   89   79   24   20   16    7
   100   90   80   24   20   16    7
   101   91   81   25   21   17    8
   102   92   82   25   21   17    8
   103   93   83   25   21   17    8
   104   94   84   26   22   18    8
   105   95   85   26   22   18    8
   106   96   86   26   22   18    8

fp32, k-mer context (4, 4), max_seq_len 20, num_out alternating between 2 and 3.  The reference is the oracle's torch.nn network
in float64 on the oracle's encoding of the same chunk arrays.  Every case runs a batch of 37 chunks and one of 1024 + 37: only
with an iteration for every CU do the fronts stage four chunks per iteration, so that a chunk has neighbours behind its rows.

Tolerances: 1e-4 against float64 (the project's gate) and 2e-5 between the Winograd and the direct forms (the load-time guard's
kWinogradTol) at reference-scale weights; 1e-4 + 3 max|oracle fp32 - oracle float64| on the same chunks for the amplified
networks (test_large_models_on_long_chunk_contexts' allowance).

Measured on an MI355X (max over the twelve lengths and both batch sizes; sizes 32 / 96 / 176 over five lengths):
    size 64 reference scale   max|out - float64| 7.7e-7, max|out - direct| 4.8e-7 (never 0); the guard keeps Winograd at every length
    size 64 amplified         max|out - float64| 3.6e-6 (direct forms 4.7e-6) against tolerances of 1.03e-4 ... 1.07e-4; the guard
                              keeps Winograd at every length: its probe's max|winograd - direct| is 4.3e-6, 4.1e-6, 3.0e-6, 4.5e-6,
                              3.6e-6, 9.1e-6, 2.7e-6, 4.1e-6, 4.9e-6, 7.5e-6, 3.3e-6, 1.1e-5 at L = 95 ... 106 (tol 2e-5)
    size 32 / 96 / 176        max|out - float64| 3.1e-6 / 4.6e-6 / 6.6e-6 against 1.03e-4"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KCB = (4, 4)
MSL = 20
N, N_BIG = 37, 1024 + 37
KEYS = ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")
LENGTHS = tuple(range(95, 107))
CLASS_LENGTHS = (95, 98, 101, 104, 106)  # one length per (P3, T, T2, T3) class and both ends
# the docstring's table: L -> (P1, P2, P3, T, T2, T3)
TABLE = {
    95: (85, 75, 23, 19, 15, 7), 96: (86, 76, 23, 19, 15, 7), 97: (87, 77, 23, 19, 15, 7),
    98: (88, 78, 24, 20, 16, 7), 99: (89, 79, 24, 20, 16, 7), 100: (90, 80, 24, 20, 16, 7),
    101: (91, 81, 25, 21, 17, 8), 102: (92, 82, 25, 21, 17, 8), 103: (93, 83, 25, 21, 17, 8),
    104: (94, 84, 26, 22, 18, 8), 105: (95, 85, 26, 22, 18, 8), 106: (96, 86, 26, 22, 18, 8),
}
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


def _geometry(L):
    """(P1, P2, P3, T, T2, T3, T4) of Conv_w_ref at chunk length L (models/Conv_w_ref.py: kernel sizes 11, 11, 9 / 3, 5, 5, 3 / 2, 3 / 2)."""
    P1 = L - 10
    P2 = P1 - 10
    P3 = (P2 - 9) // 3 + 1
    T = P3 - 4
    T2 = T - 4
    T3 = (T2 - 3) // 2 + 1
    return P1, P2, P3, T, T2, T3, (T3 - 3) // 2 + 1


def _num_out(L):
    return 2 + (L - 95) % 2


def _chunks(L):
    """Chunk arrays of N_BIG chunks of L samples and the oracle's encoding of them; computed once per length."""
    if ("chunks", L) not in _cache:
        from oracle import oracle as O
        from remora_amd import synth

        d = synth.synth_chunks(N_BIG, L, MSL, KCB, 2, True, shard=L)
        args = tuple(d[k] for k in KEYS)
        enc = O.compute_encoded_kmer_batch(*KCB, *args[1:])
        _cache["chunks", L] = (args, enc)
    return _cache["chunks", L]


def _case(L, size, amplify):
    """(model, chunk arrays of N_BIG chunks, float64 logits of all of them, max |oracle fp32 - oracle float64|) of one network
    at one chunk length; computed once."""
    key = (L, size, amplify)
    if key not in _cache:
        import torch

        from oracle import torch_ref
        from remora_amd import synth
        from remora_amd.model_util import model_from_state

        state = synth.synth_state("conv_only", size, 9, _num_out(L), seed=L, amplify=amplify)
        net = torch_ref.from_state(state)
        args, enc = _chunks(L)
        with torch.no_grad():
            ref32 = net(torch.from_numpy(args[0]), torch.from_numpy(enc)).numpy()
            ref = net.double()(torch.from_numpy(args[0]).double(), torch.from_numpy(enc).double()).numpy()
        ref.setflags(write=False)
        model = model_from_state(state, dict(chunk_context=(L // 2, L - L // 2), kmer_context_bases=KCB), device=0, dtype="fp32")
        _cache[key] = (model, args, ref, float(np.abs(ref32 - ref).max()))
    return _cache[key]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _assert_batch_independent(model, args, big, tag):
    """The first 5 chunks, the first N and the last 5 (the ragged last group) return the bits they have inside N_BIG."""
    for n in (5, N):
        out = model.infer_chunks(*[a[:n] for a in args], KCB)
        assert np.array_equal(_bits(out), _bits(big[:n])), (tag, n, float(np.abs(out - big[:n]).max()))
    tail = model.infer_chunks(*[a[N_BIG - 5 :] for a in args], KCB)
    assert np.array_equal(_bits(tail), _bits(big[N_BIG - 5 :])), (tag, "tail", float(np.abs(tail - big[N_BIG - 5 :]).max()))


def test_the_table_of_layer_lengths():
    """The docstring's table is what the geometry gives; three final positions at 95 ... 106 and nowhere else nearby; nine of the
    twelve lengths have a layer length that is no multiple of four (98 ... 100 have none), every residue of T mod 4 occurs, and T2 and T3 are each even at
    some lengths and odd at others (a stride-2 layer with and without an unread last input row)."""
    for L in LENGTHS:
        assert _geometry(L) == TABLE[L] + (3,), L
    assert _geometry(94)[-1] == 2 and _geometry(107)[-1] == 4
    ragged = [L for L in LENGTHS if any(v % 4 for v in TABLE[L][2:5])]
    assert ragged == [95, 96, 97, 101, 102, 103, 104, 105, 106]
    assert {TABLE[L][3] % 4 for L in LENGTHS} == {0, 1, 2, 3}
    assert {TABLE[L][4] % 2 for L in LENGTHS} == {0, 1} and {TABLE[L][5] % 2 for L in LENGTHS} == {0, 1}
    assert {TABLE[L][2:] for L in CLASS_LENGTHS} == {TABLE[L][2:] for L in LENGTHS}


@pytest.mark.parametrize("L", LENGTHS)
def test_size_64_reference_scale_winograd_against_direct_and_float64(L):
    """Reference-scale weights, the scale at which the load-time guard keeps the Winograd forms: within 1e-4 of the float64
    network and 2e-5 of the direct forms, and not the direct forms' bits."""
    model, args, ref, _ = _case(L, 64, False)
    assert model.numerics["winograd"] == 1, model.numerics
    for n in (N, N_BIG):
        sub = [a[:n] for a in args]
        out = model.infer_chunks(*sub, KCB)
        direct = _direct(lambda: model.infer_chunks(*sub, KCB))
        e64, edir = float(np.abs(out - ref[:n]).max()), float(np.abs(out - direct).max())
        print(f"L={L} n={n}: max|out - float64| = {e64:.3e}, max|out - direct| = {edir:.3e}, max|direct - float64| = "
              f"{float(np.abs(direct - ref[:n]).max()):.3e}")
        assert out.shape == (n, _num_out(L))
        assert e64 <= 1e-4, (L, n, e64)
        assert edir <= 2e-5, (L, n, edir)
        assert not np.array_equal(out, direct), (L, n, "RMR_WINOGRAD=0 did not select another kernel")
        assert out.std(axis=0).min() > 1e-6, (L, n)  # the chunks are told apart


@pytest.mark.parametrize("L", LENGTHS)
def test_size_64_amplified_network(L):
    """The amplified network (every layer's error reaches the logits) under whichever form the guard chose and under the direct
    forms, against float64 with the oracle's own fp32 error as the scale of the allowance."""
    model, args, ref, e32 = _case(L, 64, True)
    tol = 1e-4 + 3.0 * e32
    print(f"L={L}: guard {model.winograd_form} (max_abs_diff {model.numerics['max_abs_diff']:.3e}), oracle fp32 - float64 = {e32:.3e}")
    for n in (N, N_BIG):
        sub = [a[:n] for a in args]
        out = model.infer_chunks(*sub, KCB)
        direct = _direct(lambda: model.infer_chunks(*sub, KCB))
        e, ed = float(np.abs(out - ref[:n]).max()), float(np.abs(direct - ref[:n]).max())
        print(f"L={L} n={n}: max|out - float64| = {e:.3e}, max|direct - float64| = {ed:.3e}, tol = {tol:.3e}")
        assert e <= tol, (L, n, e, tol)
        assert ed <= tol, (L, n, ed, tol)
        assert out.std(axis=0).min() > 1e-3, (L, n)


@pytest.mark.parametrize("L", LENGTHS)
def test_size_64_chunks_do_not_see_their_neighbours(L):
    """Chunks 1 ... 3 replaced by other chunks whose signal is scaled by 8 (a row leaking into a neighbour cannot hide): chunk 0
    and chunks 4 ... return the same bits, chunks 1 ... 3 change."""
    model, args, _, _ = _case(L, 64, False)
    for n in (N, N_BIG):
        out = model.infer_chunks(*[a[:n] for a in args], KCB)
        other = [a[:n].copy() for a in args]
        for i in range(1, 4):
            other[i][1:4] = args[i][N_BIG - 3 : N_BIG]
        other[0][1:4] = 8.0 * args[0][N_BIG - 3 : N_BIG]
        out_b = model.infer_chunks(*other, KCB)
        assert np.array_equal(_bits(out_b[0]), _bits(out[0])), (L, n, out[0], out_b[0])
        assert np.array_equal(_bits(out_b[4:]), _bits(out[4:])), (L, n, float(np.abs(out_b[4:] - out[4:]).max()))
        assert not np.array_equal(out_b[1:4], out[1:4]), (L, n)


@pytest.mark.parametrize("L", LENGTHS)
def test_size_64_chunks_return_the_same_bits_in_every_batch(L):
    model, args, _, _ = _case(L, 64, False)
    _assert_batch_independent(model, args, model.infer_chunks(*args, KCB), (L, 64))


@pytest.mark.parametrize("L", CLASS_LENGTHS)
@pytest.mark.parametrize("size", [32, 96, 176])
def test_other_sizes(size, L):
    """Size 32: the direct kernels of k_conv.hip; 96 and 176 (three output classes): the streamed convolutions of k_stream.hip.
    Amplified networks against float64, and the same bits in every batch."""
    model, args, ref, e32 = _case(L, size, True)
    tol = 1e-4 + 3.0 * e32
    big = None
    for n in (N, N_BIG):
        big = model.infer_chunks(*[a[:n] for a in args], KCB)
        e = float(np.abs(big - ref[:n]).max())
        print(f"size={size} L={L} n={n}: max|out - float64| = {e:.3e}, tol = {tol:.3e} (oracle fp32 - float64 = {e32:.3e})")
        assert e <= tol, (size, L, n, e, tol)
        assert big.std(axis=0).min() > 1e-3, (size, L, n)
    _assert_batch_independent(model, args, big, (L, size))


@pytest.mark.parametrize("L", [94, 107])
def test_other_chunk_lengths_are_refused_at_load(L):
    from remora_amd import RemoraError, synth
    from remora_amd.model_util import model_from_state

    state = synth.synth_state("conv_only", 64, 9, 2, seed=L, amplify=False)
    with pytest.raises(RemoraError, match="needs 3 final positions"):
        model_from_state(state, dict(chunk_context=(L // 2, L - L // 2), kmer_context_bases=KCB), device=0, dtype="fp32")
