"""GPU tests of the sequence fronts at every k-mer length class.

Only seq_conv1 depends on the k-mer length K = kb + ka + 1.  From chunk arrays launch_front (k_front.hip) runs it as
front_seq_kernel<5, false> (ConvLSTM), front_seq_tap_kernel<11, 9> (Conv_w_ref at K = 9) or front_seq_kernel<11, true>
(Conv_w_ref at any other K: the direct form); the dense entry `model(sigs, enc_kmers)` runs seq1_dense_kernel, generic in its
4 K input channels.  The kernels pack a window's bases three bits each into a 64-bit word: wider than 32 bits from K = 11,
full at K = 21; launch_front refuses K > 21 by name, the dense entry whatever does not fit the LDS.

Contexts: K = 1, 2 (both sides), 3, 6, 8, 10, 11, 13 and 21 (centred and both one-sided windows), on ConvLSTM_w_ref 64 and 128
and Conv_w_ref 64 and 96, fp32, amplified synthetic weights (every layer's error reaches the logits), chunk length 100,
max_seq_len 20.  Chunks 1 ... 6 of every batch are hand-made edges: no bases at all, the full max_seq_len, all bases N, an N at
each end of one window, zero-dwell bases, and a mapping that starts above 0 and ends below L (positions no base owns).  Chunk 0
stays an ordinary chunk: the reference's encoder takes the chunk length from its mapping row.

The reference is the oracle's torch.nn network in float64 on the oracle's encoding of the same chunk arrays; the bound is
1e-4 + 3 max|oracle fp32 - oracle float64| on the same chunks (test_large_models_on_long_chunk_contexts' allowance), 1e-4 for
dtype f16x3 (the gate test_split_bf16_logits_golden applies to the fp32-class split dtypes).  A test that cannot see the front
would pass whatever it computed: on the reference alone, changing one base in the middle of a chunk's own bases must move
the float64 logits of at least 95 % of the chunks by more than 1e-3, ten times the gate.

A second max_seq_len per (architecture, K in {3, 21}) runs front_seq_kernel with fewer chunks per block.  launch_front's plan
(plan_front_seq, rmr_plan.h) puts the gather table of kw K 320 bytes in front of eight private carves and halves the chunk
count while table + chunks exceed 78 KB.  A carve holds, each rounded up to 16 bytes, the mapping row (2 (msl + 1) bytes), the
sequence row (msl + K - 1), the window codes (8 msl), the base-of-position row (2 L) and, for ConvLSTM (kw = 5) only, the
per-base table U of 320 (msl + 1) bytes.  At L = 100:
    kw = 5,  K = 3:  table  4800 B, eight carves fit while a carve is <= 9384 B: msl 26 gives 9152, msl 27 gives 9488 -> 27
    kw = 5,  K = 21: table 33600 B, <= 5784 B: msl 15 gives 5536, msl 16 gives 5872 -> 16 (so max_seq_len 20 runs four already)
    kw = 11, K = 3:  table 10560 B, <= 8664 B: msl 766 gives 8656, msl 767 gives 8672 -> 767
    kw = 11, K = 21: table 73920 B, <=  744 B: msl 44 gives 736, msl 45 gives 752 -> 45
(tests/c/front_plans.cpp prints the same four numbers from rmr_plan.h; test_host_cpu.py pins them.)  Rows of 767 bases on 100
samples cannot come from synth_chunks: its chunks are widened with unused columns, and the full-length chunk is hand-made.

Plain bf16 / f16 are left out on purpose: their fused kernels are instantiated for K = 9 and 6, which the goldens cover, and
a bound for them needs the low-precision emulation envelope of test_gpu_fused.py, not a fixed number.

Measured on an MI355X (max |out - float64| over the twelve contexts and both batch sizes, chunk arrays / dense entry, against
tolerances of 1.01e-4 ... 1.04e-4):
    conv_lstm 64   4.6e-6 / 3.0e-6   (second max_seq_len: 2.7e-6)
    conv_lstm 128  3.0e-6 / 3.1e-6
    conv_only 64   4.3e-6 / 3.4e-6   (second max_seq_len: 2.3e-6)
    conv_only 96   7.7e-6 / 5.4e-6
    f16x3          5.5e-6 against 1e-4
    K = 22, dense  conv_lstm 9.8e-7, conv_only 2.3e-6; the load-time guard, probing through the dense entry, keeps Winograd
One changed base moves the float64 logits of 95.2 % ... 100 % of the chunks by more than 1e-3 (median 9e-3 ... 1.9e-1)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L = 100
MSL = 20
N, N_BIG, N_DENSE = 37, 1024 + 37, 64
KEYS = ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")
CONTEXTS = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (3, 4), (4, 5), (5, 5), (6, 6), (10, 10), (0, 20), (20, 0))
MODELS = (("conv_lstm", 64), ("conv_lstm", 128), ("conv_only", 64), ("conv_only", 96))
KW1 = {"conv_lstm": 5, "conv_only": 11}
# the first max_seq_len at which launch_front runs fewer than eight chunks per block (the docstring's derivation)
SECOND_MSL_CONTEXTS = ((1, 1), (10, 10))
NARROW_MSL = {(5, 3): 27, (5, 21): 16, (11, 3): 767, (11, 21): 45}
_cache = {}


def _up4(words):
    return (words + 3) & ~3


def _front_chunks_per_block(kw, K, msl):
    """plan_front_seq (rmr_plan.h) for front_seq_kernel<5, false> / <11, true>, in 4-byte words as there."""
    words = _up4(((msl + 1) * 2 + 3) // 4) + _up4((msl + K - 1 + 3) // 4) + _up4(msl * 2) + _up4((L * 2 + 3) // 4)
    if kw == 5:
        words += (msl + 1) * kw * 16
    cb = 8
    while cb > 1 and kw * K * 80 * 4 + cb * _up4(words) * 4 > 78 * 1024:
        cb >>= 1
    return cb


def _encode(kb, ka, seq, mp, ln):
    """One chunk's one-hot k-mers f32[4 K][L] in gather form: sample s belongs to the base p < ln with mp[p] <= s < mp[p + 1] and
    gets a 1 in row 4 kp + seq[p + kp] for every slot kp whose base is not N."""
    K = kb + ka + 1
    out = np.zeros((4 * K, L), np.float32)
    for s in range(L):
        owners = [p for p in range(ln) if mp[p] <= s < mp[p + 1]]
        assert len(owners) <= 1
        for p in owners:
            for kp in range(K):
                if seq[p + kp] >= 0:
                    out[4 * kp + seq[p + kp], s] = 1.0
    return out


def _chunks(kcb, msl=MSL):
    """(chunk arrays of N_BIG chunks with the edge chunks in rows 1 ... 6, the oracle's encoding as int8); computed once."""
    if (kcb, msl) not in _cache:
        from oracle import oracle as O
        from remora_amd import synth

        kb, ka = kcb
        K = kb + ka + 1
        base_msl = msl if msl <= 45 else MSL  # synth_chunks draws distinct cuts: at most L - 1 of them
        d = synth.synth_chunks(N_BIG, L, base_msl, kcb, 2, True, shard=100 * K + kb)
        sig, seqs, maps, lens = (d[k] for k in KEYS)
        if base_msl != msl:  # wider rows: unused columns behind every chunk's own
            seqs = np.concatenate([seqs, np.full((N_BIG, msl - base_msl), -1, np.int8)], axis=1)
            maps = np.concatenate([maps, np.zeros((N_BIG, msl - base_msl), np.int16)], axis=1)
        assert seqs.shape[1] == msl + K - 1 and maps.shape[1] == msl + 1
        rng = np.random.default_rng(K)
        # 1: no bases at all
        lens[1], maps[1], seqs[1] = 0, 0, -1
        # 2: the full max_seq_len (more bases than samples: most of them without a sample)
        lens[2], maps[2] = msl, np.floor(np.linspace(0, L, msl + 1)).astype(np.int16)
        seqs[2] = rng.integers(0, 4, seqs.shape[1])
        # 3: every base N
        seqs[3] = -1
        # 4: an N at each end of the window of the middle base
        p = int(lens[4]) // 2
        seqs[4, p] = seqs[4, p + K - 1] = -1
        # 5: bases 1 and 2 without a sample
        assert lens[5] >= 4
        maps[5, 2] = maps[5, 3] = maps[5, 1]
        # 6: eight bases on samples 7 ... 78: the samples before and behind belong to no base
        lens[6], maps[6] = 8, 0
        maps[6, :9] = 7 + 9 * np.arange(9)
        seqs[6] = -1
        seqs[6, : 8 + K - 1] = rng.integers(0, 4, 8 + K - 1)
        args = (sig, seqs, maps, lens)
        enc = O.compute_encoded_kmer_batch(kb, ka, *args[1:])
        assert enc.shape == (N_BIG, 4 * K, L)
        _cache[kcb, msl] = (args, enc.astype(np.int8))  # zeros and ones: kept small, widened where it is used
    return _cache[kcb, msl]


def _net(arch, size, K):
    if ("net", arch, size, K) not in _cache:
        from oracle import torch_ref
        from remora_amd import synth

        state = synth.synth_state(arch, size, K, 2, seed=K)
        _cache["net", arch, size, K] = (state, torch_ref.from_state(state))
    return _cache["net", arch, size, K]


def _forward(net, sig, enc, double):
    import torch

    with torch.no_grad():
        if double:
            out = net.double()(torch.from_numpy(sig).double(), torch.from_numpy(enc).double()).numpy()
            net.float()
            return out
        return net(torch.from_numpy(sig), torch.from_numpy(enc).float()).numpy()


def _refs(arch, size, kcb, msl=MSL):
    """(float64 logits of the N_BIG chunks, max |oracle fp32 - oracle float64|); computed once."""
    key = ("ref", arch, size, kcb, msl)
    if key not in _cache:
        args, enc = _chunks(kcb, msl)
        net = _net(arch, size, sum(kcb) + 1)[1]
        ref = _forward(net, args[0], enc, True)
        ref.setflags(write=False)
        _cache[key] = (ref, float(np.abs(_forward(net, args[0], enc, False) - ref).max()))
    return _cache[key]


def _model(arch, size, kcb, dtype="fp32"):
    """One model per (architecture, size, K, dtype): contexts of the same K share it."""
    K = sum(kcb) + 1
    key = ("model", arch, size, K, dtype)
    if key not in _cache:
        from remora_amd.model_util import model_from_state

        _cache[key] = model_from_state(_net(arch, size, K)[0], dict(chunk_context=(L // 2, L // 2), kmer_context_bases=kcb), device=0,
                                       dtype=dtype)
    return _cache[key]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _run_chunk_arrays(model, args, ref, tol, kcb, tag):
    """Batches of N and N_BIG chunks within tol of float64; the first 5 chunks alone return the bits they have in the batch.
    Returns the largest error."""
    worst, big = 0.0, None
    for n in (N, N_BIG):
        big = model.infer_chunks(*[a[:n] for a in args], kcb)
        e = float(np.abs(big - ref[:n]).max())
        print(f"{tag} n={n}: max|out - float64| = {e:.3e}, tol = {tol:.3e}")
        assert big.shape == ref[:n].shape and e <= tol, (tag, n, e, tol)
        worst = max(worst, e)
    five = model.infer_chunks(*[a[:5] for a in args], kcb)
    assert np.array_equal(_bits(five), _bits(big[:5])), (tag, float(np.abs(five - big[:5]).max()))
    return worst


@pytest.mark.parametrize("kcb", CONTEXTS + ((10, 11),))
def test_the_oracle_encodes_the_edge_chunks(kcb):
    """On the CPU: the oracle's encoding of chunks 0 ... 6 is the gather-form restatement's, and has the properties the edges are
    there for."""
    kb, ka = kcb
    K = kb + ka + 1
    for msl in [MSL] + ([NARROW_MSL[kw, K] for kw in (5, 11)] if kcb in SECOND_MSL_CONTEXTS else []):
        (sig, seqs, maps, lens), enc = _chunks(kcb, msl)
        for c in range(7):
            assert np.array_equal(enc[c], _encode(kb, ka, seqs[c], maps[c], int(lens[c]))), (kcb, msl, c)
        assert lens[0] > 0 and maps[0, lens[0]] == L
        assert not enc[1].any() and not enc[3].any()
        assert lens[2] == msl and maps[2, msl] == L
        owned = np.zeros(L, bool)
        for p in range(msl):
            owned[maps[2, p] : maps[2, p + 1]] = True
        assert owned.all() and np.array_equal(enc[2].sum(axis=0), np.full(L, K))  # every sample K ones
        p = int(lens[4]) // 2
        assert (enc[4][:, maps[4, p] : maps[4, p + 1]].sum(axis=0) == K - (2 if K > 1 else 1)).all() and maps[4, p + 1] > maps[4, p]
        assert maps[5, 1] == maps[5, 2] == maps[5, 3] < maps[5, 4]
        assert not enc[6][:, :7].any() and not enc[6][:, 79:].any() and (enc[6][:, 7:79].sum(axis=0) == K).all()


def test_the_second_max_seq_lens_are_the_first_with_fewer_chunks_per_block():
    for (kw, K), msl in NARROW_MSL.items():
        assert _front_chunks_per_block(kw, K, msl - 1) == 8 and _front_chunks_per_block(kw, K, msl) == 4, (kw, K, msl)
    assert _front_chunks_per_block(5, 21, MSL) == 4 and _front_chunks_per_block(11, 21, MSL) == 8
    assert all(_front_chunks_per_block(kw, sum(kcb) + 1, MSL) == 8 for kw in (5, 11) for kcb in CONTEXTS if sum(kcb) + 1 < 21)


@pytest.mark.parametrize("arch,size", MODELS)
@pytest.mark.parametrize("kcb", CONTEXTS)
def test_kmer_context(kcb, arch, size):
    """Chunk arrays and the dense entry against float64; the reference itself moves when one base changes."""
    tag = f"{arch} {size} kmer_context {kcb}"
    args, enc = _chunks(kcb)
    ref, e32 = _refs(arch, size, kcb)
    tol = 1e-4 + 3.0 * e32
    # the reference sees the front: one base changed in the middle of every chunk's own bases
    kb = kcb[0]
    seqs2 = args[1].copy()
    has = np.flatnonzero(args[3] > 0)
    col = kb + args[3][has].astype(np.int64) // 2
    old = seqs2[has, col]
    seqs2[has, col] = np.where(old >= 0, (old + 1) % 4, 0)
    from oracle import oracle as O

    ref2 = _forward(_net(arch, size, sum(kcb) + 1)[1], args[0], O.compute_encoded_kmer_batch(*kcb, seqs2, args[2], args[3]), True)
    moved = np.abs(ref2 - ref).max(axis=1)[has]
    print(f"{tag}: one changed base moves the float64 logits by min {moved.min():.3e}, median {np.median(moved):.3e}; "
          f"{(moved > 1e-3).mean():.4f} of {has.size} chunks by more than 1e-3; oracle fp32 - float64 = {e32:.3e}")
    assert has.size == N_BIG - 1 and (moved > 1e-3).mean() >= 0.95, (tag, float((moved > 1e-3).mean()))

    model = _model(arch, size, kcb)
    _run_chunk_arrays(model, args, ref, tol, kcb, tag)
    dense = np.asarray(model(args[0][:N_DENSE], enc[:N_DENSE].astype(np.float32)).cpu())
    ed = float(np.abs(dense - ref[:N_DENSE]).max())
    print(f"{tag} dense n={N_DENSE}: max|out - float64| = {ed:.3e}, tol = {tol:.3e}")
    assert dense.shape == (N_DENSE, 2) and ed <= tol, (tag, ed, tol)


@pytest.mark.parametrize("arch", ["conv_lstm", "conv_only"])
@pytest.mark.parametrize("kcb", SECOND_MSL_CONTEXTS)
def test_fewer_chunks_per_block(kcb, arch):
    """Size 64 at the first max_seq_len whose rows leave room for four chunks per block instead of eight."""
    K = sum(kcb) + 1
    msl = NARROW_MSL[KW1[arch], K]
    args, _ = _chunks(kcb, msl)
    assert args[1].shape[1] == msl + K - 1 and args[2].shape[1] == msl + 1
    ref, e32 = _refs(arch, 64, kcb, msl)
    _run_chunk_arrays(_model(arch, 64, kcb), args, ref, 1e-4 + 3.0 * e32, kcb, f"{arch} 64 kmer_context {kcb} max_seq_len {msl}")


@pytest.mark.parametrize("kcb", [(0, 0), (5, 5), (10, 10)])
def test_split_dtype_f16x3(kcb):
    """The same launch_front, then the split convolutions (launch_conv_split): the dtype's stated gate against float64."""
    args, _ = _chunks(kcb)
    ref, _ = _refs("conv_lstm", 64, kcb)
    _run_chunk_arrays(_model("conv_lstm", 64, kcb, "f16x3"), args, ref, 1e-4, kcb, f"f16x3 conv_lstm 64 kmer_context {kcb}")


@pytest.mark.parametrize("arch", ["conv_lstm", "conv_only"])
def test_kmer_length_22_loads_and_runs_through_the_dense_entry_only(arch):
    """K = 22 no longer fits a 64-bit word of 3-bit codes: the model loads, the chunk-array entry refuses it by name before any
    launch, the dense entry computes it."""
    from remora_amd import RemoraError

    kcb = (10, 11)
    args, enc = _chunks(kcb)
    ref, e32 = _refs(arch, 64, kcb)
    tol = 1e-4 + 3.0 * e32
    model = _model(arch, 64, kcb)
    assert model.kmer_len == 22 and model.numerics["checked"] == 1, model.numerics  # the guard probed it through the dense entry
    with pytest.raises(RemoraError, match="kmer_len 22 > 21"):
        model.infer_chunks(*[a[:N] for a in args], kcb)
    enc64 = enc[:N_DENSE].astype(np.float32)
    dense = np.asarray(model(args[0][:N_DENSE], enc64).cpu())
    ed = float(np.abs(dense - ref[:N_DENSE]).max())
    print(f"{arch} 64 K=22 dense n={N_DENSE}: max|out - float64| = {ed:.3e}, tol = {tol:.3e}; guard {model.winograd_form}")
    assert ed <= tol, (arch, ed, tol)
    assert np.array_equal(_bits(np.asarray(model(args[0][:N_DENSE], enc64).cpu())), _bits(dense))  # the refusal left no trace


def test_kmer_length_64_loads_and_the_dense_entry_refuses_what_does_not_fit_the_lds():
    """ConvLSTM at K = 64 (the largest desc_ok admits), L = 100: weights [5][256][16] and one chunk's tensor [256][100] are 184320
    bytes, more than a CU's 160 KB of LDS."""
    from remora_amd import RemoraError, synth
    from remora_amd.model_util import model_from_state

    state = synth.synth_state("conv_lstm", 64, 64, 2, seed=64)
    model = model_from_state(state, dict(chunk_context=(L // 2, L // 2), kmer_context_bases=(31, 32)), device=0, dtype="fp32")
    assert model.kmer_len == 64 and model.numerics["checked"] == 0, model.numerics  # no entry runs it: nothing to screen
    rng = np.random.default_rng(64)
    sig = rng.standard_normal((3, 1, L)).astype(np.float32)
    with pytest.raises(RemoraError, match=r"dense seq_conv1 needs \d+ B LDS"):
        model(sig, np.zeros((3, 256, L), np.float32))
