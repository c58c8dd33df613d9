"""GPU tests of the unfused 16-bit pipeline (conv_bf16s_kernel + lstm_x16s_kernel / lstm_bf16s_kernel) at the shapes its other
tests never reach: padded size 32, plain bf16 off the fused kernels, the dense one-hot entry, ragged batches around the
convolutions' chunks-per-iteration (cb) and the LSTM's sixteen-chunk groups, one to three and more than 120 LSTM steps, cb of 1,
2 and 3, and the second trip of a persistent block.  It serves dtypes bf16x6, bf16x3 and f16x3 everywhere and plain bf16 wherever
the fused front kernel does not run (size 32, a dense one-hot input, a chunk length that is no multiple of 4).

Reference: oracle.torch_ref in float64; plain bf16 also against oracle.lowp_emulation at this pipeline's rounding sites.  Gates:
tests/test_gpu_lstm_heads.py (GATE, assert_bf16_statistics), whose helpers are used here.  Every test prints what it measured."""
import numpy as np
import pytest

from stream_cases import layer_rows
from test_gpu_lstm_heads import (GATE, KCB, assert_bf16_statistics, assert_gate, bf16_emulated_errors, bits, chunk_case, float64_logits,
                                 infer, make_model)

pytestmark = pytest.mark.gpu

NPARTS = {"bf16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 2}  # 16-bit parts per operand
SPLIT_DTYPES = ("bf16x6", "bf16x3", "f16x3")
# (first chunk, chunks): a chunk beside other neighbours and in other block iterations than in the full batch - around cb = 4 | 8
# chunks per convolution iteration and the LSTM's groups of sixteen
SUB_BATCHES = ((0, 1), (5, 3), (7, 15), (100, 16), (300, 17), (700, 257))
_cases = {}


def conv_split_plan(ic, pin, nparts):
    """plan_conv_split's arithmetic (rmr_plan.h, for k_conv_bf16s.hip): (chunks per block iteration, LDS bytes) of a split
    convolution of `ic` input channels whose chunks have `pin` input rows.  tests/test_host_stream_cases.py holds it to the header."""
    pair = ic == 16                      # two taps per k-step, two planes
    ks = 1 if pair else ic // 32
    slr = ks + 1 if ks % 2 == 0 else ks  # odd row stride in 16-byte slots
    planes = 2 if pair else 4
    cb = max(1, min(8, (112 * 1024) // (pin * slr * 16 * planes * nparts)))
    if cb >= 4:
        cb &= ~3
    plane = ((cb * pin + 2) * slr + 15) & ~15
    return cb, (planes * plane + 16) * nparts * 16


def kernels_of(model, fn):
    """(fn(), names of the kernels the model's engine launched meanwhile)."""
    eng = model.engine
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        out = fn()
        return out, set(eng.profile())
    finally:
        eng.profile_enable(False)


def _case(size, L, n, msl, num_out, cg, shard):
    """state, chunk arrays, one-hot tensor and float64 logits of one (network, batch); computed once, read-only."""
    key = (size, L, n, msl, num_out, cg, shard)
    if key not in _cases:
        from remora_amd import synth

        state = synth.synth_state("conv_lstm", size, 9, num_out, seed=7 * size + num_out)
        args, enc = chunk_case(L, n, msl, num_out, cg, shard)
        ref = float64_logits(state, args[0], enc)
        assert ref.std(axis=0).min() >= 1e-2  # the chunks are told apart by a hundred fp32 gates or more
        _cases[key] = dict(state=state, args=args, enc=enc, ref=ref, emus=None)
    return _cases[key]


def check(c, out, dtype, ctx, rows=slice(None)):
    """`out` (logits of chunks `rows` of case c) against the dtype's gate."""
    if dtype != "bf16":
        return assert_gate(out, c["ref"][rows], dtype, ctx)
    if c["emus"] is None:
        c["emus"] = bf16_emulated_errors(c["state"], c["args"][0], c["enc"], c["ref"])
    assert_bf16_statistics(out, c["ref"][rows], [e[rows] for e in c["emus"]], ctx)
    return float(np.abs(out - c["ref"][rows]).max())


def dense_inputs(c, rows):
    import torch

    return torch.tensor(c["args"][0][rows]).cuda(), torch.tensor(c["enc"][rows]).cuda()


# ---- B: padded size 32 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C100", "C200"])
@pytest.mark.parametrize("dtype", ["bf16", "bf16x3", "bf16x6", "f16x3"])
@pytest.mark.parametrize("size", [32, 24])
def test_padded_size_32(size, dtype, cfg):
    """lstm_bf16s_kernel<32, 1 | 2 | 3, false>, <32, 2, true> and conv_bf16s_kernel<64, 5, 1, ...> in all four part formats: 32
    channels, and 24 run at 32 with zero-weight channels, C100 with two classes and C200 with three.  1500 chunks against
    float64 (bf16: also against the emulation); sub-batches return the bits of the 1500-chunk call - a row leaking between the
    chunks of a staged image would show; the dense one-hot entry meets the same gate on 64 chunks."""
    from remora_amd import synth

    cc, _, msl, num_out, cg = synth.CONFIGS[cfg]
    c = _case(size, sum(cc), 1500, msl, num_out, cg, 11)
    model = make_model(c["state"], cc, dtype)
    assert model.size == size and model.kernel_size == 32
    ctx = f"size {size} {cfg} {dtype}"
    out, kernels = kernels_of(model, lambda: infer(model, c["args"]))
    assert {"conv_sig3", "conv_seq2", "conv_merge1", "lstm_head"} <= kernels and "fused_front" not in kernels, kernels
    check(c, out, dtype, ctx + " n 1500")
    for start, m in SUB_BATCHES:
        part = infer(model, c["args"], start, m)
        assert np.array_equal(bits(part), bits(out[start : start + m])), (ctx, start, m, float(np.abs(part - out[start : start + m]).max()))
    dense = model(*dense_inputs(c, slice(0, 64))).cpu().numpy()
    check(c, dense, dtype, ctx + " dense n 64", slice(0, 64))
    if dtype != "bf16":  # seq_conv1 is summed in another order from a one-hot tensor: the last bits of seq1 differ, no more
        assert np.abs(dense - out[:64]).max() <= GATE[dtype], (ctx, float(np.abs(dense - out[:64]).max()))


# ---- C: size 64 off the fused path ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "bf16x3", "bf16x6", "f16x3"])
def test_size_64_dense_entry(dtype):
    """model(sig, enc) on 257 chunks: launch_seq1_dense, then the split convolutions and lstm_x16s_kernel - for plain bf16
    conv_bf16s_kernel<.., 1> and lstm_bf16s_kernel<64, 1>, which chunk arrays never reach at this size.  Against float64 / the
    emulation; slices of the batch return the same bits."""
    c = _case(64, 100, 257, 20, 2, True, 13)
    model = make_model(c["state"], (50, 50), dtype)
    ctx = f"size 64 dense {dtype}"
    out, kernels = kernels_of(model, lambda: model(*dense_inputs(c, slice(None))).cpu().numpy())
    assert {"seq_conv1_dense", "conv_sig3", "conv_seq2", "conv_merge1", "lstm_head"} <= kernels and "fused_front" not in kernels, kernels
    check(c, out, dtype, ctx + " n 257")
    for start, m in ((0, 1), (5, 3), (7, 15), (100, 16), (200, 17), (3, 254)):
        part = model(*dense_inputs(c, slice(start, start + m))).cpu().numpy()
        assert np.array_equal(bits(part), bits(out[start : start + m])), (ctx, start, m, float(np.abs(part - out[start : start + m]).max()))
    if dtype != "bf16":  # (plain bf16 takes the fused kernels from chunk arrays: other rounding sites)
        arrays = infer(model, c["args"])
        assert np.abs(arrays - out).max() <= GATE[dtype], (ctx, float(np.abs(arrays - out).max()))


def test_size_64_bf16_chunk_length_no_multiple_of_four():
    """chunk_context (49, 49): L = 98 is no multiple of 4, the fused front kernel does not take it - plain bf16 runs the unfused
    pipeline from chunk arrays (24 LSTM steps), f16 keeps refusing."""
    from remora_amd import RemoraError

    cc = (49, 49)
    assert layer_rows(98) == (94, 90, 28, 24)
    c = _case(64, 98, 1500, 20, 2, True, 17)
    model = make_model(c["state"], cc, "bf16")
    out, kernels = kernels_of(model, lambda: infer(model, c["args"]))
    assert {"conv_sig3", "conv_seq2", "conv_merge1", "lstm_head"} <= kernels and "fused_front" not in kernels, kernels
    check(c, out, "bf16", "size 64 L 98 bf16 n 1500")
    for start, m in SUB_BATCHES:
        part = infer(model, c["args"], start, m)
        assert np.array_equal(bits(part), bits(out[start : start + m])), (start, m, float(np.abs(part - out[start : start + m]).max()))
    half = make_model(c["state"], cc, "f16")
    with pytest.raises(RemoraError, match="fused kernels only"):
        infer(half, c["args"], 0, 8)


# ---- D: step counts and long chunks ---------------------------------------------------------------------------------------------
# (200, 200): the reference's default chunk_context.  cb of (sig_conv3, seq_conv2, merge_conv1) by conv_split_plan, keyed by
# (size, parts): 112 KB / (392 rows x 32 B x parts) = 3 (three parts) or 4 (two); 112 KB / (396 x 32 x parts) likewise;
# merge_conv1: 128 rows x 320 B x parts at size 64 (120 KB | 80 KB: one chunk), 128 x 192 x parts at size 32 (72 KB: one chunk;
# 48 KB: two)
LONG_CB = {(64, 3): (3, 3, 1), (64, 2): (4, 4, 1), (32, 3): (3, 3, 1), (32, 2): (4, 4, 2)}


@pytest.mark.parametrize("cc,T,msl", [((14, 15), 1, 7), ((16, 16), 2, 8), ((17, 18), 3, 8), ((200, 200), 124, 80)])
@pytest.mark.parametrize("dtype", SPLIT_DTYPES)
@pytest.mark.parametrize("size", [64, 32])
def test_split_step_counts_and_long_chunks(size, dtype, cc, T, msl):
    """lstm_x16s_kernel (size 64) and lstm_bf16s_kernel (size 32) at one, two and three steps - the second x tile is x_0 again at
    T = 1 (`a.T > 1 ? 1 : 0`), every x_{t+2} fetch is a clamped re-read, step 0 reads no h and hs[(t - 1) & 1] first at t = 1 -
    and at 124 steps on the reference's default chunks of 400 samples, where the split convolutions stage 1, 2, 3 or 4 chunks
    per iteration (LONG_CB) in images whose plane and part strides are not C100's or C200's.  Batches of 5 and 37 chunks against
    float64, the same bits in both."""
    L = sum(cc)
    P1, P2, P3, steps = layer_rows(L)
    assert steps == T
    if L == 400:
        assert T > 120
        np_ = NPARTS[dtype]
        plans = (conv_split_plan(16, P2, np_), conv_split_plan(16, P1, np_), conv_split_plan(2 * size, P3, np_))
        assert tuple(p[0] for p in plans) == LONG_CB[(size, np_)] and all(p[1] <= 160 * 1024 for p in plans), plans
    c = _case(size, L, 37, msl, 2, True, L)
    model = make_model(c["state"], cc, dtype)
    ctx = f"size {size} cc {cc} T {T} {dtype}"
    out = infer(model, c["args"])
    check(c, out, dtype, ctx + " n 37")
    few = infer(model, c["args"], 0, 5)
    check(c, few, dtype, ctx + " n 5", slice(0, 5))
    assert np.array_equal(bits(few), bits(out[:5])), (ctx, float(np.abs(few - out[:5]).max()))


def test_split_convolution_too_long_for_the_lds_is_refused_by_name():
    """bf16x6 at chunk_context (300, 300), size 64: merge_conv1 stages 195 rows of 128 channels in three parts - one chunk needs
    (4 planes x 992 slots + 16) x 3 x 16 B = 191 232 B, more than the 160 KB of a block: refused on the host before the launch,
    with the layer's name; the engine then returns for a C100 model the bits it returned before."""
    from remora_amd import RemoraError, synth

    assert layer_rows(600)[2] == 195 and conv_split_plan(128, 195, 3) == (1, 191232)
    short = _case(64, 100, 257, 20, 2, True, 13)
    model = make_model(short["state"], (50, 50), "bf16x6")
    before = infer(model, short["args"])
    check(short, before, "bf16x6", "size 64 C100 bf16x6 n 257")
    d = synth.synth_chunks(5, 600, 80, KCB, 2, True, shard=600)
    long_model = make_model(short["state"], (300, 300), "bf16x6")
    with pytest.raises(RemoraError, match=r"conv_merge1 needs 191232 B of LDS"):
        long_model.infer_chunks(d["signal"], d["sequence"], d["sequence_to_signal_mapping"], d["sequence_lengths"], KCB)
    after = infer(model, short["args"])
    assert np.array_equal(bits(after), bits(before))


# ---- E: the second trip of a persistent block -----------------------------------------------------------------------------------
@pytest.mark.parametrize("size,dtype", [(64, "bf16x6"), (64, "bf16x3"), (64, "f16x3"), (32, "bf16x6"), (32, "bf16")])
def test_second_trip_of_a_persistent_block(size, dtype):
    """lstm_x16s_kernel launches 8 x CUs blocks of sixteen chunks, lstm_bf16s_kernel and the split convolutions 2 x CUs: with
    16 x blocks + 37 chunks the first three blocks start a second group - xs staged again, c reset, hs / part reused - and the
    convolutions (8 chunks an iteration, 2 x CUs blocks) run three or more iterations per block.  The first 64, the last 53 (the
    last first-trip group and the three second-trip ones) and 2048 chunks drawn from the batch return the same bits as a batch
    of their own; the 2048 meet the gate against float64; two calls on the full batch agree and are finite."""
    import torch

    from remora_amd import synth

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (8 if size == 64 else 2) * cus * 16 + 37
    d = synth.synth_chunks(n, 100, 20, KCB, 2, True, shard=size)
    keys = ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")
    args = tuple(d[k] for k in keys)
    pick = np.sort(np.random.default_rng(5).choice(n, 2048, replace=False))
    state = synth.synth_state("conv_lstm", size, 9, 2, seed=7 * size + 2)
    model = make_model(state, (50, 50), dtype)
    ctx = f"size {size} {dtype} n {n} ({cus} CUs)"
    full, kernels = kernels_of(model, lambda: infer(model, args))
    assert "fused_front" not in kernels and "conv_merge1" in kernels, kernels
    assert np.isfinite(full).all() and np.array_equal(bits(full), bits(infer(model, args))), ctx
    for name, rows in (("first 64", np.arange(64)), ("last 53", np.arange(n - 53, n)), ("2048 drawn", pick)):
        own = model.infer_chunks(*[np.ascontiguousarray(a[rows]) for a in args], KCB)
        assert np.array_equal(bits(own), bits(full[rows])), (ctx, name, float(np.abs(own - full[rows]).max()))
    from oracle import oracle as O

    sub = tuple(np.ascontiguousarray(a[pick]) for a in args)
    c = dict(state=state, args=sub, enc=O.compute_encoded_kmer_batch(*KCB, *sub[1:]), emus=None)
    c["ref"] = float64_logits(state, sub[0], c["enc"])
    check(c, full[pick], dtype, ctx + ", 2048 drawn")
