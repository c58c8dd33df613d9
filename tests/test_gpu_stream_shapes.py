"""GPU tests of the streamed-weight kernels (networks of more than 64 channels) at every width, LSTM step count and position window.

k_stream.hip (fp32: conv_stream_kernel<9,3>, <13,3>, <5,1>, lstm_stream_kernel<4,512> and <2,1024>) and k_stream16.hip (bf16 / f16:
conv_stream16_kernel, lstm_stream16_kernel) choose on the host how a launch runs: waves per block, chunks per block iteration (cb),
position windows, column tiles per work item, chunks per LSTM group.  tests/stream_cases.py holds the cases and restates that
arithmetic; tests/test_host_stream_cases.py asserts without a GPU that every case takes the path it is named for, and that the
fp32 gate sees one wrong 16-channel tile at one position through the LSTM of the long cases.  Here the cases run.

ConvLSTM_w_ref, three classes, k-mer context (4, 4), synth.synth_state(..., amplify=True) weights, synth.synth_chunks inputs.  The
reference is oracle.torch_ref in float64 on oracle.compute_encoded_kmer_batch's one-hot tensor.

fp32: max |logit - float64| <= GATE["fp32"] = 1e-4 (the project's gate), every run into a NaN-filled buffer, conv_merge1 and
lstm_head in the engine's profile; torch's own fp32 forward on the same inputs is printed beside every figure.  Sub-batches return
the bits of the full batch and a second run the bits of the first (k-ordered fmaf chains: an equality, not a tolerance).

bf16 / f16: rounding noise (1e-2 / 1e-3) would hide one wrong column inside an absolute gate, so three checks together: the error
statistics of the whole batch inside the envelope of oracle.lowp_emulation's four draws at this pipeline's rounding sites
(assert_bf16_statistics' margins, unchanged), every chunk's bits equal across groupings that put it first in an LSTM group, last
in one and in a ragged tail and across the convolutions' cb values, and no logit left unwritten.

Measured on an MI355X (256 CUs), max over the cases and batch sizes of a group; torch's own fp32 forward on the same chunks beside it:
    fp32  every width (12 sizes, 37 and 65 | 33 chunks)      max|out - float64| 1.95e-6    torch fp32 8.8e-7
          T = 1, 2, 3 (5 sizes, 37 and 1061 chunks)                             1.45e-6                5.1e-7
          window switch (6 cases of 5 chunks)                                   1.36e-6                1.09e-6
          (256, 233) with 260 chunks                                            9.5e-6                 1.4e-6
          window remainders (L 266, 269)                                        9.0e-7                 9.0e-7
          second LSTM trip (65 573 and 32 805 chunks, every chunk)              1.42e-6                6.5e-7
    every sub-batch and second run of test_sub_batches_and_second_runs_return_the_same_bits: equal bits.
    16-bit |out - float64|, kernel mean / q99 against the emulation's four draws (mean range; q99 range):
          size 192 L 100   bf16 1.48e-3 / 5.2e-3  (0.90..1.74e-3; 3.2..6.5e-3)    f16 1.76e-4 / 7.6e-4  (1.46..2.32e-4; 5.0..9.4e-4)
          size 224 L 100   bf16 1.31e-3 / 4.6e-3  (1.45..1.74e-3; 5.2..6.3e-3)    f16 1.79e-4 / 6.6e-4  (1.98..2.29e-4; 7.0..8.5e-4)
          size  96 T 1..3  bf16 5.6..9.4e-4 / 1.8..2.9e-3 (5.8e-4..1.23e-3; 1.9..3.8e-3)
                           f16 0.72..1.09e-4 / 2.4..3.6e-4 (0.74..1.50e-4; 2.4..4.7e-4)
          size 256 T 1..3  bf16 7.0..9.5e-4 / 2.3..3.1e-3 (6.6e-4..1.26e-3; 2.2..4.0e-3)
                           f16 0.86..1.26e-4 / 2.9..4.6e-4 (0.85..1.57e-4; 2.8..5.2e-4)
          size  96 L 100, 2085 chunks (cb 8)   bf16 1.40e-3 / 5.2e-3 (0.94..2.59e-3; 3.0..8.4e-3)   f16 2.54e-4 / 9.3e-4 (1.64..2.66e-4; 5.4e-4..1.07e-3)
          size 256 L 464, 64 chunks (bf16)     3.4e-3 / 2.5e-2 (2.7..5.1e-3; 1.5..3.8e-2)
    every grouping of check 2 returned the bits of the full batch."""
import numpy as np
import pytest

from stream_cases import CASES16, DTYPES16, FP32_CASES, LDS_EDGE16, SUB_BATCHES, conv16_plan, conv_layers, layer_rows, lstm_stream_plan, weights_seed
from test_gpu_lstm_heads import (GATE, KCB, KEYS, assert_bf16_statistics, assert_gate, bf16_emulated_errors, bits, chunk_case, float64_logits,
                                 frozen, infer, infer_into_nan, make_model)
from test_gpu_split_shapes import kernels_of

pytestmark = pytest.mark.gpu

NUM_OUT = 3
_cases, _cases16, _trips = {}, {}, {}


def chunk_context(L):
    return (L // 2, L - L // 2)


def fp32_error(state, sig, enc, exact):
    """max |torch fp32 forward - float64| of the oracle's network on the same inputs: what fp32 costs a plain implementation."""
    import torch

    from oracle import torch_ref

    with torch.no_grad():
        return float(np.abs(torch_ref.from_state(state)(torch.tensor(sig), torch.tensor(enc)).numpy() - exact).max())


def _case(size, L, n):
    """state, chunk arrays (host and device), float64 logits and torch fp32's error of n chunks; computed once, read-only."""
    if (size, L, n) not in _cases:
        import torch

        from remora_amd import synth

        state = synth.synth_state("conv_lstm", size, 9, NUM_OUT, seed=weights_seed(size), amplify=True)
        args, enc = chunk_case(L, n, min(20, L // 4), NUM_OUT, True, shard=L)
        ref = float64_logits(state, args[0], enc)
        assert ref.std(axis=0).min() >= 1e-2  # the chunks are told apart in every class, by a hundred gates or more
        _cases[(size, L, n)] = dict(state=state, args=args, dev=tuple(torch.tensor(a).cuda() for a in args), ref=ref,
                                    torch32=fp32_error(state, args[0], enc, ref))
    return _cases[(size, L, n)]


def run_into_nan(model, dev, n, ctx):
    """Logits of the first n chunks, written into a NaN-filled device buffer by the streamed kernels (asserted from the profile)."""
    out, kernels = kernels_of(model, lambda: infer_into_nan(model, dev, n))
    assert {"conv_sig3", "conv_seq2", "conv_merge1", "lstm_head"} <= kernels and "fused_front" not in kernels, (ctx, kernels)
    unwritten = np.argwhere(np.isnan(out))
    assert unwritten.size == 0, (ctx, f"{len(unwritten)} logits left unwritten, first (chunk, class): {unwritten[:4].tolist()}")
    return out


def check_fp32(case):
    c = _case(case.size, case.L, max(case.batches))
    model = make_model(c["state"], chunk_context(case.L), "fp32")
    assert model.kernel_size == case.size and model.num_out == NUM_OUT
    for n in case.batches:
        ctx = f"{case.group} size {case.size} L {case.L} T {layer_rows(case.L)[3]} n {n}"
        out = run_into_nan(model, c["dev"], n, ctx)
        print(f"{ctx}: torch fp32 max|out - float64| = {c['torch32']:.3e} (on {max(case.batches)} chunks)")
        assert_gate(out, c["ref"][:n], "fp32", ctx)


def _ids(c):
    return f"{c.size}-{c.L}-{c.batches[-1]}"


def group(name):
    return [c for c in FP32_CASES if c.group == name]


# ---- a: every width ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", group("widths"), ids=_ids)
def test_every_width(case):
    """Sizes 80, 96 ... 256 at L = 100: five, six, seven and eight waves per convolution block (an uneven share of 9, 11 and 13
    output tiles at 144, 176 and 208), lstm_stream_kernel<4, 512> up to 128 units and <2, 1024> above, on 320 ... 1024 threads.
    Batches of 37 chunks (a ragged last LSTM group) and of one full group and one chunk (65 or 33)."""
    assert case.batches == (37, 16 * lstm_stream_plan(case.size).nt + 1)
    check_fp32(case)


# ---- b: step counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", group("steps"), ids=_ids)
def test_one_two_and_three_lstm_steps(case):
    """L = 29, 32, 35: T = 1, 2, 3.  lstm_stream_kernel at T = 1 runs no recurrent product, its x_{t+1} fetch is a clamped re-read
    and lstm2 reads h from image (T - 1) & 1 = 0; merge_conv1 stages cb = 4 .. 8 chunks whose T columns each share ONE column
    tile; sig_conv3 / seq_conv2 run 2, 3 and 4 tiles per work item.  37 chunks and 1024 + 37."""
    check_fp32(case)


# ---- c, d: the window switch and the window remainders ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", group("window"), ids=_ids)
def test_both_sides_of_the_window_switch(case):
    """merge_conv1 just below the switch - one chunk per block in the largest LDS image the kernel ever takes (152 640 B at sizes 256
    and 224, 153 664 B at 128) - and just above it, in windows of 16 (48 at size 128) columns whose last one is partial; 260
    chunks of (256, 233) are 1300 window iterations: 276 of an MI355X's 1024 blocks take a second one and restage after the barrier."""
    import torch

    if case.batches == (260,):
        assert 260 * 5 > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    check_fp32(case)


@pytest.mark.parametrize("case", group("remainder"), ids=_ids)
def test_window_remainders(case):
    """Size 256: 80 columns are five full windows (the last one of exactly pout_w columns), 81 a sixth window of ONE column, which
    stages rows == KW."""
    check_fp32(case)


# ---- e: the second trip of a persistent LSTM block --------------------------------------------------------------------------------
def _trip_case(case):
    """The batch of a "trips" case, its float64 logits (computed in slices of 8192 chunks: the one-hot tensor stays small) and the
    kernels' logits of the whole batch; computed once."""
    if case not in _trips:
        import torch

        from oracle import oracle as O
        from remora_amd import synth

        n = case.batches[0]
        d = synth.synth_chunks(n, case.L, min(20, case.L // 4), KCB, NUM_OUT, True, shard=case.L + case.size)
        args = tuple(frozen(d[k]) for k in KEYS)
        state = synth.synth_state("conv_lstm", case.size, 9, NUM_OUT, seed=weights_seed(case.size), amplify=True)
        ref, torch32 = np.empty((n, NUM_OUT)), 0.0
        for s in range(0, n, 8192):
            part = tuple(a[s : s + 8192] for a in args)
            enc = O.compute_encoded_kmer_batch(*KCB, *part[1:])
            ref[s : s + 8192] = float64_logits(state, part[0], enc)
            torch32 = max(torch32, fp32_error(state, part[0], enc, ref[s : s + 8192]))
        model = make_model(state, chunk_context(case.L), "fp32")
        ctx = f"trips size {case.size} L {case.L} n {n}"
        out = run_into_nan(model, tuple(torch.tensor(a).cuda() for a in args), n, ctx)
        _trips[case] = dict(state=state, args=args, ref=frozen(ref), torch32=torch32, model=model, out=frozen(out), ctx=ctx)
    return _trips[case]


@pytest.mark.parametrize("case", group("trips"), ids=_ids)
def test_second_trip_of_a_persistent_lstm_block(case):
    """lstm_stream_kernel launches 4 x CUs blocks of 16 NT chunks: with 65 536 + 37 chunks at NT = 4 (size 80) and 32 768 + 37 at
    NT = 2 (size 144) the first blocks start a second group - x staged again, c reset, the fc partial sums over what was h.  Every
    chunk of the batch against float64."""
    import torch

    c = _trip_case(case)
    nt = lstm_stream_plan(case.size).nt
    assert -(-case.batches[0] // (16 * nt)) > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    print(f"{c['ctx']}: torch fp32 max|out - float64| = {c['torch32']:.3e}")
    assert_gate(c["out"], c["ref"], "fp32", c["ctx"])


# ---- f: position independence -----------------------------------------------------------------------------------------------------
def test_sub_batches_and_second_runs_return_the_same_bits():
    """One case each of the step counts (size 208, T = 3, 1061 chunks), the windows (size 256, L = 233, 260 chunks) and the second
    trip (size 80, 65 573 chunks): the chunks of a sub-batch - alone, beside other neighbours in a block iteration, in another
    LSTM group and tile - return the bits they have in the full batch, and a second run of the full batch the bits of the first."""
    picks = ([c for c in group("steps") if (c.size, c.L) == (208, 35)] + [c for c in group("window") if c.batches == (260,)] +
             [c for c in group("trips") if c.size == 80])
    assert len(picks) == 3
    for case in picks:
        n = case.batches[-1]
        if case.group == "trips":
            t = _trip_case(case)
            model, args, full = t["model"], t["args"], t["out"]
        else:
            c = _case(case.size, case.L, n)
            model, args = make_model(c["state"], chunk_context(case.L), "fp32"), c["args"]
            full = infer(model, args)
            assert_gate(full, c["ref"], "fp32", f"{case.group} size {case.size} L {case.L} n {n} (host arrays)")
        ctx = f"{case.group} size {case.size} L {case.L} n {n}"
        assert np.array_equal(bits(infer(model, args)), bits(full)), (ctx, "second run")
        ran = 0
        for start, m in SUB_BATCHES:
            if start + m > n:
                continue
            part = infer(model, args, start, m)
            assert np.array_equal(bits(part), bits(full[start : start + m])), (ctx, start, m, float(np.abs(part - full[start : start + m]).max()))
            ran += 1
        assert ran >= 4, ctx
        print(f"{ctx}: {ran} sub-batches and a second run return the same bits")


# ---- bf16 / f16 -------------------------------------------------------------------------------------------------------------------
def _case16(size, L, n):
    if (size, L, n) not in _cases16:
        import torch

        from remora_amd import synth

        state = synth.synth_state("conv_lstm", size, 9, NUM_OUT, seed=weights_seed(size), amplify=True)
        args, enc = chunk_case(L, n, min(20, L // 4), NUM_OUT, True, shard=L + 1)
        _cases16[(size, L, n)] = dict(state=state, args=args, enc=enc, dev=tuple(torch.tensor(a).cuda() for a in args),
                                      ref=float64_logits(state, args[0], enc), emus={})
    return _cases16[(size, L, n)]


def check_statistics(c, model, dtype, n, ctx):
    """Checks 1 and 3: the first n chunks into a NaN-filled buffer, their error within the envelope of the emulation's draws."""
    if dtype not in c["emus"]:
        c["emus"][dtype] = bf16_emulated_errors(c["state"], c["args"][0], c["enc"], c["ref"], fmt=dtype)
    out = run_into_nan(model, c["dev"], n, ctx)
    assert_bf16_statistics(out, c["ref"][:n], [e[:n] for e in c["emus"][dtype]], f"{ctx} {dtype}")
    return out


def check_groupings(model, args, out, size, n, ctx, pivot=200):
    """Check 2: chunk `pivot` first in an LSTM group of 16 NT chunks, last in one and in a ragged tail of three, a chunk alone, and
    (where the batch holds them) 600 chunks from chunk 300 - on a GPU of 256 CUs the convolutions take those two at a time, a
    batch of a thousand chunks or more three or four at a time and the small groupings one at a time.  All return `out`'s bits."""
    rows = 16 * lstm_stream_plan(size).nt
    ran = 0
    for start, m in ((pivot, rows), (pivot - rows + 1, rows), (pivot - rows - 2, rows + 3), (0, 1), (300, 600)):
        if start + m > n:
            continue
        part = infer(model, args, start, m)
        assert np.array_equal(bits(part), bits(out[start : start + m])), (ctx, start, m, float(np.abs(part - out[start : start + m]).max()))
        ran += 1
    assert ran >= 4, ctx


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("case", CASES16, ids=lambda c: f"{c.group}-{c.size}-{c.L}")
def test_16bit_widths_step_counts_and_chunk_batching(case, dtype):
    """conv_stream16_kernel and lstm_stream16_kernel at sizes 192 and 224 (six and seven waves; NT = 2 on 768 and 896 threads), at
    one, two and three LSTM steps (the swish of the last h falls into step 0 at T = 1) at sizes 96 and 256, and at size 96 with
    8 x CUs + 37 chunks, the smallest batch whose sig_conv3 and seq_conv2 keep eight chunks per iteration (launch_conv16_t halves
    cb until every CU has an iteration): its first 300 chunks, sent alone, run one chunk per iteration and return the same bits."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count  # what rmr_engine_create reads into the engine's num_cus
    n = case.n if case.n is not None else 8 * cus + 37
    c = _case16(case.size, case.L, n)
    model = make_model(c["state"], chunk_context(case.L), dtype)
    assert model.kernel_size == case.size
    ctx = f"{case.group} size {case.size} L {case.L} n {n}"
    out = check_statistics(c, model, dtype, n, ctx)
    check_groupings(model, c["args"], out, case.size, n, f"{ctx} {dtype}")
    if case.group == "cb8":
        spec = conv_layers(case.size, case.L)["sig_conv3"]
        plan = lambda m: conv16_plan(spec[0], spec[1], spec[2], spec[4], spec[5], m, cus)  # noqa: E731
        assert plan(n).cb == 8 and plan(8 * (cus - 1)).cb < 8 and plan(300).cb == 1, (cus, plan(n), plan(300))
        alone = infer(model, c["args"], 0, 300)
        assert np.array_equal(bits(alone), bits(out[:300])), (ctx, dtype, float(np.abs(alone - out[:300]).max()))


def test_16bit_lds_edge_runs_below_and_refuses_above():
    """Size 256 in bf16: at L = 464 merge_conv1 stages 150 rows of 512 channels, (150 + 5 + 2) x 1040 B = 163 280 B of the 163 584 a
    block may take - 64 chunks within the emulation's statistics, 3 chunks the same bits; at L = 467 (151 rows, 164 320 B) the call
    is refused by name ("... run in fp32 ...") before anything is launched, and the engine goes on serving the first model."""
    from remora_amd import RemoraError, synth

    size, fits, refused = LDS_EDGE16
    assert layer_rows(fits)[2] == 150 and layer_rows(refused)[2] == 151
    c = _case16(size, fits, 64)
    model = make_model(c["state"], chunk_context(fits), "bf16")
    ctx = f"lds edge size {size} L {fits}"
    out = check_statistics(c, model, "bf16", 64, ctx + " n 64")
    few = run_into_nan(model, c["dev"], 3, ctx + " n 3")
    assert np.array_equal(bits(few), bits(out[:3])), ctx
    d = synth.synth_chunks(3, refused, 20, KCB, NUM_OUT, True, shard=refused)
    long_model = make_model(c["state"], chunk_context(refused), "bf16")
    eng = long_model.engine
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        with pytest.raises(RemoraError, match="run in fp32"):
            long_model.infer_chunks(*[d[k] for k in KEYS], KCB)
        assert not eng.profile(), eng.profile()
    finally:
        eng.profile_enable(False)
    assert np.array_equal(bits(run_into_nan(model, c["dev"], 3, ctx + " n 3, after the refusal")), bits(few))
