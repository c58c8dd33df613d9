"""GPU tests of the LSTM heads' logit stores: every class count, every head width, fp32 and the 16-bit dtypes.

lstm_head_kernel<H> (k_lstm.hip) and lstm_bf16s_kernel<H, ...> (k_lstm_bf16s.hip) run 4 H threads per block and end a group of 16
chunks by storing 16 x num_out logits: 256 threads at H = 64 cover the 16 classes the engine admits, 128 threads at H = 32 cover
8 classes, 64 threads at H = 16 cover 4.  With one store per thread (`if (tid < 16 * num_out)`) a size-32 model of 9 or more
classes and a size-16 model of 5 or more left the last chunks of every group unwritten; the store is a loop strided by the block
size now (unrolled to the 16 x 16 logits the engine admits: one pass at H = 64, as before).  The output buffer handed to rmr_infer_chunks here is filled with NaN first, so a logit that is never written shows
as NaN whatever the allocator would have left there.

Networks are synth.synth_state's amplified ones (per-class logit std of a hundred gates or more, asserted below: a 1e-4 gate sees every layer); the reference
is oracle.torch_ref in float64 on oracle.compute_encoded_kmer_batch's one-hot tensor (torch_ref's own fp32 forward is within 8e-7
of it).  The helpers below are shared with tests/test_gpu_split_shapes.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KCB = (4, 4)
KEYS = ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")
N, N_BIG = 37, 1024 + 37  # above 1024 chunks size 64 takes lstm_head_kernel (sixteen chunks per block), not lstm_small_kernel
# max |logit - float64|: the project's own figures (the north star's 1e-4; SPLIT_TOL of tests/test_gpu_parity.py; f16 as in
# test_f16_dtype_refuses_what_it_cannot_run).  Plain bf16 has no absolute gate: assert_bf16_statistics below.
GATE = {"fp32": 1e-4, "bf16x6": 1e-4, "f16x3": 1e-4, "bf16x3": 5e-4, "f16": 4e-3}
# where the unfused 16-bit pipeline (conv_bf16s_kernel + lstm_bf16s_kernel, one part) holds 16-bit values: the site list of
# test_16bit_networks_of_more_than_64_channels (tests/test_gpu_fused.py)
STREAM16_SITES = ("wconv.sig3", "wconv.seq2", "wconv.merge1", "aconv.sig2", "aconv.seq1", "aconv.cat", "x", "wlstm", "h")
PRESCALES = (1.0, 1.19, 1.4426950408889634, 1.7)
_chunks, _refs = {}, {}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def frozen(a):
    a.setflags(write=False)
    return a


def chunk_case(L, n, msl, num_out=2, cg=True, shard=0):
    """(chunk arrays in KEYS order, one-hot k-mer tensor) of n synthetic chunks of L samples; computed once, read-only."""
    key = (L, n, msl, num_out, cg, shard)
    if key not in _chunks:
        from oracle import oracle as O
        from remora_amd import synth

        d = synth.synth_chunks(n, L, msl, KCB, num_out, cg, shard=shard)
        args = tuple(frozen(d[k]) for k in KEYS)
        _chunks[key] = (args, frozen(O.compute_encoded_kmer_batch(*KCB, *args[1:])))
    return _chunks[key]


def float64_logits(state, sig, enc):
    import torch

    from oracle import torch_ref

    with torch.no_grad():
        return frozen(torch_ref.from_state(state).double()(torch.tensor(sig).double(), torch.tensor(enc).double()).numpy())


def bf16_emulated_errors(state, sig, enc, exact, sites=STREAM16_SITES, fmt="bf16"):
    """|emulated 16-bit logits - float64| for the four `prescale` draws of oracle.lowp_emulation (one array per draw); `fmt`: "bf16"
    or "f16"."""
    import torch

    from oracle import lowp_emulation, torch_ref

    net = torch_ref.from_state(state)
    with torch.no_grad():
        return [frozen(np.abs(lowp_emulation.forward(net, torch.tensor(sig), torch.tensor(enc), sites=sites, fmt=fmt, prescale=ps).numpy() - exact))
                for ps in PRESCALES]


def assert_bf16_statistics(out, exact, emus, ctx):
    """Plain bf16 against the envelope of the emulation's draws, the form of test_16bit_networks_of_more_than_64_channels: the
    kernel's error is the arithmetic's - neither larger than the emulated rounding explains nor implausibly smaller."""
    gpu = np.abs(out - exact)
    emu_mean, emu_q99 = [float(e.mean()) for e in emus], [float(np.quantile(e, 0.99)) for e in emus]
    print(f"{ctx}: bf16 |err| mean {gpu.mean():.3e} q99 {np.quantile(gpu, 0.99):.3e} max {gpu.max():.3e}; "
          f"emulated mean {min(emu_mean):.3e}..{max(emu_mean):.3e} q99 {min(emu_q99):.3e}..{max(emu_q99):.3e}")
    stats = (ctx, float(gpu.mean()), emu_mean, float(np.quantile(gpu, 0.99)), emu_q99, float(gpu.max()))
    assert np.isfinite(out).all(), ctx
    assert gpu.mean() <= 1.3 * max(emu_mean) + 2e-5, stats
    assert np.quantile(gpu, 0.99) <= 2.0 * max(emu_q99) + 1e-4, stats
    assert min(emu_mean) <= 3.0 * gpu.mean() + 2e-5, stats


def assert_gate(out, exact, dtype, ctx):
    err = float(np.abs(out - exact).max())
    print(f"{ctx}: {dtype} max|out - float64| = {err:.3e} (gate {GATE[dtype]:.0e})")
    assert np.isfinite(out).all(), ctx
    assert err <= GATE[dtype], (ctx, dtype, err)
    return err


def make_model(state, cc, dtype):
    from remora_amd.model_util import model_from_state

    return model_from_state(state, dict(chunk_context=cc, kmer_context_bases=KCB), device=0, dtype=dtype)


def infer(model, args, start=0, n=None):
    n = len(args[3]) - start if n is None else n
    return model.infer_chunks(*[a[start : start + n] for a in args], KCB)


def infer_into_nan(model, dev_args, n):
    """rmr_infer_chunks on the first n chunks of device-resident chunk arrays, into a device tensor pre-filled with NaN."""
    import torch

    from remora_amd import _lib as L

    sig, seq, mp, ln = (t[:n].contiguous() for t in dev_args)
    out = torch.full((n, model.num_out), float("nan"), dtype=torch.float32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    L.check(model._lib.rmr_infer_chunks(model._h, p(sig), p(seq), int(seq.shape[1]), p(mp), int(mp.shape[1]), p(ln), KCB[0], KCB[1], n,
                                        p(out), None, L.MEM_DEVICE))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _head_case(size, num_out):
    """(state, chunk arrays, device copies, float64 logits of N_BIG C100 chunks) of one (size, class count); computed once."""
    if (size, num_out) not in _refs:
        import torch

        from remora_amd import synth

        state = synth.synth_state("conv_lstm", size, 9, num_out, seed=100 * size + num_out)
        args, enc = chunk_case(100, N_BIG, 20, shard=41)
        ref = float64_logits(state, args[0], enc)
        assert ref.std(axis=0).min() >= 1e-2  # the chunks are told apart in every class, by a hundred fp32 gates or more
        _refs[(size, num_out)] = (state, args, tuple(torch.tensor(a).cuda() for a in args), enc, ref)
    return _refs[(size, num_out)]


CLASS_COUNTS = (1, 4, 5, 8, 9, 16)
HEAD_CASES = ([(size, no, "fp32") for size in (16, 32, 64, 96) for no in CLASS_COUNTS] +
              [(32, no, dt) for no in (8, 9, 16) for dt in ("bf16", "bf16x3", "bf16x6", "f16x3")] +
              [(64, 16, dt) for dt in ("bf16", "f16", "f16x3")])


@pytest.mark.parametrize("size,num_out,dtype", HEAD_CASES)
def test_every_logit_is_written_and_correct(size, num_out, dtype):
    """C100 batches of 37 and of 1024 + 37 chunks (ragged last group of sixteen; more than one block) into a NaN-filled device
    buffer: no NaN is left and every logit is within the dtype's gate of the float64 network.  Class counts 4 | 5 and 8 | 9 are
    the last that 64 and 128 threads cover with one store each (H = 16, H = 32); 16 is the most the engine admits.  Size 64 in
    bf16 / f16 takes the fused kernels here (lstm_x16_g2_kernel: 32 x num_out stores on 512 threads), whose rounding sites are
    lowp_emulation's default list; size 32 in bf16 the unfused pipeline (STREAM16_SITES)."""
    state, args, dev, enc, ref = _head_case(size, num_out)
    model = make_model(state, (50, 50), dtype)
    assert model.kernel_size == size  # 16 / 32 / 64: the register-resident heads; 96: lstm_stream_kernel
    emus = None
    for n in (N, N_BIG):
        out = infer_into_nan(model, dev, n)
        ctx = f"size {size} num_out {num_out} n {n}"
        unwritten = np.argwhere(np.isnan(out))
        assert unwritten.size == 0, (ctx, dtype, f"{len(unwritten)} logits left unwritten, first (chunk, class): {unwritten[:4].tolist()}")
        if dtype == "bf16":
            if emus is None:
                from oracle import lowp_emulation

                emus = bf16_emulated_errors(state, args[0], enc, ref, sites=STREAM16_SITES if size <= 32 else lowp_emulation.ALL_SITES)
            assert_bf16_statistics(out, ref[:n], [e[:n] for e in emus], ctx)
        else:
            assert_gate(out, ref[:n], dtype, ctx)


@pytest.mark.parametrize("size", [16, 32, 64, 96])
def test_label_tally_of_sixteen_classes(size):
    """infer_chunks(..., label_counts=...) at 16 classes: count_kernel's 16 LDS bins and its `threadIdx.x < num_out` flush hold
    all of them - the tally is the histogram of the returned logits' first maxima, on top of what the array held.  The random fc
    bias alone would decide nearly every call, so it is shifted by the float64 logits' class means: every class gets calls."""
    state, args, _, _, ref = _head_case(size, 16)
    state = dict(state)
    state["fc.bias"] = (state["fc.bias"] - ref.mean(axis=0)).astype(np.float32)
    ref = ref + (state["fc.bias"].astype(np.float64) - _head_case(size, 16)[0]["fc.bias"].astype(np.float64))
    model = make_model(state, (50, 50), "fp32")
    counts = np.arange(16, dtype=np.int64)
    out = infer(model, args)
    again = model.infer_chunks(*args, KCB, label_counts=counts)
    assert np.array_equal(bits(out), bits(again))
    assert np.abs(out - ref).max() <= 1e-4
    hist = np.bincount(out.argmax(1), minlength=16)
    assert hist.sum() == N_BIG and (hist > 0).sum() >= 12, hist
    assert np.array_equal(counts - np.arange(16), hist), (size, counts, hist)


def test_widths_and_dtypes_the_heads_refuse():
    """The 16-bit matrix-core kernels contract 32 channels per step: bf16 and the split dtypes do not exist at a padded size of
    16, f16 (fused kernels only) not below 33 channels - RemoraError at load, no kernel launched."""
    from remora_amd import RemoraError, synth

    for size in (16, 9):
        state = synth.synth_state("conv_lstm", size, 9, 5, seed=1)
        for dtype in ("bf16", "bf16x3", "bf16x6", "f16x3", "f16"):
            with pytest.raises(RemoraError, match="not supported"):
                make_model(state, (50, 50), dtype)
    state = synth.synth_state("conv_lstm", 32, 9, 9, seed=1)
    with pytest.raises(RemoraError, match="not supported"):
        make_model(state, (50, 50), "f16")
    assert make_model(state, (50, 50), "bf16").kernel_size == 32
