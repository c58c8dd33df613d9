"""The chunk data kernels of remora_amd/csrc/k_data.hip at the shapes where they can go wrong - encode_kernel in every
instantiation and form, the validation tally, the label count, trim, the motif flags, normalisation and the chunks' read index -
each against the oracle or a numpy restatement of tests/data_cases.py that tests/test_host_data_cases.py has checked on the CPU.
Exact equality except for the winning probability and the loss sum, whose bounds are worked out where they are asserted."""
import ctypes

import numpy as np
import pytest

import data_cases as D
from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.fixture(scope="module")
def cus(torch_cuda):
    return int(torch_cuda.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def eng(torch_cuda):
    from remora_amd.engine import get_engine

    return get_engine(0)


# ---- encode ------------------------------------------------------------------------------------------------------------------------
def check_encode(torch, monkeypatch, kb, ka, arrs, ref, what, host=False):
    """compute_encoded_kmer_batch on device arrays (and on host arrays) under RMR_ENCODE_FORM 2, 1 and 0: the oracle's bits."""
    from remora_amd.encoded_kmers import compute_encoded_kmer_batch

    dev = [torch.from_numpy(a).cuda() for a in arrs]
    wrong = {}
    for form in (2, 1, 0):
        monkeypatch.setenv("RMR_ENCODE_FORM", str(form))
        got = compute_encoded_kmer_batch(kb, ka, *dev).cpu().numpy()
        assert got.shape == ref.shape and got.dtype == np.float32
        wrong[f"device form {form}"] = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        if host:
            got = compute_encoded_kmer_batch(kb, ka, *arrs)
            assert got.shape == ref.shape
            wrong[f"host form {form}"] = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"{what}: wrong elements of {ref.size}: {wrong}")
    assert not any(wrong.values()), (what, wrong)


@pytest.mark.parametrize("case", D.ENCODE_CASES, ids=lambda c: c.name)
def test_encode_every_shape(torch_cuda, O, monkeypatch, case):
    """37 chunks (a ragged last block) of every (K, L) of the case table - the shipped pairs, other shapes of their unrolled
    kernels, shapes with the shipped store counts that those kernels are wrong for, both sides of the code form's limits, the
    shortest and longest chunks - with chunks of 0, 1 and max_len bases and -1 bases inside the context.  While launch_encode
    chose the unrolled kernels by the store count alone, every `collide` case came back wrong under RMR_ENCODE_FORM 2 (142 of
    91 168 elements for 11 x 56 up to 12 777 of 133 200 for 15 x 60, measured on an MI355X) and right under 1 and 0.  Wrong
    elements per case then (device arrays; the count varies a little with what the LDS held): 6x150 325, 10x90 553, 12x75 4613,
    15x60 12777, 9x101 807, 9x202 562, 9x201 772, 12x152 8300, 6x301 550, 6x101 470, 6x102 344, 11x56 142, 3x202 171, 6x201 528,
    6x202 351, 12x100 5417."""
    arrs = D.encode_inputs(case.kb, case.ka, case.L, D.N_SWEEP, case.max_len)
    ref = O.compute_encoded_kmer_batch(case.kb, case.ka, *arrs)
    assert ref.shape == (D.N_SWEEP, 4 * (case.kb + case.ka + 1), case.L)
    check_encode(torch_cuda, monkeypatch, case.kb, case.ka, arrs, ref, case.name, host=case.name in D.HOST_FORM_CASES)


@pytest.mark.parametrize("width", D.WIDTHS)
def test_encode_row_widths_and_second_chunks(torch_cuda, O, monkeypatch, cus, width):
    """Rows of 64, 65, 128, 129, 256 and 257 elements (the array widths; the chunks are as short as before): one, two and four
    prefetched elements per lane and rows read where they are needed, with more chunks than the grid has waves - every wave
    publishes the rows it prefetched for its second chunk behind the first one's stores."""
    kb, ka, L = D.WIDTH_SHAPES[width]
    n = D.second_trip_chunks(cus)
    arrs = D.encode_inputs(kb, ka, L, n, 20, seq_w=width, map_w=width, seed=width)
    assert arrs[0].shape == (n, width) and arrs[1].shape == (n, width)
    ref = O.compute_encoded_kmer_batch(kb, ka, *arrs)
    check_encode(torch_cuda, monkeypatch, kb, ka, arrs, ref, f"width {width}, {n} chunks")


def test_encode_second_chunks_of_an_unrolled_kernel(torch_cuda, O, monkeypatch, cus):
    """(6, 100) with a second chunk for every wave: the unrolled stores with the prefetched rows consumed behind them."""
    n = D.second_trip_chunks(cus)
    arrs = D.encode_inputs(2, 3, 100, n, 20, seed=5)
    assert D.encode_plan(6, 100, arrs[0].shape[1], arrs[1].shape[1]).NST == 10
    ref = O.compute_encoded_kmer_batch(2, 3, *arrs)
    check_encode(torch_cuda, monkeypatch, 2, 3, arrs, ref, f"6 x 100, {n} chunks")


def test_encode_refuses_a_chunk_beyond_the_lds_limit(eng):
    """A chunk length whose position table does not fit the LDS a launch may take is refused by name, before any launch (the
    arrays are host arrays of the right sizes: the call stages them and stops at the launcher's check)."""
    from remora_amd import _lib as L

    kb, ka, length, max_len = D.ENCODE_REFUSED
    seqs, maps, lens = D.encode_inputs(kb, ka, length, 2, max_len)
    out = np.full((2, 4 * (kb + ka + 1), length), 7.0, np.float32)
    rc = L.lib().rmr_encode_kmers(eng.handle, kb, ka, seqs.ctypes.data, seqs.shape[1], maps.ctypes.data, maps.shape[1], lens.ctypes.data, 2,
                                  length, out.ctypes.data, L.MEM_HOST)
    msg = L.lib().rmr_last_error().decode()
    assert rc == -1 and "encode" in msg and "LDS" in msg and str(length) in msg, (rc, msg)   # RMR_ERR_INVALID
    assert (out == 7.0).all()
    eng.synchronize()


# ---- validation tally --------------------------------------------------------------------------------------------------------------
def run_tally(torch, eng, logits, labels, kf, loc, conf0, loss0, calls=1):
    """rmr_validation_tally `calls` times on the same buffers -> (call, win_prob, confusion, loss_sum)."""
    from remora_amd import _lib as L

    n, km = logits.shape
    d_logits, d_labels = torch.from_numpy(logits).cuda(), torch.from_numpy(labels.astype(np.int64)).cuda()
    conf, loss = torch.from_numpy(conf0.copy()).cuda(), torch.tensor([loss0], dtype=torch.float64, device="cuda")
    win, call = torch.full((n,), -5.0, dtype=torch.float32, device="cuda"), torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    loc = np.ascontiguousarray(loc, np.int32)
    torch.cuda.synchronize()
    for _ in range(calls):
        L.check(L.lib().rmr_validation_tally(eng.handle, d_logits.data_ptr(), d_labels.data_ptr(), n, km, kf, loc.ctypes.data, conf.data_ptr(),
                                             win.data_ptr(), call.data_ptr(), loss.data_ptr()))
    eng.synchronize()
    return call.cpu().numpy(), win.cpu().numpy(), conf.cpu().numpy(), float(loss.cpu()[0])


def check_tally(torch, eng, n, kf, form, loc, seed, nonfinite=False):
    """One batch, tallied twice into confusion counts and a loss sum that start non-zero."""
    km = int((loc >= 0).sum())
    rng = np.random.default_rng([seed, n, kf])
    labels = rng.integers(0, kf, n)
    x = D.tally_logits(n, km, seed, nonfinite=nonfinite)
    t = D.tally_ref(x, labels, kf, loc)
    conf0, loss0 = rng.integers(1, 1000, (kf, kf)).astype(np.int64), 12.5
    call, win, conf, loss = run_tally(torch, eng, x, labels, kf, loc, conf0, loss0, calls=2)
    what = f"n {n} labels {kf} outputs {km} ({form}{', non-finite rows' if nonfinite else ''})"
    wrong = np.flatnonzero(call != t.call)
    assert wrong.size == 0, (what, f"{wrong.size} calls differ from np.argmax, first row {wrong[0]}: {x[wrong[0]]} got {call[wrong[0]]} want {t.call[wrong[0]]}")
    assert np.array_equal(conf, conf0 + 2 * t.confusion), what
    fin = t.finite
    assert np.array_equal(np.isnan(win), np.isnan(t.win64)), what   # NaN for NaN (non-finite rows: nothing more)
    # one rounding of the difference, an expf within 2 ulp, kf - 1 additions, one division: (kf + 8) 2^-24 on the float64 softmax;
    # the plain float32 restatement stays within (kf + 4) 2^-24 on the same rows
    if fin.any():
        rel = np.abs(win[fin].astype(np.float64) - t.win64[fin]) / t.win64[fin]
        rel_np = np.abs(t.win32[fin].astype(np.float64) - t.win64[fin]) / t.win64[fin]
        print(f"{what}: win_prob worst relative error {rel.max() * 2**24:.2f} x 2^-24 (numpy float32: {rel_np.max() * 2**24:.2f})")
        assert rel_np.max() <= (kf + 4) * 2.0**-24, what
        assert rel.max() <= (kf + 8) * 2.0**-24, what
    if not nonfinite:
        # float64 sums in any order: n 2^-53 sum|term| is 3e-11 sum|term| at the largest n; 1e-9 leaves the atomics their order
        assert fin.all()
        want, scale = loss0 + 2 * t.terms.sum(), loss0 + 2 * np.abs(t.terms).sum()
        print(f"{what}: loss_sum {loss!r} want {want!r}, |diff| / sum|term| = {abs(loss - want) / scale:.2e}")
        assert abs(loss - want) <= 1e-9 * scale, what


@pytest.mark.parametrize("kf", D.NUM_LABELS)
def test_validation_tally_every_size_and_label_layout(torch_cuda, eng, cus, kf):
    """Every num_labels with num_out equal to it, permuted, and smaller with the unmodelled columns in front, in the middle and
    at the end; rows either side of a wave and of a block; ties (the first wins), rows that an unmodelled column wins, ties
    with it."""
    sizes = D.tally_sizes(cus)
    for form, loc in D.label_maps(kf).items():
        for n in sizes[:-1]:
            check_tally(torch_cuda, eng, n, kf, form, loc, seed=7)


@pytest.mark.parametrize("kf,form", [(2, "equal"), (3, "front"), (16, "permuted")])
def test_validation_tally_second_trip_of_the_capped_grid(torch_cuda, eng, cus, kf, form):
    n = D.tally_sizes(cus)[-1]
    assert (n + D.BLOCK - 1) // D.BLOCK > 4 * cus
    check_tally(torch_cuda, eng, n, kf, form, D.label_maps(kf)[form], seed=8)


@pytest.mark.parametrize("kf,form", [(1, "equal"), (2, "front"), (3, "permuted"), (5, "middle"), (8, "end"), (15, "equal"), (16, "equal"), (16, "front")])
def test_validation_tally_calls_non_finite_rows_as_argmax_does(torch_cuda, eng, kf, form):
    """Rows with NaN, +inf and -inf entries: the call is np.argmax's (the first NaN, else the first +inf), the confusion counts
    follow it, the probability is NaN exactly where the float64 softmax is.  (A `v > best` scan never calls a NaN outside
    column 0: 8 of 65 rows differed from np.argmax at every label count above 1 before the kernels compared for NaN.)"""
    for n in (65, 257, 4099):
        check_tally(torch_cuda, eng, n, kf, form, D.label_maps(kf)[form], seed=9, nonfinite=True)


def test_validation_tally_fills_the_last_bin(torch_cuda, eng):
    """16 labels, every row labelled 15 and called 15: all counts in bin 255 of the block's 256."""
    n, kf = 777, 16
    x = D.tally_logits(n, kf, 3, special=False)
    x[:, 15] = 60.0
    labels = np.full(n, 15, np.int64)
    conf0 = np.arange(256, dtype=np.int64).reshape(16, 16)
    call, win, conf, loss = run_tally(torch_cuda, eng, x, labels, kf, np.arange(16, dtype=np.int32), conf0, 0.25)
    want = conf0.copy()
    want[15, 15] += n
    assert (call == 15).all() and np.array_equal(conf, want)
    t = D.tally_ref(x, labels, kf, np.arange(16))
    assert abs(loss - 0.25 - t.terms.sum()) <= 1e-9 * (0.25 + np.abs(t.terms).sum())


# ---- label counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_out", D.COUNT_NUM_OUT)
def test_count_labels_every_size(torch_cuda, eng, cus, num_out):
    """np.bincount(np.argmax) added to counts that start non-zero, from host and from device memory, with ties and rows of
    NaN, +inf and -inf among the logits."""
    from remora_amd import _lib as L

    torch = torch_cuda
    for n in D.tally_sizes(cus):
        x = D.tally_logits(n, num_out, 11, nonfinite=True)
        start = np.arange(5, 5 + num_out, dtype=np.int64)
        want = start + D.count_ref(x, num_out)
        host = start.copy()
        L.check(L.lib().rmr_count_labels(eng.handle, x.ctypes.data, n, num_out, host.ctypes.data, L.MEM_HOST))
        d_x, d_counts = torch.from_numpy(x).cuda(), torch.from_numpy(start.copy()).cuda()
        torch.cuda.synchronize()
        L.check(L.lib().rmr_count_labels(eng.handle, d_x.data_ptr(), n, num_out, d_counts.data_ptr(), L.MEM_DEVICE))
        eng.synchronize()
        assert np.array_equal(host, want), (n, num_out, host - start, want - start)
        assert np.array_equal(d_counts.cpu().numpy(), want), (n, num_out)


def test_infer_chunks_counts_the_labels_of_its_own_logits(torch_cuda, O):
    from remora_amd.model_util import model_from_state

    g = golden("model_convlstm_s64_l200_o3.npz")
    size, kb, ka, length, num_out = (int(v) for v in g["params"])
    model = model_from_state(O.state_from_npz(g), dict(chunk_context=(length // 2, length - length // 2), kmer_context_bases=(kb, ka)), device=0)
    counts = np.array([100, 200, 300], np.int64)[:num_out].copy()
    start = counts.copy()
    logits = model.infer_chunks(g["sigs"], g["seqs"], g["maps"], g["lens"], (kb, ka), label_counts=counts)
    assert logits.shape == g["logits"].shape and num_out == 3
    assert np.array_equal(counts - start, np.bincount(np.argmax(logits, axis=1), minlength=num_out))


# ---- trim --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stored,kept", D.TRIM_CONTEXTS)
def test_trim_every_clip_combination(torch_cuda, O, eng, stored, kept):
    """Stored context longer than the kept one before, after, both and neither; 255, 256 and 257 chunks; chunks whose bases all
    lie left of the kept window, whose entries all lie beyond it, and chunks of one base - the oracle's arrays, from host and
    from device memory."""
    from remora_amd import _lib as L
    from remora_amd.data_chunks_core import trim_sb_chunk_context_core

    torch = torch_cuda
    (sb, sa), (cb, ca) = stored, kept
    for n in D.TRIM_SIZES:
        arrs = D.trim_inputs(stored, kept, n)
        want = [a.copy() for a in arrs]
        O.trim_sb_chunk_context_core(sb, sa, cb, ca, D.TRIM_SEQ_CONTEXT, *want)
        host = [a.copy() for a in arrs]
        trim_sb_chunk_context_core(sb, sa, cb, ca, D.TRIM_SEQ_CONTEXT, *host)
        dev = [torch.from_numpy(a.copy()).cuda() for a in arrs]
        torch.cuda.synchronize()
        L.check(L.lib().rmr_trim_chunk_context(eng.handle, sb, sa, cb, ca, D.TRIM_SEQ_CONTEXT, dev[0].data_ptr(), dev[0].shape[1], dev[1].data_ptr(),
                                               dev[1].shape[1], dev[2].data_ptr(), n, L.MEM_DEVICE))
        eng.synchronize()
        for name, w, h, d in zip(("seqs", "maps", "lens"), want, host, dev):
            assert np.array_equal(h, w), (n, name)
            assert np.array_equal(d.cpu().numpy(), w), (n, name)


# ---- motif flags -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.MOTIF_SETS))
def test_motif_flags_at_group_and_block_boundaries(torch_cuda, eng, name):
    """Reads that end at bases 15, 16, 17, 4095, 4096 and 4097 of the concatenation, empty reads first, twice in the middle and
    last, a last group of 7 bases: Motif.findall's hits per read, from host memory and from device memory with the flags
    16-byte aligned (one store per 16 bases) and one byte off (byte stores).  Motifs lying over a read boundary flag nothing."""
    from remora_amd import _lib as L

    torch = torch_cuda
    reads, motifs = D.motif_reads(), D.MOTIF_SETS[name]
    seq, off = D.concat_reads(reads)
    want, ms = D.motif_flags_ref(reads, motifs), D.motif_set(motifs)
    for motif, base in D.STRADDLES:
        if motifs == (motif,):
            assert want[base] == 0
    host = np.full(seq.size, 9, np.uint8)
    L.check(L.lib().rmr_motif_flags(eng.handle, seq.ctypes.data, off.ctypes.data, len(reads), ctypes.byref(ms), host.ctypes.data, L.MEM_HOST))
    assert np.array_equal(host, want), np.flatnonzero(host != want)[:10]
    d_seq, d_off = torch.from_numpy(seq).cuda(), torch.from_numpy(off).cuda()
    for shift in (0, 1):
        buf = torch.full((seq.size + 32,), 9, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        L.check(L.lib().rmr_motif_flags(eng.handle, d_seq.data_ptr(), d_off.data_ptr(), len(reads), ctypes.byref(ms), buf.data_ptr() + shift, L.MEM_DEVICE))
        eng.synchronize()
        got = buf.cpu().numpy()
        assert np.array_equal(got[shift : shift + seq.size], want), (shift, np.flatnonzero(got[shift : shift + seq.size] != want)[:10])
        assert (got[:shift] == 9).all() and (got[shift + seq.size :] == 9).all(), shift   # nothing written around the flags


# ---- extraction --------------------------------------------------------------------------------------------------------------------
def test_extract_reads_that_end_inside_groups_and_reads_without_chunks(torch_cuda, O):
    """Signals of 1, 7, 8, 9 and 2049 samples (normalise_kernel's groups of eight samples cross reads and end inside them),
    reads without focus bases first, twice in the middle and last (chunk_read_kernel's bisection passes reads without chunks),
    a read of one base, focus bases on first and last bases, an asymmetric chunk context: the oracle's signal and chunks."""
    from remora_amd.data_chunks import RemoraRead, extract_chunk_arrays

    cc, kcb = D.EXTRACT_CONTEXT, D.EXTRACT_KMER
    reads = []
    for i, r in enumerate(D.extract_reads()):
        reads.append(RemoraRead(dacs=r["dacs"], shift=r["shift"], scale=r["scale"], seq_to_sig_map=r["seq_to_sig_map"], int_seq=r["int_seq"],
                                read_id=f"r{i}", focus_bases=r["focus_bases"]))
    arrs, sig = extract_chunk_arrays(reads, cc, kcb)
    sig = sig.cpu().numpy()
    st = s_off = 0
    for rd in reads:
        osig = O.normalise_signal(rd.dacs, rd.shift, rd.scale)
        assert np.array_equal(sig[s_off : s_off + osig.size].view(np.uint32), osig.view(np.uint32)), rd.read_id
        s_off += osig.size
        if rd.focus_bases is None:
            continue
        ch = O.extract_chunks(osig, rd.seq_to_sig_map, rd.int_seq, rd.focus_bases, cc, kcb)
        n, sl = rd.focus_bases.size, ch["sequence_lengths"]
        assert np.array_equal(arrs.lengths[st : st + n].cpu().numpy(), sl), rd.read_id
        assert np.array_equal(arrs.signal[st : st + n].cpu().numpy().view(np.uint32), ch["signal"].view(np.uint32)), rd.read_id
        seqs, maps = arrs.sequence[st : st + n].cpu().numpy(), arrs.mapping[st : st + n].cpu().numpy()
        for i in range(n):
            assert np.array_equal(seqs[i, : sl[i] + sum(kcb)], ch["sequence"][i, : sl[i] + sum(kcb)]), (rd.read_id, i)
            assert np.array_equal(maps[i, : sl[i] + 1], ch["sequence_to_signal_mapping"][i, : sl[i] + 1]), (rd.read_id, i)
        assert np.array_equal(arrs.read_focus_bases[st : st + n].cpu().numpy(), ch["read_focus_bases"]), rd.read_id
        st += n
    assert s_off == sig.size and st == len(arrs) == 12
