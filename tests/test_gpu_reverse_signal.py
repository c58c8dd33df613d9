"""Reverse-signal reads (models whose metadata says reverse_signal: signal recorded 3'->5', src/remora/io.py:2001-2010,
:401-402) on the batch ingest: the reversed assembly kernel (rmr_assemble_reads_dir) against numpy, the batch ingest against
the per-read path it replaces - which tests/test_gpu_parity.py pins on reference-generated fixtures for this branch - bit
for bit, and the three users of the ingest (`infer from_pod5_and_bam`, `dataset prepare --reverse-signal`,
io.get_site_kmer_levels(reverse_signal=True)) against their per-read forms."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "data")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------
def _synthetic_batch(rng, kept_lengths):
    """Windows of a random int16 signal and random monotone mappings inside them: per read q[0] > 0, q[last] < span_len,
    q[last] - q[0] = the kept length asked for.  Window starts are odd and even, so source runs begin at every alignment; the
    kept lengths decide where the destination runs begin."""
    src_start, span_len, qs, pos = [], [], [], int(rng.randint(0, 7))
    for kept in kept_lengths:
        q0 = int(rng.randint(1, 40))
        n_seq = int(min(kept, rng.randint(1, 400)))
        inner = np.sort(rng.randint(0, kept + 1, n_seq - 1)) if n_seq > 1 else np.zeros(0, np.int64)
        qs.append(q0 + np.concatenate([[0], inner, [kept]]).astype(np.int64))
        span_len.append(q0 + kept + int(rng.randint(1, 30)))
        src_start.append(pos)
        pos += span_len[-1] + int(rng.randint(0, 9))
    signal = rng.randint(-32768, 32768, pos + 5).astype(np.int16)
    pad = [rng.randint(-5, 5, int(rng.randint(0, 4))).astype(np.int64) for _ in qs]  # the tables are not back to back
    q2s_off, q2s, at = [], [], 0
    for q, p in zip(qs, pad):
        q2s_off.append(at + p.size)
        q2s.extend([p, q])
        at += p.size + q.size
    return (signal, np.asarray(src_start, np.int64), np.asarray(span_len, np.int64), np.concatenate(q2s), np.asarray(q2s_off, np.int64),
            np.asarray([q.size - 1 for q in qs], np.int64), qs)


def _assemble(torch, eng, batch, reverse_signal, entry="rmr_assemble_reads_dir"):
    from remora_amd import _lib as L

    signal, src_start, span_len, q2s, q2s_off, seq_len, qs = batch
    n, dev = len(qs), eng.torch_device
    total = int(sum(q[-1] - q[0] for q in qs))
    d_signal, d_q2s = torch.from_numpy(signal).to(dev), torch.from_numpy(q2s).to(dev)
    dacs = torch.full((total + 64,), -12345, dtype=torch.int16, device=dev)  # room behind the last read: it must stay untouched
    s2s = torch.full((int(seq_len.sum()) + n + 8,), -99, dtype=torch.int64, device=dev)
    d_sig_off, d_seq_off = (torch.empty(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
    sig_off = np.full(n + 1, -1, np.int64)
    torch.cuda.synchronize()  # the fills above run on torch's stream, the kernels on the engine's own
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if entry == "rmr_assemble_reads_dir":
        L.check(L.lib().rmr_assemble_reads_dir(eng.handle, n, d_signal.data_ptr(), p(src_start), p(span_len), reverse_signal, d_q2s.data_ptr(),
                                               p(q2s_off), p(seq_len), dacs.data_ptr(), total, s2s.data_ptr(), d_sig_off.data_ptr(),
                                               d_seq_off.data_ptr(), p(sig_off)))
    else:
        L.check(L.lib().rmr_assemble_reads(eng.handle, n, d_signal.data_ptr(), p(src_start), d_q2s.data_ptr(), p(q2s_off), p(seq_len),
                                           dacs.data_ptr(), total, s2s.data_ptr(), d_sig_off.data_ptr(), d_seq_off.data_ptr(), p(sig_off)))
    return dacs.cpu().numpy(), s2s.cpu().numpy(), sig_off, d_sig_off.cpu().numpy(), d_seq_off.cpu().numpy()


BATCHES = {
    # every kept length at which the strided, reversed copy changes shape: shorter than one 8-byte word, one sample either side
    # of a block's 256 threads and of the 16 x 256 threads of a read's grid row, a read far longer than that
    "lengths": [1, 2, 255, 256, 257, 16 * 256 - 1, 16 * 256 + 1, 70001, 3, 4, 5, 7, 8, 9, 1],
    "one read": [1000],
    "one read of one sample": [1],
    "ends of length 1": [1, 517, 1],
}


@pytest.mark.parametrize("name", list(BATCHES))
def test_reversed_assembly_equals_numpy(torch_cuda, name):
    """dacs_i = trimmed_i[::-1][q0:q1], s2s_i = q - q0 - exact; with reverse_signal = 0 the forward slice, and the very arrays
    rmr_assemble_reads writes."""
    from remora_amd.engine import get_ingest_engine

    eng = get_ingest_engine(0)
    batch = _synthetic_batch(np.random.RandomState(len(name)), BATCHES[name])
    signal, src_start, span_len, _, _, seq_len, qs = batch
    old = _assemble(torch_cuda, eng, batch, 0, entry="rmr_assemble_reads")
    for reverse_signal in (0, 1):
        dacs, s2s, sig_off, d_sig_off, d_seq_off = got = _assemble(torch_cuda, eng, batch, reverse_signal)
        want_sig_off = np.concatenate([[0], np.cumsum([q[-1] - q[0] for q in qs])])
        want_seq_off = np.concatenate([[0], np.cumsum(seq_len)])
        assert np.array_equal(sig_off, want_sig_off) and np.array_equal(d_sig_off, want_sig_off) and np.array_equal(d_seq_off, want_seq_off)
        for i, q in enumerate(qs):
            trimmed = signal[src_start[i] : src_start[i] + span_len[i]]
            want = (trimmed[::-1] if reverse_signal else trimmed)[q[0] : q[-1]]
            assert want.size == BATCHES[name][i]
            assert np.array_equal(dacs[sig_off[i] : sig_off[i + 1]], want), (name, reverse_signal, i)
            assert np.array_equal(s2s[want_seq_off[i] + i : want_seq_off[i + 1] + i + 1], q - q[0]), (name, reverse_signal, i)
        assert (dacs[sig_off[-1] :] == -12345).all() and (s2s[want_seq_off[-1] + len(qs) :] == -99).all()
        if not reverse_signal:
            assert all(np.array_equal(a, b) for a, b in zip(got, old))


def test_reversed_assembly_turns_away_a_mapping_outside_its_window(torch_cuda):
    """The reversed copy addresses the signal from the END of the window: a mapping that leaves [0, span_len] fails the call
    before anything is copied."""
    from remora_amd import RemoraError
    from remora_amd.engine import get_ingest_engine

    batch = list(_synthetic_batch(np.random.RandomState(3), [40, 50]))
    batch[2] = batch[2].copy()
    batch[2][1] = int(batch[6][1][-1]) - 1  # one sample less than the mapping's end
    with pytest.raises(RemoraError, match="leaves its signal window"):
        _assemble(torch_cuda, get_ingest_engine(0), batch, 1)


# ---- 2. the batch ingest against the per-read path -----------------------------------------------------------------------
def _per_read(rio, pod5, bam, pa_scaling, skip_non_primary, ref_anchored):
    want, want_err = [], []
    for read, err in rio.iter_reads_from_pod5_and_bam(pod5, bam, reverse_signal=True, pa_scaling=pa_scaling, skip_non_primary=skip_non_primary,
                                                      parse_ref_align=ref_anchored, decode_batch=4):
        if err is None:
            try:
                want.append(read.into_remora_read(ref_anchored))
                want_err.append(None)
                continue
            except rio.RemoraError as e:
                err = f"Read prep error: {e}"
        want_err.append(err)
    return want, want_err


def _compare_ingest(rio, pod5, bam, pa_scaling, skip_non_primary, ref_anchored, batch):
    want, want_err = _per_read(rio, pod5, bam, pa_scaling, skip_non_primary, ref_anchored)
    got_err, k = [], 0
    for ib in rio.iter_ingest_batches(pod5, bam, pa_scaling=pa_scaling, skip_non_primary=skip_non_primary, batch=batch,
                                      ref_anchored=ref_anchored, reverse_signal=True):
        assert isinstance(ib, rio.IngestBatch), "the batch was handed back to the per-read path"
        got_err.extend(ib.err)
        if not ib.good.size:
            continue
        dr = ib.dr
        dacs, s2s, iseq = dr.dacs.cpu().numpy(), dr.s2s.cpu().numpy(), dr.iseq.cpu().numpy()
        shift, scale = dr.shift.cpu().numpy(), dr.scale.cpu().numpy()
        for g in range(ib.good.size):
            rr = want[k]
            k += 1
            assert np.array_equal(dacs[dr.sig_off[g] : dr.sig_off[g + 1]], rr.dacs)
            assert np.array_equal(s2s[dr.seq_off[g] + g : dr.seq_off[g + 1] + g + 1], rr.seq_to_sig_map)
            assert np.array_equal(iseq[dr.seq_off[g] : dr.seq_off[g + 1]], rr.int_seq)
            assert shift[g] == rr.shift and scale[g] == rr.scale  # the same float64 operations: equal, not close
            assert ib.reads[g].shift == rr.shift and ib.reads[g].scale == rr.scale
    assert k == len(want) and got_err == want_err
    return want, want_err


@pytest.mark.parametrize("ref_anchored", [False, True])
@pytest.mark.parametrize("prefix", ["can", "mod"])
def test_reverse_signal_ingest_batches_equal_the_per_read_path(torch_cuda, prefix, ref_anchored, tmp_path):
    """Both anchors, with and without pa_scaling, secondary records skipped and kept, on the reference's test alignments with
    records of every kind the ingest turns away in between (tests/test_gpu_ingest.py builds that file): error text or none,
    dacs, mapping, int_seq, shift, scale of every record - and every batch an IngestBatch."""
    from remora_amd import io as rio
    from test_gpu_ingest import _dirty_bam

    pod5 = os.path.join(DATA, f"{prefix}_reads.pod5")
    bam = str(tmp_path / "dirty.bam")
    _dirty_bam(bam, prefix, with_missing_moves=not ref_anchored)
    forward = next(iter(rio.iter_reads_from_pod5_and_bam(pod5, bam, parse_ref_align=False)))[0].into_remora_read(False).dacs
    for skip_non_primary in (True, False):
        for pa_scaling in (None, (87.5, 14.25)):
            want, want_err = _compare_ingest(rio, pod5, bam, pa_scaling, skip_non_primary, ref_anchored, batch=4)
            assert len(want) >= 10 and sum(e is not None for e in want_err) == (2 if ref_anchored else 3)
        # 15 records, one of them of a read the POD5 file does not hold, one secondary
        assert len(want_err) == (13 if skip_non_primary else 14)
    if not ref_anchored:  # and it is the reversed signal that was compared
        assert not np.array_equal(want[0].dacs, forward)


@pytest.mark.parametrize("ref_anchored", [False, True])
def test_reverse_signal_reads_without_scaling_tags_stay_on_the_batch_ingest(torch_cuda, ref_anchored, tmp_path):
    """Records without sm / sd (tests/test_gpu_ingest.py strips them): median and MAD are order statistics of the window, the
    GPU histograms do not care which way it is read - same shift and scale as np.median on the reversed samples."""
    from remora_amd import io as rio
    from test_gpu_ingest import _dirty_bam

    pod5 = os.path.join(DATA, "can_reads.pod5")
    bam = str(tmp_path / "untagged.bam")
    _dirty_bam(bam, "can", with_missing_moves=False, without_scaling_tags=True)
    assert sum(not {"sm", "sd"} <= set(dict(rec.tags)) for rec in rio.iter_bam_records(bam)) == 4
    for pa_scaling in (None, (87.5, 14.25)):
        want, _ = _compare_ingest(rio, pod5, bam, pa_scaling, True, ref_anchored, batch=5)
        assert len(want) >= 10


# ---- 3. infer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [False, True])
def test_reverse_signal_infer_output_is_the_same_file_with_and_without_the_batch_ingest(torch_cuda, refine, tmp_path, monkeypatch):
    """A reverse-signal model (metadata reverse_signal: true; the s64 ConvLSTM golden weights), alone and with a non-iterative
    signal-mapping refiner, both anchors: the output BAM of the default run - which must take the batch ingest - and of
    RMR_INFER_BATCH_INGEST=0 are the same bytes."""
    from oracle import oracle as O
    from remora_amd import io as rio
    from remora_amd.inference import infer_from_pod5_and_bam
    from remora_amd.model_util import load_model, model_from_state
    from remora_amd.refine_signal_map import SigMapRefiner
    from test_gpu_parity import _mint_pt, _real_reads_golden

    g = _real_reads_golden("can")
    _, md = load_model(_mint_pt(tmp_path, g, O), device=0)
    md = dict(md, reverse_signal=True)
    if refine:
        md["sig_map_refiner"] = SigMapRefiner(kmer_model_filename=os.path.join(DATA, "levels_4mer.txt"), do_rough_rescale=True, scale_iters=0,
                                              do_fix_guage=True)
        assert md["sig_map_refiner"].is_loaded
    model = model_from_state(O.state_from_npz(g), md, device=0)
    batches = []
    real = rio.iter_ingest_batches

    def counted(*a, **k):
        assert k.get("reverse_signal") is True
        for ib in real(*a, **k):
            batches.append(isinstance(ib, rio.IngestBatch))
            yield ib

    monkeypatch.setattr(rio, "iter_ingest_batches", counted)
    pod5, bam = os.path.join(DATA, "can_reads.pod5"), os.path.join(DATA, "can_mappings.bam")
    forward = str(tmp_path / "forward.bam")
    for ref_anchored in (False, True):
        outs, stats = [], []
        for mode in ("1", "0"):
            monkeypatch.setenv("RMR_INFER_BATCH_INGEST", mode)
            del batches[:]
            out = str(tmp_path / f"o{mode}.bam")
            stats.append(infer_from_pod5_and_bam(pod5, bam, model, md, out, reads_per_batch=5, ref_anchored=ref_anchored))
            outs.append(open(out, "rb").read())
            assert (len(batches) >= 2 and all(batches)) if mode == "1" else not batches, "which ingest ran"
        assert stats[0] == stats[1] and stats[0][None] >= 10 and outs[0] == outs[1]
        # not the forward-signal file
        monkeypatch.setenv("RMR_INFER_BATCH_INGEST", "0")
        infer_from_pod5_and_bam(pod5, bam, model, dict(md, reverse_signal=False), forward, reads_per_batch=5, ref_anchored=ref_anchored)
        assert open(forward, "rb").read() != outs[0]


# ---- 4. dataset prepare ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["can_ctrl", "can_refine"])
def test_reverse_signal_dataset_prepare_writes_the_same_directory_on_either_path(torch_cuda, name, tmp_path, monkeypatch):
    """extract_chunk_dataset(..., rev_sig=True) on the batch ingest (counted) and with RMR_PREPARE_BATCH_INGEST=0: every file of
    the dataset directory byte for byte, and metadata that says reverse_signal."""
    import json

    import remora_amd.prepare_train_data as ptd
    from remora_amd.refine_signal_map import SigMapRefiner
    from remora_amd.util import Motif
    from test_gpu_parity import _prep_args

    _, which, mod_base, kw = _prep_args(name)
    assert not kw["basecall_anchor"] and kw["bed"] is None

    def run(out_dir):
        refiner = SigMapRefiner()
        if kw["refine"]:
            refiner = SigMapRefiner(kmer_model_filename=os.path.join(DATA, "levels_4mer.txt"), do_rough_rescale=True, scale_iters=0,
                                    do_fix_guage=True)
        np.random.seed(11)
        ptd.extract_chunk_dataset(
            bam_path=os.path.join(DATA, f"{which}_mappings.bam"), pod5_path=os.path.join(DATA, f"{which}_reads.pod5"), out_path=out_dir,
            mod_base=mod_base, mod_base_control=mod_base is None, motifs=[Motif(*m) for m in kw["motifs"]], focus_ref_pos=None,
            chunk_context=kw["chunk_context"], min_samps_per_base=kw["min_samps_per_base"], max_chunks_per_read=kw["max_chunks_per_read"],
            pa_scaling=None, sig_map_refiner=refiner, kmer_context_bases=kw["kmer_context_bases"], base_start_justify=kw["base_start_justify"],
            offset=kw["offset"], num_reads=None, basecall_anchor=False, rev_sig=True, reads_per_batch=5)

    calls = []
    real = ptd.extract_chunk_arrays_from_ingest
    monkeypatch.setattr(ptd, "extract_chunk_arrays_from_ingest", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    run(str(tmp_path / "batch"))
    assert len(calls) >= 2, "the batch ingest did not run"
    n_batch_calls = len(calls)
    monkeypatch.setenv("RMR_PREPARE_BATCH_INGEST", "0")
    run(str(tmp_path / "reads"))
    assert len(calls) == n_batch_calls
    files = sorted(os.listdir(tmp_path / "batch"))
    assert files == sorted(os.listdir(tmp_path / "reads")) and "metadata.jsn" in files and len(files) >= 5
    for f in files:
        assert open(tmp_path / "batch" / f, "rb").read() == open(tmp_path / "reads" / f, "rb").read(), f
    assert json.load(open(tmp_path / "batch" / "metadata.jsn"))["reverse_signal"] is True
    assert os.path.getsize(tmp_path / "batch" / "signal.npy") > 1000


# ---- 5. k-mer levels -------------------------------------------------------------------------------------------------------
def _site_levels_numpy(reads, kb, ka, min_cov):
    """{k-mer index: [site levels]} of the reads of ONE contig - (is_reverse, ref_start, read-oriented base codes,
    read-oriented trimmean) each: per strand the reads side by side over the contig in read orientation, a site's level =
    np.median of its finite values where there are min_cov of them and its k-mer has no base missing.  What
    tests/test_gpu_metrics.py::_region_kmer_levels restates of io.get_region_kmers (src/remora/io.py:966-982), visiting only the
    covered sites instead of every offset of the contig."""
    k = kb + ka + 1
    lo = min(r[1] for r in reads)
    span = max(r[1] + r[2].size for r in reads) - lo
    out = {}
    for rev in (False, True):
        mine = [r for r in reads if r[0] == rev]
        mat = np.full((len(mine), span), np.nan)
        seq = np.full(span + kb + ka, -2, np.int64)  # read-oriented; [kb + o] is the base of read-oriented offset o
        for row, (_, start, codes, vals) in enumerate(mine):
            o0 = span - (start - lo + codes.size) if rev else start - lo
            mat[row, o0 : o0 + codes.size] = vals
            seq[kb + o0 : kb + o0 + codes.size] = codes
        finite = np.isfinite(mat)
        for offset in np.nonzero(finite.sum(axis=0) >= min_cov)[0].tolist():
            kmer = seq[offset : offset + k]
            if (kmer < 0).any():
                continue
            idx = int(sum(int(b) * 4 ** (k - 1 - j) for j, b in enumerate(kmer)))
            out.setdefault(idx, []).append(np.median(mat[finite[:, offset], offset]))
    return out


def test_reverse_signal_site_kmer_levels_equal_the_per_read_path(torch_cuda):
    """io.get_site_kmer_levels(..., reverse_signal=True) against reads built one by one with reverse_signal=True, refined on
    the reference anchor, io.Read.compute_per_base_metric("dwell_trimmean") per read and the median per site in numpy
    (_site_levels_numpy) - equal to the last bit.  --min-coverage 3: the files
    cover a site at most 10 times on one strand and 4 on the other."""
    from remora_amd import RemoraError
    from remora_amd import io as rio
    from remora_amd.refine_signal_map import SigMapRefiner
    from remora_amd.util import seq_to_int

    pod5, bam, table = (os.path.join(DATA, f) for f in ("can_reads.pod5", "can_mappings.bam", "levels_4mer.txt"))
    kb, ka, min_cov = 2, 2, 3
    refiner = SigMapRefiner(kmer_model_filename=table, scale_iters=0, do_fix_guage=True)
    got = rio.get_site_kmer_levels(pod5, bam, refiner, (kb, ka), min_cov=min_cov, reverse_signal=True)
    by_ctg = {}
    for io_read, err in rio.iter_reads_from_pod5_and_bam(pod5, bam, reverse_signal=True):
        if err is not None or io_read.ref_to_signal is None:
            continue
        try:
            io_read.set_refine_signal_mapping(refiner, ref_mapping=True)
        except RemoraError:  # a read the refiner rejects is left out, there as here
            continue
        tm = io_read.compute_per_base_metric("dwell_trimmean", start_trim=1, end_trim=1)["trimmean"]
        by_ctg.setdefault(io_read.ref_reg.ctg, []).append((io_read.ref_reg.strand == "-", io_read.ref_reg.start,
                                                          np.asarray(seq_to_int(io_read.ref_seq)), tm))
    assert sum(len(v) for v in by_ctg.values()) >= 10
    want = {}
    for reads in by_ctg.values():
        for idx, lv in _site_levels_numpy(reads, kb, ka, min_cov).items():
            want.setdefault(idx, []).extend(lv)
    k = kb + ka + 1
    assert len(got) == 4**k and sum(len(v) for v in want.values()) >= 50
    for idx in range(4**k):
        kmer = "".join("ACGT"[(idx >> (2 * (k - 1 - j))) & 3] for j in range(k))
        exp = np.sort(np.asarray(want.get(idx, []), np.float64))
        assert got[kmer].dtype == np.float64 and np.array_equal(got[kmer].view(np.uint64), exp.view(np.uint64)), kmer
    # and these are not the levels of the signal read forwards
    fwd = rio.get_site_kmer_levels(pod5, bam, refiner, (kb, ka), min_cov=min_cov)
    assert any(not np.array_equal(fwd[kmer], got[kmer]) for kmer in got)
