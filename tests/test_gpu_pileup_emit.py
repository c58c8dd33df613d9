"""The emit pair of the C ABI, rmr_pileup_emit_counts / _fill, driven directly with every valid combination of its options on
one batch: the synthetic duplex records of test_host_pileup_duplex.py, whose '-' entries and off-motif calls are what the modes
differ on.  Status, counts, histogram and the records' words are compared with the restatements the suite has for each mode -
equal integers -, so an options struct that reaches the wrong launcher gives a wrong answer here."""
import ctypes

import numpy as np
import pytest

import modbam_restate as mr
import test_gpu_pileup as tp
import test_gpu_pileup_coverage as tc
import test_gpu_pileup_ref as tgr
import test_host_pileup_duplex as hd

pytestmark = pytest.mark.gpu

REFS, ALPHABET, MOTIF, K_T = tp.REFS, ["C", "m"], hd.CG, 307
FAIL = len(ALPHABET)  # the code of a call below the threshold: n_mods + 1
# name -> (ref, combine, duplex, hemi): {ref NULL, ref plain, ref folded} x {duplex 0, 1}, and hemi
MODES = {"plain": (False, 0, 0, 0), "ref": (True, 0, 0, 0), "ref_fold": (True, 1, 0, 0), "duplex": (False, 0, 1, 0),
         "duplex_ref": (True, 0, 1, 0), "duplex_ref_fold": (True, 1, 1, 0), "hemi": (True, 1, 1, 1)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def emit_input(torch_cuda, tmp_path_factory):
    """The records, their genome as text and on the device, and the one device batch they make."""
    from remora_amd.engine import get_engine
    from remora_amd.pileup import RefGenome

    recs, genome, _ = hd.synth()
    d = tmp_path_factory.mktemp("pileup_emit")
    bam, fa = str(d / "duplex.bam"), str(d / "genome.fa")
    mr.write_bam(bam, REFS, recs)
    with open(fa, "w") as fh:
        fh.write(tgr.fasta_text([(name, seq) for (name, _), seq in zip(REFS, genome)], 60))
    eng = get_engine(None)
    batches = list(tc.device_batches(eng, bam, ALPHABET[1:], len(REFS)))
    assert len(batches) == 1 and int(batches[0][1].n_records) == len(recs)
    with RefGenome.from_fasta(fa, [n for n, _ in REFS], [ln for _, ln in REFS]) as g:
        yield eng, recs, genome, g, batches[0]


def restated(recs, genome, mode):
    """-> (status per record, [(ref_id, pos, strand, class, kmax)] per record, each call where the mode writes it)."""
    has_ref, combine, duplex, hemi = MODES[mode]
    record_calls = hd.record_calls if duplex else tp.record_calls
    statuses, calls = [], []
    d = len(MOTIF[0]) - 1 - 2 * MOTIF[1]
    for rec in recs:
        st, cs = record_calls(rec, ALPHABET)
        if hemi:  # kept as with the reference, folded as combine folds, the strand bit kept
            cs = [(c[0], c[1] - d if c[2] else c[1], c[2], c[3], c[4]) for c in hd.hemi_record(rec, ALPHABET, genome, MOTIF)[0]]
        elif has_ref:
            cs = [p for p in (tgr.place(c, genome, [MOTIF], bool(combine)) for c in cs) if p is not None]
        statuses.append(st)
        calls.append(cs)
    return statuses, calls


def test_restatements_tell_the_modes_apart():
    """What makes the input the smallest that a wrong dispatch fails on: every mode keeps calls, and no two modes keep the
    same words."""
    recs, genome, _ = hd.synth()
    seen = {}
    for mode in MODES:
        statuses, calls = restated(recs, genome, mode)
        words = tuple(tuple(sorted(tp.word(c[0], c[1], c[2], c[3]) for c in cs)) for cs in calls)
        assert sum(map(len, calls)) > 100 and statuses.count(0) > 40, mode
        assert words not in seen.values(), (mode, [m for m, w in seen.items() if w == words])
        seen[mode] = words
    assert restated(recs, genome, "plain")[0] != restated(recs, genome, "duplex")[0]  # (status 5 is asked of both strands' entries)


@pytest.mark.parametrize("mode", list(MODES))
def test_every_combination_of_the_options_equals_its_restatement(torch_cuda, emit_input, mode):
    from remora_amd import _lib as L
    from remora_amd.pileup import _pileup_ref_struct, check_pileup_motifs

    torch = torch_cuda
    eng, recs, genome, dev_genome, (buf, b, n_cig, n_deltas) = emit_input
    lib, dev, n = L.lib(), eng.torch_device, len(recs)
    has_ref, combine, duplex, hemi = MODES[mode]
    pref = _pileup_ref_struct(dev_genome, check_pileup_motifs([MOTIF], ALPHABET[0], bool(combine)), bool(combine)) if has_ref else None
    opts = L.PileupEmitOpts(region_ref=-1, ref=None if pref is None else ctypes.pointer(pref), duplex=duplex, hemi=hemi)
    want_status, want_calls = restated(recs, genome, mode)
    want_hist = np.bincount([c[4] for cs in want_calls for c in cs], minlength=513)

    ords = torch.empty(max(n_deltas, 1), dtype=torch.int32, device=dev)
    cig_q, cig_r = (torch.empty(max(n_cig, 1), dtype=torch.int64, device=dev) for _ in range(2))
    counts = torch.full((n,), -7, dtype=torch.int64, device=dev)
    status = torch.full((n,), -7, dtype=torch.int32, device=dev)
    hist = torch.zeros(513, dtype=torch.int64, device=dev)
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        L.check(lib.rmr_pileup_emit_counts(eng.handle, ctypes.byref(b), ctypes.byref(opts), ords.data_ptr(), cig_q.data_ptr(), cig_r.data_ptr(),
                                           counts.data_ptr(), status.data_ptr(), hist.data_ptr()))
        eng.synchronize()
        assert status.cpu().tolist() == want_status
        assert counts.cpu().tolist() == [len(cs) for cs in want_calls]
        assert np.array_equal(hist.cpu().numpy(), want_hist)
        out_off = np.zeros(n + 1, np.int64)
        np.cumsum([len(cs) for cs in want_calls], out=out_off[1:])
        total, guard = int(out_off[-1]), 0x7EAD_BEEF_0BAD_F00D
        words = torch.full((total + 1,), guard, dtype=torch.int64, device=dev)
        d_off = torch.from_numpy(out_off).to(dev)
        L.check(lib.rmr_pileup_emit_fill(eng.handle, ctypes.byref(b), ctypes.byref(opts), K_T, ords.data_ptr(), cig_q.data_ptr(), cig_r.data_ptr(),
                                         status.data_ptr(), d_off.data_ptr(), words.data_ptr()))
        eng.synchronize()
        got = words.cpu().numpy()
        assert int(got[-1]) == guard
        got = got[:-1].view(np.uint64).tolist()
        want = [sorted(tp.word(c[0], c[1], c[2], c[3] if c[4] >= K_T else FAIL) for c in cs) for cs in want_calls]
        bad = [r for r in range(n) if sorted(got[out_off[r] : out_off[r + 1]]) != want[r]]
        assert not bad, (mode, bad[:5])
        assert any(w & 15 == FAIL for w in got) and (not hemi or any(w & 16 for w in got))  # (the threshold and the kept strand bit bite)
        assert eng.profile()["pileup_emit"][1] == 2  # the count pass and the fill pass, under the emit's name
        # no record: both passes return 0 and launch nothing
        eng.profile_reset()
        b.n_records = 0
        try:
            rc = (lib.rmr_pileup_emit_counts(eng.handle, ctypes.byref(b), ctypes.byref(opts), ords.data_ptr(), cig_q.data_ptr(), cig_r.data_ptr(),
                                             counts.data_ptr(), status.data_ptr(), hist.data_ptr()),
                  lib.rmr_pileup_emit_fill(eng.handle, ctypes.byref(b), ctypes.byref(opts), K_T, ords.data_ptr(), cig_q.data_ptr(), cig_r.data_ptr(),
                                           status.data_ptr(), d_off.data_ptr(), words.data_ptr()))
        finally:
            b.n_records = n
        eng.synchronize()
        assert rc == (0, 0) and not any(k.startswith("pileup_") for k in eng.profile()), (rc, eng.profile())
        assert np.array_equal(hist.cpu().numpy(), want_hist) and words.cpu().numpy()[:-1].view(np.uint64).tolist() == got
    finally:
        eng.profile_enable(False)
