"""The region API on the GPU (rmr_region_base_metrics, rmr_region_signals, remora_amd/region_metrics.py) on the 14-record fixtures
of tests/golden/data: every row against the per-read path bit for bit, against the reference's values
(tests/golden/region_metrics.npz, tools/gen_golden.py --only regions), independent of batching and of how regions are grouped,
sampled as the reference samples, and refused when a pair does not fit.

The regions (chr13, names as in the golden):
    a_fwd / a_rev   52310000-52310100   7 / 3 reads of `can` (8 / 4 of `mod`); one reverse read ends at 52310007: 7 covered
                                        positions, then NaN, and the row is flipped under ref_orient
    b_fwd / b_rev   52308990-52309050   9 / 4 reads; reads that start at 52309013 and 52309018 give leading NaN
    one_read        52317000-52317050   exactly one read
    nobody          52300000-52300100   no read: an error in the single call, None in the plural form
    one_base, wide  52310000-52310001, -52310200   one base; more than three 64-base groups per read"""
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, golden
from metrics_exact import exact_stats, mean_bound, var_bound

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, "data")
METRICS = ("dwell", "dwell_mean", "dwell_mean_sd", "dwell_trimmean", "dwell_trimmean_trimsd")
TRIMS = ((1, 1), (0, 3))
WITH_READS = ("a_fwd", "a_rev", "b_fwd", "b_rev", "one_read", "one_base", "wide")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fx():
    return golden("region_metrics.npz")


def _paths(sample):
    return os.path.join(DATA, f"{sample}_reads.pod5"), os.path.join(DATA, f"{sample}_mappings.bam")


def _region(fx, name):
    from remora_amd import io as rio

    ctg, strand, start, end = fx["regions"][list(fx["region_names"]).index(name)]
    return rio.RefRegion(str(ctg), str(strand), int(start), int(end))


def _refiner():
    from remora_amd.refine_signal_map import SigMapRefiner

    return SigMapRefiner(kmer_model_filename=os.path.join(DATA, "levels_4mer.txt"), do_rough_rescale=True, scale_iters=0, do_fix_guage=True)


_READS = {}


def _per_read(sample, refined=False, reverse_signal=False):
    """{query name: io.Read} of the per-read path (Read.from_pod5 + add_alignment, refined one by one as
    set_refine_signal_mapping(refiner, ref_mapping=True) does).  Built once per flavour; nobody changes them."""
    from remora_amd import io as rio

    key = (sample, refined, reverse_signal)
    if key not in _READS:
        pod5, bam = _paths(sample)
        reads = {}
        for read, err in rio.iter_reads_from_pod5_and_bam(pod5, bam, reverse_signal=reverse_signal):
            if err is not None or read.ref_to_signal is None:
                continue
            if refined:
                read.set_refine_signal_mapping(_refiner(), ref_mapping=True)
            reads[read.record.query_name] = read
        _READS[key] = reads
    return _READS[key]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)  # (float32 dwell widens exactly)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("refined", [False, True], ids=["unrefined", "refined"])
def test_rows_equal_the_per_read_path(torch_cuda, fx, refined):
    """Every row of every region, metric, trim and orientation is Read.compute_per_base_metric(metric, region=...) of the same
    read on the per-read path, bit for bit (that path is held to the reference by tests/test_gpu_metrics.py)."""
    from remora_amd import io as rio

    regs = [_region(fx, name) for name in WITH_READS]
    reads = _per_read("can", refined)
    refiner = _refiner() if refined else None
    rows_seen = 0
    for metric in METRICS:
        for st, en in TRIMS:
            want = {}
            for orient in (False, True):
                got = rio.get_ref_regs_samples_metrics(regs, [_paths("can")], sig_map_refiner=refiner, metric=metric, ref_orient=orient,
                                                       start_trim=st, end_trim=en)
                for name, reg, (samples_metrics, all_recs) in zip(WITH_READS, regs, got):
                    (mets,), (recs,) = samples_metrics, all_recs
                    assert list(mets) == list(reads[recs[0].query_name].compute_per_base_metric(metric, region=reg, start_trim=st, end_trim=en))
                    for row, rec in enumerate(recs):
                        if (name, row) not in want:
                            want[name, row] = reads[rec.query_name].compute_per_base_metric(metric, region=reg, start_trim=st, end_trim=en)
                        for key, mat in mets.items():
                            assert mat.shape == (len(recs), reg.len)
                            exp = want[name, row][key]
                            exp = exp[::-1] if orient and reg.strand == "-" else exp
                            assert _same_bits(mat[row], exp), (metric, st, en, orient, name, row, key)
                        rows_seen += 1
    assert rows_seen == len(METRICS) * len(TRIMS) * 2 * (7 + 3 + 9 + 4 + 1 + 7 + 7)


def _golden_cases(fx):
    return sorted({k[: -len("_n_samples")] for k in fx.files if k.startswith("m_") and k.endswith("_n_samples")})


def _parse_case(case):
    name, samples, rest = case[2:].split("_can", 1)[0], None, None
    samples = ["can", "mod"] if "_can+mod_" in case else ["can"]
    rest = case.split("+mod_" if len(samples) == 2 else "_can_", 1)[1]
    metric, orient = rest.rsplit("_", 1)
    return name, samples, metric, orient == "ref"


def test_against_the_reference_golden(torch_cuda, fx):
    """Row count, read ids in row order, keys, dtype and NaN pattern equal the reference's; dwell is equal; and for every covered
    base, with n its samples after the trims (bounds: tests/metrics_exact.py, the inequality of tests/test_gpu_metrics.py)
        |gpu - exact| <= mean_bound        |gpu - ref| <= |ref - exact| + mean_bound
    for mean / trimmean and the same with var_bound for sd^2 / trimsd^2.  No refiner: the golden's mapping is the move table's."""
    from remora_amd import RemoraError
    from remora_amd import io as rio

    trims = {"dwell_mean_sd": (0, 0), "dwell_trimmean_trimsd": (1, 1), "dwell_trimmean": (2, 2)}
    worst = {"mean": 0.0, "mean_vs_ref": 0.0, "var": 0.0, "var_vs_ref": 0.0}
    exact = {}
    cases = _golden_cases(fx)
    assert len(cases) == 54
    for case in cases:
        name, samples, metric, orient = _parse_case(case)
        reg = _region(fx, name)
        st, en = trims[metric]
        kw = {} if metric == "dwell_mean_sd" else {"start_trim": st, "end_trim": en}
        mets, recs = rio.get_ref_reg_samples_metrics(reg, [_paths(s) for s in samples], metric=metric, ref_orient=orient, **kw)
        assert len(mets) == len(recs) == int(fx[f"{case}_n_samples"]) == len(samples)
        for s, sample in enumerate(samples):
            ids = fx[f"{case}_s{s}_ids"].tolist()
            assert [r.query_name for r in recs[s]] == ids, case
            assert list(mets[s]) == fx[f"{case}_s{s}_keys"].tolist(), case
            for key, mat in mets[s].items():
                ref = fx[f"{case}_s{s}_{key}"]
                assert mat.dtype == ref.dtype and mat.shape == ref.shape, (case, key, mat.dtype, ref.dtype)
                assert np.array_equal(np.isnan(mat), np.isnan(ref)), (case, key)
                assert not np.isinf(mat).any()
            dkey = "dwells" if metric == "dwell_trimmean" else "dwell"
            assert np.array_equal(mets[s][dkey], fx[f"{case}_s{s}_{dkey}"], equal_nan=True), case
            mname = "mean" if metric == "dwell_mean_sd" else "trimmean"
            sname = {"dwell_mean_sd": "sd", "dwell_trimmean_trimsd": "trimsd"}.get(metric)
            for row, rid in enumerate(ids):
                read = _per_read(sample)[rid]
                sig, m, mine = read.norm_signal, read.ref_to_signal, read.ref_reg
                rev = mine.strand == "-"
                for col in np.nonzero(~np.isnan(fx[f"{case}_s{s}_{mname}"][row]))[0].tolist():
                    pos = reg.start + (reg.len - 1 - col if (rev and not orient) else col)  # reference position of the column
                    base = mine.end - 1 - pos if rev else pos - mine.start
                    k = (sample, rid, base, st, en)
                    if k not in exact:
                        x = sig[int(m[base]) + st : int(m[base + 1]) - en].tolist()
                        exact[k] = (len(x),) + exact_stats(x)
                    n, mean, var, sabs, ssq = exact[k]
                    g, r = mets[s][mname][row, col], fx[f"{case}_s{s}_{mname}"][row, col]
                    bm = mean_bound(n, sabs)
                    worst["mean"] = max(worst["mean"], abs(g - mean) / bm)
                    worst["mean_vs_ref"] = max(worst["mean_vs_ref"], abs(g - r) / (abs(r - mean) + bm))
                    assert abs(g - mean) <= bm and abs(g - r) <= abs(r - mean) + bm, (case, row, col, g, r, mean, bm)
                    if sname is not None:
                        gv, rv, bv = mets[s][sname][row, col] ** 2, fx[f"{case}_s{s}_{sname}"][row, col] ** 2, var_bound(n, ssq, mean)
                        worst["var"] = max(worst["var"], abs(gv - var) / bv)
                        worst["var_vs_ref"] = max(worst["var_vs_ref"], abs(gv - rv) / (abs(rv - var) + bv))
                        assert abs(gv - var) <= bv and abs(gv - rv) <= abs(rv - var) + bv, (case, row, col, gv, rv, var, bv)
    print("bases checked:", len(exact), "worst error / bound:", worst)
    assert len(exact) > 8000 and {k[0] for k in exact} == {"can", "mod"} and max(worst.values()) <= 1.0, worst
    # nobody covers the region: the reference's error in the single call, None in the plural one, the neighbours untouched
    nobody = _region(fx, "nobody")
    with pytest.raises(RemoraError, match="^No reads covering region$"):
        rio.get_ref_reg_samples_metrics(nobody, [_paths("can")])
    assert str(fx["m_nobody_can_dwell_mean_sd_ref_error"]) == "No reads covering region"
    with pytest.raises(RemoraError, match="^No reads covering region$"):
        rio.get_reads_reference_regions(nobody, [_paths("can")])
    plural = rio.get_ref_regs_samples_metrics([nobody, _region(fx, "one_read")], [_paths("can")])
    assert plural[0] is None and plural[1][0][0]["trimmean"].shape == (1, 50)


def test_reads_reference_regions(torch_cuda, fx):
    """get_reads_reference_regions against the golden (seq, seq_to_sig_map, sig_start, ref_reg equal; norm_signal the same
    correctly rounded float64 expression: np.array_equal) and against the host Read.extract_ref_reg, field by field; "dac" and
    "pa" against the host form as well."""
    from remora_amd import io as rio

    names = ("a_fwd", "a_rev", "b_fwd", "b_rev", "one_base")
    regs = [_region(fx, n) for n in names]
    many = rio.get_reads_reference_regions_many(regs, [_paths("can")], max_reads=None)
    reads = _per_read("can")
    for name, reg, got in zip(names, regs, many):
        (rrs,), (recs,) = got
        assert [r.query_name for r in recs] == fx[f"x_{name}_ids"].tolist() and len(rrs) == len(recs)
        single = rio.get_reads_reference_regions(reg, [_paths("can")], max_reads=None)
        for i, (rr, rec) in enumerate(zip(rrs, recs)):
            k = f"x_{name}_r{i}"
            assert isinstance(rr, rio.ReadRefReg) and rr.read_id == str(fx[f"{k}_read_id"]) and rr.seq == str(fx[f"{k}_seq"]), k
            assert np.array_equal(rr.seq_to_sig_map, fx[f"{k}_map"]) and rr.seq_to_sig_map.dtype == np.int64, k
            assert int(rr.sig_start) == int(fx[f"{k}_sig_start"]), k
            assert [rr.ref_reg.ctg, rr.ref_reg.strand, str(rr.ref_reg.start), str(rr.ref_reg.end)] == fx[f"{k}_ref_reg"].tolist(), k
            assert rr.norm_signal.dtype == np.float64 and np.array_equal(rr.norm_signal, fx[f"{k}_sig"]), k
            assert np.array_equal(rr.ref_sig_coords, fx[f"{k}_coords"]), k
            for other in (reads[rec.query_name].extract_ref_reg(reg), single[0][0][i]):
                assert (other.read_id, other.seq, other.ref_reg, int(other.sig_start)) == (rr.read_id, rr.seq, rr.ref_reg, int(rr.sig_start))
                assert np.array_equal(other.seq_to_sig_map, rr.seq_to_sig_map)
                assert _same_bits(other.norm_signal, rr.norm_signal)
    for signal_type, dtype in (("dac", np.int16), ("pa", np.float64)):
        (rrs,), (recs,) = rio.get_reads_reference_regions(regs[1], [_paths("can")], max_reads=None, signal_type=signal_type)
        for rr, rec in zip(rrs, recs):
            want = reads[rec.query_name].extract_ref_reg(regs[1], signal_type=signal_type)
            assert rr.norm_signal.dtype == dtype == want.norm_signal.dtype
            assert np.array_equal(rr.norm_signal, want.norm_signal) and np.array_equal(rr.seq_to_sig_map, want.seq_to_sig_map)
    # refined: mapping and scaling are the refiner's on both paths
    refined = _per_read("can", refined=True)
    (rrs,), (recs,) = rio.get_reads_reference_regions(regs[3], [_paths("can")], sig_map_refiner=_refiner(), max_reads=None)
    for rr, rec in zip(rrs, recs):
        want = refined[rec.query_name].extract_ref_reg(regs[3])
        assert np.array_equal(rr.seq_to_sig_map, want.seq_to_sig_map) and int(rr.sig_start) == int(want.sig_start)
        assert _same_bits(rr.norm_signal, want.norm_signal)


def _flat(result):
    """Everything a plural metrics result holds, as bytes per region."""
    out = []
    for got in result:
        if got is None:
            out.append(None)
            continue
        mets, recs = got
        out.append(([[r.query_name for r in sample] for sample in recs],
                    [[(k, v.dtype.str, v.shape, v.tobytes()) for k, v in m.items()] for m in mets]))
    return out


def test_results_do_not_depend_on_batching_or_grouping(torch_cuda, fx):
    """The same bits for reads_per_batch 4 and 256, for the single-region call and the plural call, and for the region list in
    either order - with the refiner, two samples, and a region nobody covers among the others."""
    from remora_amd import io as rio

    names = WITH_READS[:4] + ("nobody", "wide")
    regs = [_region(fx, n) for n in names]
    pairs = [_paths("can"), _paths("mod")]
    kw = dict(sig_map_refiner=_refiner(), metric="dwell_trimmean_trimsd")
    base = _flat(rio.get_ref_regs_samples_metrics(regs, pairs, reads_per_batch=256, **kw))
    assert base[4] is None and all(b is not None for b in base[:4])
    assert _flat(rio.get_ref_regs_samples_metrics(regs, pairs, reads_per_batch=4, **kw)) == base
    assert _flat(rio.get_ref_regs_samples_metrics(regs[::-1], pairs, reads_per_batch=4, **kw))[::-1] == base
    for reg, want in zip(regs, base):
        if want is not None:
            assert _flat([rio.get_ref_reg_samples_metrics(reg, pairs, **kw)]) == [want]
    sig = [rio.get_reads_reference_regions_many(regs, pairs, max_reads=None, reads_per_batch=b) for b in (4, 256)]
    for a, b in zip(*sig):
        assert (a is None) == (b is None)
        if a is not None:
            for ra, rb in zip(a[0][0] + a[0][1], b[0][0] + b[0][1]):
                assert ra.read_id == rb.read_id and ra.norm_signal.tobytes() == rb.norm_signal.tobytes()
                assert np.array_equal(ra.seq_to_sig_map, rb.seq_to_sig_map)


def test_sampling_draws_the_reference_rows(torch_cuda, fx):
    """max_reads=3 under random.seed(7), two regions and two samples in one run of the random numbers (for region: for sample:):
    the rows the reference drew, in its order, with its values' NaN pattern and dwells."""
    from remora_amd import io as rio

    regs, pairs = [_region(fx, "a_fwd"), _region(fx, "a_rev")], [_paths("can"), _paths("mod")]
    random.seed(7)
    plural = rio.get_ref_regs_samples_metrics(regs, pairs, max_reads=3, metric="dwell_trimmean", start_trim=1, end_trim=1)
    random.seed(7)
    singles = [rio.get_ref_reg_samples_metrics(reg, pairs, max_reads=3, metric="dwell_trimmean", start_trim=1, end_trim=1) for reg in regs]
    assert _flat(plural) == _flat(singles)
    full = rio.get_ref_regs_samples_metrics(regs, pairs, metric="dwell_trimmean", start_trim=1, end_trim=1)
    for name, (mets, recs), (all_mets, all_recs) in zip(("a_fwd", "a_rev"), plural, full):
        for s in range(2):
            ids = [r.query_name for r in recs[s]]
            assert ids == fx[f"sampled_{name}_s{s}_ids"].tolist() and len(ids) == 3
            assert np.array_equal(mets[s]["dwells"], fx[f"sampled_{name}_s{s}_dwells"], equal_nan=True)
            assert mets[s]["dwells"].dtype == fx[f"sampled_{name}_s{s}_dwells"].dtype
            order = [[r.query_name for r in all_recs[s]].index(i) for i in ids]  # a sampled row is the unsampled call's row of that read
            assert _same_bits(mets[s]["trimmean"], all_mets[s]["trimmean"][order])


def test_reverse_signal(torch_cuda, fx):
    """reverse_signal=True (reads built as for signal recorded 3'->5') equals the per-read path built the same way."""
    from remora_amd import io as rio

    reg = _region(fx, "b_rev")
    reads = _per_read("can", reverse_signal=True)
    (mets,), (recs,) = rio.get_ref_reg_samples_metrics(reg, [_paths("can")], reverse_signal=True, metric="dwell_trimmean_trimsd")
    assert len(recs) == 4
    fwd = rio.get_ref_reg_samples_metrics(reg, [_paths("can")], metric="dwell_trimmean_trimsd")[0][0]
    assert not _same_bits(mets["trimmean"], fwd["trimmean"])
    for row, rec in enumerate(recs):
        want = reads[rec.query_name].compute_per_base_metric("dwell_trimmean_trimsd", region=reg)
        for key in mets:
            assert _same_bits(mets[key][row], want[key][::-1]), (row, key)
    (rrs,), _ = rio.get_reads_reference_regions(reg, [_paths("can")], reverse_signal=True, max_reads=None)
    for rr, rec in zip(rrs, recs):
        want = reads[rec.query_name].extract_ref_reg(reg)
        assert np.array_equal(rr.seq_to_sig_map, want.seq_to_sig_map) and int(rr.sig_start) == int(want.sig_start)
        assert _same_bits(rr.norm_signal, want.norm_signal)


def test_caller_chosen_records_and_missing_reads(torch_cuda, fx):
    """get_ref_reg_sample_metrics on records the caller chose equals the streamed call's rows; a record whose signal is not in the
    POD5 raises the reference's error, or is left out with missing_ok."""
    import dataclasses

    from remora_amd import RemoraError
    from remora_amd import io as rio

    reg = _region(fx, "a_rev")
    (mets,), (recs,) = rio.get_ref_reg_samples_metrics(reg, [_paths("can")], sig_map_refiner=_refiner(), metric="dwell_mean_sd")
    pod5 = rio.Pod5File(_paths("can")[0])
    chosen = rio.get_ref_reg_sample_metrics(reg, pod5, recs[::-1], "dwell_mean_sd", _refiner())
    assert list(chosen) == list(mets)
    for key in mets:
        assert chosen[key].dtype == mets[key].dtype and _same_bits(chosen[key], mets[key][::-1]), key
    assert rio.get_ref_reg_sample_metrics(reg, pod5, [], "dwell_mean_sd", None) is None
    stranger = dataclasses.replace(rio.BamRecord(**{f.name: getattr(recs[0], f.name, None) for f in dataclasses.fields(rio.BamRecord)}),
                                   query_name="not-in-the-pod5")
    with pytest.raises(RemoraError, match="^BAM record not found in POD5$"):
        rio.get_ref_reg_sample_metrics(reg, pod5, [recs[0], stranger], "dwell_mean_sd", None)
    kept = rio.get_ref_reg_sample_metrics(reg, pod5, [recs[0], stranger], "dwell_mean_sd", None, missing_ok=True)
    assert kept["mean"].shape == (1, reg.len)


def test_only_covering_reads_are_decoded_and_no_read_object_is_built(torch_cuda, fx, monkeypatch):
    """The batch path: records are picked from the raw batches' fixed fields, so the POD5 is asked for the signal rows of the
    covering reads alone (one read for `one_read`), and no io.Read is built on the way - with the refiner as without."""
    from remora_amd import io as rio

    asked = []
    rows_of_reads = rio.Pod5File.rows_of_reads

    def spy(self, read_rows):
        asked.append(len(read_rows))
        return rows_of_reads(self, read_rows)

    def no_reads(*a, **k):
        raise AssertionError("the per-read path was taken")

    monkeypatch.setattr(rio.Pod5File, "rows_of_reads", spy)
    monkeypatch.setattr(rio, "_reads_of_records", no_reads)
    got = rio.get_ref_regs_samples_metrics([_region(fx, "nobody"), _region(fx, "one_read")], [_paths("can")], sig_map_refiner=_refiner())
    assert got[0] is None and got[1][0][0]["trimmean"].shape == (1, 50) and asked == [1]
    del asked[:]
    rio.get_reads_reference_regions(_region(fx, "a_rev"), [_paths("can")], max_reads=2, reads_per_batch=4)
    assert sum(asked) == 2  # sampled before anything is decoded


def test_an_iterative_refiner_goes_read_by_read_through_the_same_kernels(torch_cuda, fx):
    """scale_iters=1 is not covered by the resident refiner: the reads are refined one by one and measured by the same kernels;
    the rows equal the per-read path's.  (The iterative re-scaling draws its Theil-Sen points with np.random: both sides start
    from the same seed and refine the reads in row order.)"""
    from remora_amd import io as rio
    from remora_amd.refine_signal_map import SigMapRefiner

    make = lambda: SigMapRefiner(kmer_model_filename=os.path.join(DATA, "levels_4mer.txt"), do_rough_rescale=True, scale_iters=1,  # noqa: E731
                                 do_fix_guage=True)
    reg = _region(fx, "b_rev")
    np.random.seed(5)
    (mets,), (recs,) = rio.get_ref_reg_samples_metrics(reg, [_paths("can")], sig_map_refiner=make(), metric="dwell_mean_sd")
    plain = rio.get_ref_reg_samples_metrics(reg, [_paths("can")], sig_map_refiner=_refiner(), metric="dwell_mean_sd")[0][0]
    assert not _same_bits(mets["mean"], plain["mean"])
    np.random.seed(5)
    for row, rec in enumerate(recs):
        read = _per_read("can")[rec.query_name].copy()
        read.set_refine_signal_mapping(make(), ref_mapping=True)
        want = read.compute_per_base_metric("dwell_mean_sd", region=reg)
        for key in mets:
            assert _same_bits(mets[key][row], want[key][::-1]), (row, key)


def test_bad_pairs_are_refused_before_any_launch(torch_cuda, fx):
    """A pair that does not fit its read, its region or the output raises RemoraError from DeviceReads.region_metrics /
    region_signals; nothing is launched (the profiler counts no launch) and nothing is written.  A good pair beside it runs."""
    from remora_amd import RemoraError
    from remora_amd.data_chunks import DeviceReads

    rng = np.random.default_rng(9)

    class R:
        def __init__(self, nb):
            dw = rng.integers(1, 12, size=nb)
            self.seq_to_sig_map = np.concatenate([[0], np.cumsum(dw)]).astype(np.int64)
            self.dacs = rng.integers(-500, 1500, size=int(self.seq_to_sig_map[-1])).astype(np.int16)
            self.shift, self.scale, self.int_seq, self.read_id = 400.0, 90.0, np.zeros(nb, np.int8), None

    dr = DeviceReads([R(70), R(200)])
    eng = dr.engine
    good = [1, 60, 200, 5, 0, 150, 1]
    whole = {k: v.cpu().numpy() for k, v in dr.per_base_metrics("dwell_trimmean_trimsd", 1, 1).items()}
    got = {k: v.cpu().numpy() for k, v in dr.region_metrics([good], "dwell_trimmean_trimsd", 1, 1).items()}
    one = slice(int(dr.seq_off[1]) + 60, int(dr.seq_off[1]) + 200)
    for key in got:
        assert got[key].shape == (1, 150) and np.isnan(got[key][0, :5]).all() and np.isnan(got[key][0, 145:]).all()
        assert _same_bits(got[key][0, 5:145][::-1], whole[key][one]), key  # flipped: column 150 - 1 - (5 + i)
    bad = {
        "read outside the batch": [2, 0, 10, 0, 0, 10, 0],
        "negative read": [-1, 0, 10, 0, 0, 10, 0],
        "last beyond the read": [0, 60, 71, 0, 0, 11, 0],
        "empty span": [0, 10, 10, 0, 0, 10, 0],
        "negative first": [0, -1, 10, 0, 0, 11, 0],
        "lead pushes past the region": [0, 0, 10, 1, 0, 10, 0],
        "negative lead": [0, 0, 10, -1, 0, 10, 0],
        "row outside the output": [0, 0, 10, 0, 3, 10, 0],
        "negative row": [0, 0, 10, 0, -1, 10, 0],
        "flip that is no flag": [0, 0, 10, 0, 0, 10, 2],
    }
    eng.profile_enable(True)
    eng.profile_reset()
    for why, pair in bad.items():
        with pytest.raises(RemoraError):
            dr.region_metrics([good, pair], "dwell_trimmean", rows=2, width=150)
        if "row" not in why and "lead" not in why:
            with pytest.raises(RemoraError):
                dr.region_signals([good, pair])
    with pytest.raises(RemoraError):
        dr.region_metrics([good, [0, 0, 10, 0, 0, 10, 0]], "dwell_trimmean", rows=2, width=150)  # two pairs for one row
    with pytest.raises(RemoraError):
        dr.region_metrics([good], "dwell_trimmean", rows=1, width=149)  # a region wider than the output
    with pytest.raises(RemoraError):
        dr.region_metrics([good[:5]], "dwell_trimmean")  # too few columns
    prof = eng.profile()
    eng.profile_enable(False)
    assert prof.get("region_metrics", (0.0, 0))[1] == 0 and prof.get("region_signals", (0.0, 0))[1] == 0, prof
    sig, sig_off, smap, map_off, start = dr.region_signals([good, [0, 3, 9, -4, -1, 0, 0]])  # lead, row, region length: not looked at
    m1, m0 = dr.s2s.cpu().numpy()[71:], dr.s2s.cpu().numpy()[:71]
    assert sig_off.tolist() == [0, int(m1[200] - m1[60]), int(m1[200] - m1[60] + m0[9] - m0[3])] and start.tolist() == [int(m1[60]), int(m0[3])]
    assert np.array_equal(smap[map_off[0] : map_off[1]], m1[200] - m1[60:201][::-1]) and np.array_equal(smap[map_off[1] :], m0[3:10] - m0[3])
    d1 = dr.dacs.cpu().numpy()[int(dr.sig_off[1]) :]
    assert np.array_equal(sig[: sig_off[1]], ((d1[m1[60] : m1[200]] - 400.0) / 90.0)[::-1])
