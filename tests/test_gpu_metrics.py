"""Per-base signal metrics (rmr_base_metrics) and the k-mer level table (rmr_site_kmer_levels) on the GPU: against the
reference's values (tests/golden/base_metrics.npz), against exactly rounded sums, independent of the batch, and the two-stage
median against a numpy restatement of io.get_region_kmers; `analyze estimate_kmer_levels` end to end."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden
from metrics_exact import N_READS, cases, mean_bound, var_bound

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, "data")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def fx():
    return golden("base_metrics.npz")


class _R:
    """What DeviceReads gathers from."""

    def __init__(self, dacs, seq_to_sig, shift, scale):
        self.dacs, self.seq_to_sig_map, self.shift, self.scale = dacs, np.asarray(seq_to_sig, np.int64), float(shift), float(scale)
        self.int_seq, self.read_id = np.zeros(self.seq_to_sig_map.size - 1, np.int8), None


def _fixture_reads(fx):
    return [_R(fx[f"r{i}_dacs"], fx[f"r{i}_map"], fx["shift"][i], fx["scale"][i]) for i in range(N_READS)]


@pytest.fixture(scope="module")
def gpu_metrics(torch_cuda, fx):
    """All five outputs for the fixture's reads as ONE batch, per trim: {trim index: {name: per-read arrays}}."""
    from remora_amd.data_chunks import DeviceReads

    dr = DeviceReads(_fixture_reads(fx))
    out = {}
    for t, (st, en) in enumerate(fx["trims"].tolist()):
        a = {k: v.cpu().numpy() for k, v in dr.per_base_metrics("dwell_mean_sd", st, en).items()}
        b = {k: v.cpu().numpy() for k, v in dr.per_base_metrics("dwell_trimmean_trimsd", st, en).items()}
        assert np.array_equal(a["dwell"], b["dwell"])
        a.update(b)
        out[t] = {k: [v[dr.seq_off[i] : dr.seq_off[i + 1]] for i in range(N_READS)] for k, v in a.items()}
    return out


def test_per_base_metrics_against_the_reference_and_the_exact_sums(fx, gpu_metrics):
    """dwell equal, NaN in the same places, and for every base of every read and trim (bounds: tests/metrics_exact.py)
        |gpu - exact| <= mean_bound                           |gpu - ref| <= |ref - exact| + mean_bound
    for mean and trimmean, and the same with var_bound for the variances sd^2 and trimsd^2.  That the reference alone is
    consistent with these bounds on this fixture is checked without a GPU in tests/test_host_metrics.py.  The worst ratios
    error / bound seen are printed and stand in the assertion messages."""
    worst = {"mean": 0.0, "mean_vs_ref": 0.0, "var": 0.0, "var_vs_ref": 0.0}
    for i in range(N_READS):
        for t in gpu_metrics:
            assert np.array_equal(gpu_metrics[t]["dwell"][i], fx[f"r{i}_dwell"]), (i, t)
    for case in cases(fx):
        i, t, mname, sname, ref_m, ref_s = (case[k] for k in ("read", "trim", "mean_name", "sd_name", "ref_mean", "ref_sd"))
        g_m, g_s = gpu_metrics[t][mname][i], gpu_metrics[t][sname][i]
        assert np.array_equal(np.isnan(g_m), np.isnan(ref_m)), (i, t, mname)
        assert np.array_equal(np.isnan(g_s), np.isnan(ref_s)), (i, t, sname)
        assert not np.isinf(g_m).any() and not np.isinf(g_s).any()
        for base, n, mean, var, sabs, ssq in case["bases"]:
            bm, bv = mean_bound(n, sabs), var_bound(n, ssq, mean)
            em, er = abs(g_m[base] - mean), abs(g_m[base] - ref_m[base])
            worst["mean"] = max(worst["mean"], em / bm)
            worst["mean_vs_ref"] = max(worst["mean_vs_ref"], er / (abs(ref_m[base] - mean) + bm))
            gv, rv = g_s[base] ** 2, ref_s[base] ** 2
            ev, evr = abs(gv - var), abs(gv - rv)
            worst["var"] = max(worst["var"], ev / bv)
            worst["var_vs_ref"] = max(worst["var_vs_ref"], evr / (abs(rv - var) + bv))
            assert em <= bm, (i, t, mname, base, em, bm, worst)
            assert er <= abs(ref_m[base] - mean) + bm, (i, t, mname, base, er, worst)
            assert ev <= bv, (i, t, sname, base, ev, bv, worst)
            assert evr <= abs(rv - var) + bv, (i, t, sname, base, evr, worst)
    print("worst error / bound:", worst)
    assert max(worst.values()) <= 1.0, worst


def test_a_reads_metrics_do_not_depend_on_the_batch(torch_cuda, fx, gpu_metrics):
    """The same bits alone, as one of 300 reads at batch positions 0 and 299, and from io.Read.compute_per_base_metric."""
    from remora_amd import io as rio
    from remora_amd.data_chunks import DeviceReads

    rng = np.random.default_rng(5)
    fillers = []
    for _ in range(299):
        dw = rng.integers(0, 14, size=int(rng.integers(1, 90)))
        mp = np.concatenate([[0], np.cumsum(dw)])
        fillers.append(_R(rng.integers(-500, 1500, size=max(int(mp[-1]), 1)).astype(np.int16), mp, rng.uniform(300, 500), rng.uniform(50, 150)))
    names = ("dwell", "trimmean", "trimsd")
    for i in (3, 6, 7):  # 65 bases; the dwells 0 .. 5000; the clipped read of 130 bases
        read = _fixture_reads(fx)[i]
        want = {k: gpu_metrics[0][k][i] for k in names}  # inside the fixture's batch of 8, trims (1, 1)
        alone = {k: v.cpu().numpy() for k, v in DeviceReads([read]).per_base_metrics("dwell_trimmean_trimsd", 1, 1).items()}
        for pos in (0, 299):
            batch = fillers[:pos] + [read] + fillers[pos:]
            dr = DeviceReads(batch)
            got = {k: v.cpu().numpy()[dr.seq_off[pos] : dr.seq_off[pos + 1]] for k, v in dr.per_base_metrics("dwell_trimmean_trimsd", 1, 1).items()}
            for k in names:
                assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (i, pos, k)
        io_read = rio.Read(read_id="r", dacs=read.dacs, ref_to_signal=read.seq_to_sig_map, shift_dacs_to_norm=read.shift,
                           scale_dacs_to_norm=read.scale)
        single = io_read.compute_per_base_metric("dwell_trimmean_trimsd", start_trim=1, end_trim=1)
        assert list(single) == ["dwell", "trimmean", "trimsd"]
        for k in names:
            assert np.array_equal(alone[k].view(np.uint8), want[k].view(np.uint8)), (i, k)
            assert np.array_equal(single[k].view(np.uint8), want[k].view(np.uint8)), (i, k)
        tm = io_read.compute_per_base_metric("dwell_trimmean", start_trim=1, end_trim=1)
        assert list(tm) == ["dwells", "trimmean"] and np.array_equal(tm["trimmean"].view(np.uint8), want["trimmean"].view(np.uint8))


# ---- site and k-mer levels ------------------------------------------------------------------------------------------------
from metric_cases import region_kmer_levels as _region_kmer_levels  # noqa: E402  (the numpy restatement of io.get_region_kmers)


@pytest.fixture(scope="module")
def site_reads():
    rng = np.random.default_rng(11)
    ctg_len = 300
    ref = rng.integers(0, 4, size=ctg_len)
    ref[140] = -1  # an N inside covered windows
    reads = []
    for i in range(40):
        rev = bool(i % 2)
        start = 7 * (i // 2) + (3 if rev else 0)
        n = 150 - (i // 2)  # coverage on a strand climbs to 20 and falls back to 0 before the contig ends
        fwd = ref[start : start + n]
        codes = np.where(fwd[::-1] >= 0, 3 - fwd[::-1], -1) if rev else fwd.copy()
        vals = rng.normal(size=n)
        vals[rng.random(n) < 0.05] = np.nan
        vals[rng.random(n) < 0.01] = np.inf
        if not rev and start <= 100 < start + n:
            vals[100 - start] = np.nan  # forward site 100: covered, every value NaN
        reads.append((rev, start, codes.astype(np.int8), vals))
    return ctg_len, reads


@pytest.mark.parametrize("min_cov", [1, 10, 41])
def test_site_and_kmer_levels_equal_the_numpy_restatement(torch_cuda, site_reads, min_cov):
    from remora_amd.engine import get_engine
    from remora_amd.metrics import SiteLevels, site_key0

    torch = torch_cuda
    ctg_len, reads = site_reads
    kb, ka = 1, 2
    want = _region_kmer_levels(reads, ctg_len, kb, ka, min_cov)
    eng = get_engine(0)
    acc = SiteLevels(eng, (kb, ka), min_cov)
    for part in (reads[:13], reads[13:]):  # two batches
        acc.add(torch.from_numpy(np.concatenate([r[3] for r in part])).to(eng.torch_device),
                torch.from_numpy(np.concatenate([r[2] for r in part])).to(eng.torch_device),
                site_key0(0, [2] * len(part), [r[0] for r in part], [r[1] for r in part], [r[2].size for r in part]),
                [r[2].size for r in part])
    levels, counts, site_kmer, site_level = acc.levels(want_sites=True)
    assert levels.shape == counts.shape == (256,)
    exp = np.array([np.median(want[i]) if i in want else np.nan for i in range(256)])
    assert np.array_equal(counts, [len(want.get(i, ())) for i in range(256)])
    assert np.array_equal(levels.view(np.uint64)[~np.isnan(exp)], exp.view(np.uint64)[~np.isnan(exp)])
    assert np.array_equal(np.isnan(levels), np.isnan(exp))
    assert np.array_equal(site_kmer, np.repeat(np.arange(256), counts))
    assert np.array_equal(site_level, np.concatenate([np.sort(want[i]) for i in sorted(want)]) if want else np.zeros(0))
    if min_cov == 41:
        assert np.isnan(levels).all() and not counts.any()
    else:
        assert np.isfinite(levels).sum() >= 8
    if min_cov == 1:  # what the data was built to hold
        fwd = [r for r in reads if not r[0]]
        cov = lambda p: sum(np.isfinite(r[3][p - r[1]]) for r in fwd if r[1] <= p < r[1] + r[2].size)  # noqa: E731
        covs = {cov(p) for p in range(ctg_len)}
        assert 0 in covs and any(c % 2 == 0 and c > 0 for c in covs) and any(c % 2 == 1 for c in covs)
        assert cov(100) == 0 and sum(r[1] <= 100 < r[1] + r[2].size for r in fwd) > 0


def test_kmers_longer_than_the_bound_are_refused(torch_cuda):
    from remora_amd import RemoraError
    from remora_amd.engine import get_engine
    from remora_amd.metrics import SiteLevels

    with pytest.raises(RemoraError):
        SiteLevels(get_engine(0), (4, 4), 1)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_estimate_kmer_levels_end_to_end(torch_cuda, tmp_path):
    """`analyze estimate_kmer_levels` on the 14 canonical reads of tests/golden/data against the per-read path
    (Read.set_refine_signal_mapping + Read.compute_per_base_metric read by read, then the numpy aggregation).  The data's
    coverage is at most 10 on one strand and 4 on the other, which leaves no k-mer observed at the default --min-coverage 10:
    the test runs at --min-coverage 3, where most of the 256 4-mers are."""
    from remora_amd import RemoraError
    from remora_amd import io as rio
    from remora_amd.__main__ import main
    from remora_amd.refine_signal_map import SigMapRefiner

    pod5, bam, table = (os.path.join(DATA, f) for f in ("can_reads.pod5", "can_mappings.bam", "levels_4mer.txt"))
    kb, ka, min_cov = 1, 2, 3
    outs = []
    for run in range(2):
        out = tmp_path / f"levels{run}.txt"
        assert main(["analyze", "estimate_kmer_levels", "--pod5-and-bam", pod5, bam, "--refine-kmer-level-table", table,
                     "--kmer-context-bases", str(kb), str(ka), "--min-coverage", str(min_cov), "--levels-filename", str(out)]) == 0
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]
    lines = outs[0].decode().splitlines()
    kmers = [ln.split("\t")[0] for ln in lines]
    assert len(lines) == 256 and kmers == sorted(kmers) and len(set(kmers)) == 256 and all(len(k) == 4 for k in kmers)
    got = np.array([float(ln.split("\t")[1]) for ln in lines])
    assert np.isfinite(got).sum() >= 8

    refiner = SigMapRefiner(kmer_model_filename=table, scale_iters=0, do_fix_guage=True, sd_params=[4, 3, 0.5])
    by_strand = {}
    for io_read, err in rio.iter_reads_from_pod5_and_bam(pod5, bam):
        if err is not None or io_read.ref_to_signal is None:
            continue
        try:
            io_read.set_refine_signal_mapping(refiner, ref_mapping=True)
        except RemoraError:  # a read the refiner rejects is left out, there as here
            continue
        tm = io_read.compute_per_base_metric("dwell_trimmean", start_trim=1, end_trim=1)["trimmean"]
        from remora_amd.util import seq_to_int

        by_strand.setdefault(io_read.ref_reg.ctg, []).append((io_read.ref_reg.strand == "-", io_read.ref_reg.start,
                                                              np.asarray(seq_to_int(io_read.ref_seq)), tm))
    assert by_strand
    want = {}
    for ctg, reads in by_strand.items():
        lo = min(r[1] for r in reads)
        reads = [(rev, start - lo, codes, tm) for rev, start, codes, tm in reads]
        span = max(r[1] + r[2].size for r in reads)
        for idx, lv in _region_kmer_levels(reads, span, kb, ka, min_cov).items():
            want.setdefault(idx, []).extend(lv)
    exp = np.array([np.median(want[i]) if i in want else np.nan for i in range(256)])
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.array_equal(got[np.isfinite(exp)], exp[np.isfinite(exp)])  # the file holds repr(float64): it reads back exactly
