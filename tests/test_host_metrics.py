"""CPU-only checks of the per-base metrics feature: the golden fixture (tests/golden/base_metrics.npz, written by
tools/gen_golden_metrics.py from the reference's remora.metrics) is well-formed and covers the shapes it is there for,
METRIC_FUNCS carries the reference's names and returned keys, the host form of the metrics agrees with the fixture, and the
command line accepts the reference's argument set."""
import json
import math

import numpy as np
import pytest

from conftest import golden
from metrics_exact import N_READS, U, cases, mean_bound, read_signal, var_bound


@pytest.fixture(scope="module")
def fx():
    return golden("base_metrics.npz")


def test_fixture_is_well_formed_and_covers_the_edge_shapes(fx):
    trims = fx["trims"]
    assert trims.tolist() == [[1, 1], [2, 2], [0, 0], [6000, 6000]]
    assert fx["shift"].shape == fx["scale"].shape == (N_READS,)
    n_bases, all_dwells = [], []
    for i in range(N_READS):
        dacs, m = fx[f"r{i}_dacs"], fx[f"r{i}_map"]
        assert dacs.dtype == np.int16 and m.dtype == np.int64
        assert m[0] >= 0 and m[-1] <= dacs.size and (np.diff(m) >= 0).all()
        nb = m.size - 1
        n_bases.append(nb)
        assert fx[f"r{i}_dwell"].dtype == np.float32 and np.array_equal(fx[f"r{i}_dwell"], np.diff(m).astype(np.float32))
        all_dwells.append(np.diff(m))
        for name in ("mean", "sd"):
            assert fx[f"r{i}_{name}"].shape == (nb,) and fx[f"r{i}_{name}"].dtype == np.float64
            assert np.array_equal(np.isnan(fx[f"r{i}_{name}"]), np.diff(m) == 0)  # a zero dwell is NaN, never inf
        for t, (st, en) in enumerate(trims.tolist()):
            for name in ("trimmean", "trimsd"):
                v = fx[f"r{i}_t{t}_{name}"]
                assert v.shape == (nb,) and not np.isinf(v).any()
                assert np.array_equal(np.isnan(v), np.maximum(0, np.diff(m) - st - en) == 0)
        assert np.isnan(fx[f"r{i}_t3_trimmean"]).all()  # the trim larger than every dwell
    assert sorted(n_bases)[:4] == [1, 1, 18, 63] and {64, 65, 4097, 130} <= set(n_bases)
    assert fx["r5_dacs"].size == 1  # the read whose whole signal is one sample
    assert {0, 1, 2, 3, 5000} <= set(all_dwells[6].tolist())
    assert fx["r7_map"][0] > 0 and fx["r7_map"][-1] < fx["r7_dacs"].size  # exercises the clip


def test_metric_funcs_have_the_reference_names_and_keys(fx):
    from remora_amd import metrics

    keys = json.loads(bytes(fx["returned_keys"]).decode())
    assert list(metrics.METRIC_FUNCS) == ["dwell", "dwell_mean", "dwell_mean_sd", "dwell_trimmean", "dwell_trimmean_trimsd"]
    assert keys["dwell_trimmean"] == ["dwells", "trimmean"]  # the reference's quirk
    i = 7
    sig = (fx[f"r{i}_dacs"] - float(fx["shift"][i])) / float(fx["scale"][i])
    for name, func in metrics.METRIC_FUNCS.items():
        got = func(sig, fx[f"r{i}_map"], start_trim=2, end_trim=2)
        assert list(got) == keys[name], name
        assert [k for k, _ in metrics.METRIC_KEYS[name]] == keys[name], name  # the batch form returns the same keys


def test_host_metric_funcs_agree_with_the_fixture_to_the_cumsum_rounding(fx):
    """The host form sums every base directly; the reference's values carry the rounding of a whole-read cumulative sum: a
    prefix of N samples is off by at most N u sum|x| (u = 2^-53), a difference of two prefixes by twice that."""
    from remora_amd import metrics

    for i in range(N_READS):
        m = fx[f"r{i}_map"]
        sig = (fx[f"r{i}_dacs"] - float(fx["shift"][i])) / float(fx["scale"][i])
        clipped = sig[m[0] : m[-1]]
        slack = 2 * clipped.size * U * float(np.abs(clipped).sum())
        got = metrics.compute_dwell_mean_sd(sig, m)
        assert np.array_equal(got["dwell"], fx[f"r{i}_dwell"])
        assert np.array_equal(np.isnan(got["mean"]), np.isnan(fx[f"r{i}_mean"]))
        ok = ~np.isnan(got["mean"])
        assert (np.abs(got["mean"] - fx[f"r{i}_mean"])[ok] <= (slack / got["dwell"][ok]) + 4 * U * np.abs(got["mean"][ok])).all()
        for t, (st, en) in enumerate(fx["trims"].tolist()):
            tm = metrics.compute_trimmean(sig, m, start_trim=st, end_trim=en)["trimmean"]
            ref = fx[f"r{i}_t{t}_trimmean"]
            assert np.array_equal(np.isnan(tm), np.isnan(ref))
            ok = ~np.isnan(tm)
            eff = np.maximum(0, np.diff(m) - st - en)[ok]
            assert (np.abs(tm - ref)[ok] <= slack / eff + 4 * U * np.abs(tm[ok])).all()


def test_the_reference_alone_meets_the_gpu_tests_inequalities(fx):
    """What tests/test_gpu_metrics.py leans on, for every read, trim and all four quantities, with that test's own bounds
    (tests/metrics_exact.py).  Its second inequality is |value - ref| <= |ref - exact| + bound:
      - with a value that has no error of its own (value = exact) it reads |ref - exact| <= |ref - exact|; what can fail on
        the fixture is that `ref` and `exact` are not of the same inputs, so the reference's own error is asserted to stay
        inside the bound of ITS summation: the same two expressions with the N samples and the sums of the whole clipped read
        in place of the base's, since the reference differences a cumulative sum over the read (two prefixes: x2);
      - with the host's direct sums (METRIC_FUNCS here, numpy) as the value, both inequalities must hold as they must on the GPU."""
    from remora_amd import metrics

    worst = {"ref_mean": 0.0, "ref_var": 0.0, "host_mean": 0.0, "host_var": 0.0}
    host = {}
    for case in cases(fx):
        i, t, st, en, mname, sname, ref_m, ref_s = (case[k] for k in ("read", "trim", "st", "en", "mean_name", "sd_name", "ref_mean", "ref_sd"))
        m, sig = fx[f"r{i}_map"], read_signal(fx, i)
        clipped = sig[m[0] : m[-1]].tolist()
        N, SABS, SSQ = len(clipped), math.fsum(abs(v) for v in clipped), math.fsum(v * v for v in clipped)
        if (i, st, en) not in host:
            host[i, st, en] = metrics.compute_trimmean_trimsd(sig, m, start_trim=st, end_trim=en)
        h_m, h_s = host[i, st, en]["trimmean"], host[i, st, en]["trimsd"]
        assert np.array_equal(np.isnan(h_m), np.isnan(ref_m)) and np.array_equal(np.isnan(h_s), np.isnan(ref_s)), (i, t, mname)
        for base, n, mean, var, sabs, ssq in case["bases"]:
            rm, rv = abs(ref_m[base] - mean), abs(ref_s[base] ** 2 - var)
            ref_bm = 2 * mean_bound(N, SABS) * N / n
            ref_bv = 2 * (2 * N * U * SSQ / n) + 2 * abs(mean) * ref_bm + ref_bm**2 + 8 * U * (ssq / n + mean * mean)
            worst["ref_mean"], worst["ref_var"] = max(worst["ref_mean"], rm / ref_bm), max(worst["ref_var"], rv / ref_bv)
            assert rm <= ref_bm, (i, t, mname, base, rm, ref_bm)
            assert rv <= ref_bv, (i, t, sname, base, rv, ref_bv)
            bm, bv = mean_bound(n, sabs), var_bound(n, ssq, mean)
            em, ev = abs(h_m[base] - mean), abs(h_s[base] ** 2 - var)
            worst["host_mean"], worst["host_var"] = max(worst["host_mean"], em / bm), max(worst["host_var"], ev / bv)
            assert em <= bm and abs(h_m[base] - ref_m[base]) <= rm + bm, (i, t, mname, base, em, bm)
            assert ev <= bv and abs(h_s[base] ** 2 - ref_s[base] ** 2) <= rv + bv, (i, t, sname, base, ev, bv)
    print("worst error / bound:", worst)


def test_cli_parser_accepts_the_reference_argument_set(tmp_path):
    from remora_amd.__main__ import build_parser

    args = build_parser().parse_args([
        "analyze", "estimate_kmer_levels", "--pod5-and-bam", "a.pod5", "a.bam", "--pod5-and-bam", "b.pod5", "b.bam",
        "--refine-kmer-level-table", "levels.txt", "--refine-rough-rescale", "--refine-scale-iters", "0",
        "--refine-half-bandwidth", "7", "--refine-algo", "Viterbi", "--refine-short-dwell-parameters", "4", "3", "0.5",
        "--min-coverage", "5", "--kmer-context-bases", "1", "2", "--levels-filename", str(tmp_path / "out.txt"),
        "--log-filename", str(tmp_path / "log.txt"), "--num-workers", "4", "--chunk-width", "500", "--max-chunk-coverage", "50",
        "--device", "0"])
    assert args.pod5_and_bam == [["a.pod5", "a.bam"], ["b.pod5", "b.bam"]]
    assert args.kmer_context_bases == [1, 2] and args.min_coverage == 5 and args.refine_algo == "Viterbi"
    d = build_parser().parse_args(["analyze", "estimate_kmer_levels", "--pod5-and-bam", "a", "b"])
    assert (d.min_coverage, tuple(d.kmer_context_bases), d.refine_scale_iters, d.refine_half_bandwidth, d.refine_algo,
            d.levels_filename, d.chunk_width, d.max_chunk_coverage, d.num_workers) == (
        10, (2, 2), 0, 5, "dwell_penalty", "remora_kmer_levels.txt", 1000, 100, 1)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["analyze", "estimate_kmer_levels"])


def test_site_keys_keep_samples_and_contigs_apart_or_refuse():
    """Every (sample, contig, strand) has a key range of its own, also for contig indices of 512 and more beside a second
    pod5/BAM pair (GRCh38 with alts has ~3,000 contigs, a transcriptome 100,000 and more); what does not fit is refused."""
    from remora_amd import RemoraError
    from remora_amd.metrics import MAX_LEVEL_CONTIGS, MAX_LEVEL_SAMPLES, MAX_LEVEL_KMER, site_key0

    span = 1 << 34
    seen = {}
    contigs = [0, 1, 511, 512, 513, 1023, 1024, 3000, 200_000, MAX_LEVEL_CONTIGS - 1]
    for sample in (0, 1, 2, MAX_LEVEL_SAMPLES - 1):
        for rev in (False, True):
            lo = site_key0(sample, contigs, [rev] * len(contigs), [0] * len(contigs), [1] * len(contigs))  # first base on position 0
            hi = site_key0(sample, contigs, [rev] * len(contigs), [(1 << 31) - 2] * len(contigs), [1] * len(contigs))
            for c, a, b in zip(contigs, lo.tolist(), hi.tolist()):
                assert a >= 0 and b >= 0 and abs(a - b) == (1 << 31) - 2
                assert a // span == b // span and (a // span) not in seen, (sample, c, rev, seen.get(a // span))
                seen[a // span] = (sample, c, rev)
                # a k-mer window never reaches from one range into the next
                assert max(a, b) % span + 2 * MAX_LEVEL_KMER < span
    assert len(seen) == 4 * 2 * len(contigs)
    # the collision the narrower packing had: sample s, contig c + 512 against sample s + 1, contig c
    assert site_key0(0, [512 + 7], [False], [100], [50])[0] != site_key0(1, [7], [False], [100], [50])[0]
    for bad in (dict(sample=MAX_LEVEL_SAMPLES, ref_id=[0]), dict(sample=-1, ref_id=[0]), dict(sample=0, ref_id=[MAX_LEVEL_CONTIGS]),
                dict(sample=0, ref_id=[-1]), dict(sample=0, ref_id=[0], ref_start=[(1 << 32) - 10])):
        kw = dict(sample=0, ref_id=[0], is_reverse=[False], ref_start=[100], ref_len=[50])
        kw.update(bad)
        with pytest.raises(RemoraError):
            site_key0(**kw)


def test_site_keys_step_by_one_in_read_orientation():
    from remora_amd.metrics import site_key0

    k = site_key0(0, [3, 3, 4], [False, True, True], [100, 100, 100], [50, 50, 50])
    # forward: first base on position 100; reverse: first base (read orientation) on position 149, the next on 148
    assert k[0] & ((1 << 34) - 1) == 100
    assert k[1] & ((1 << 34) - 1) == (1 << 32) - 1 - 149
    assert len({int(x) >> 34 for x in k}) == 3  # contig and strand keep the sites apart
    assert site_key0(1, [3], [False], [100], [50])[0] != k[0]
