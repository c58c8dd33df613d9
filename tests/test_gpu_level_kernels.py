"""The site and k-mer level kernels of csrc/k_metrics.hip at every k-mer length from 1 to RMR_MAX_LEVEL_KMER and every split of
the context, on the values that decide the sort key (both zeros, mixed signs, ties, subnormals, large magnitudes, min_cov met
exactly), with empty reads in the batches, and the counting kernel on both of its routes (LDS counters up to 4096 k-mers, global
atomics above) with more sites than its capped grid covers in one trip.  One pass (rmr_site_kmer_levels) against numpy, the
ranged path (rmr_site_medians, rmr_kmer_levels_from_sites) against the one pass byte for byte."""
import ctypes

import numpy as np
import pytest

import metric_cases as mc
from test_gpu_level_ranges import Observations, _same_bytes

pytestmark = pytest.mark.gpu

SEED = 20
GRID_SITES = 1024 * 256  # sites one trip of kmer_count_kernel's capped grid covers


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class _Batches(Observations):
    """Reads of one (sample, contig) in two batches whose order is given (`batches`: indices into `reads`), empty reads included."""

    def __init__(self, torch, eng, reads, batches, ctg_len, sample=1, contig=4):
        from remora_amd.metrics import site_key0

        self.groups, self.ctg_len, self.eng = {(sample, contig): reads}, ctg_len, eng
        key0 = np.concatenate([site_key0(sample, [contig], [r[0]], [r[1]], [r[2].size]) for r in reads])
        lens = np.array([r[2].size for r in reads], np.int64)
        order = batches[0] + batches[1]
        self.key0, self.lens = key0[order], lens[order]
        self.batches = [(torch.from_numpy(np.concatenate([reads[j][3] for j in part]).astype(np.float64)).to(eng.torch_device),
                         torch.from_numpy(np.concatenate([reads[j][2] for j in part]).astype(np.int8)).to(eng.torch_device),
                         key0[part], lens[part]) for part in batches]
        self._one_shot, self._numpy = {}, {}


def _splits(k):
    return sorted({(0, k - 1), (k - 1, 0), ((k - 1) // 2, k - 1 - (k - 1) // 2)})


def _equals_numpy(got, exp, nk):
    """The comparison of test_gpu_level_ranges.test_ranges_give_the_bytes_of_the_one_pass: equality, NaN in the same places."""
    levels, counts, site_kmer, site_level = got
    assert np.array_equal(counts, [len(exp.get(i, ())) for i in range(nk)])
    assert np.array_equal(site_level, np.concatenate([np.sort(exp[i]) for i in sorted(exp)]))
    assert np.array_equal(site_kmer, np.repeat(np.arange(nk), counts))
    assert np.array_equal(levels, np.array([np.median(exp[i]) if i in exp else np.nan for i in range(nk)]), equal_nan=True)


# ---- 1. every k-mer length ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_every_kmer_length_and_split(torch_cuda, k):
    """k = 5 with (2, 2) is the command's default; k = 6 is the last table the counting kernel keeps in LDS, 7 and 8 count with
    global atomics; k = 8 takes 65 536-entry tables, a 16-bit second sort in stage 2 and windows across seven neighbours."""
    from remora_amd.engine import get_engine

    reads, batches = mc.kmer_reads(SEED, k)
    obs = _Batches(torch_cuda, get_engine(0), reads, batches, mc.CTG_LEN)
    total = int(obs.lens.sum())
    assert (obs.lens == 0).sum() == 8 and obs.lens[0] == obs.lens[-1] == 0
    splits = _splits(k)
    assert k != 5 or (2, 2) in splits
    for kb_ka in splits:
        for min_cov in (1, 3):
            want = obs.one_shot(kb_ka, min_cov)
            _equals_numpy(want, obs.restated(kb_ka, min_cov), 4**k)
            assert want[2].size == want[1].sum() >= 20
            for budget, least in ((total // 3, 3), (total // 7, 7)):
                got, acc = obs.ranged(kb_ka, min_cov, budget)
                assert len(acc.range_sites) >= least and sum(acc.range_sites) == acc.n_sites == want[2].size
                _same_bytes(got, want)
                if k >= 6 and budget == total // 7:
                    assert acc.n_kmer_groups >= 2


# ---- 2. medians and the sort key ------------------------------------------------------------------------------------------------------------
def test_median_and_key_edges(torch_cuda):
    """Hand-made sites at k = 1 (mc.median_edge_sites), every observation a read of one base.  The kernel gives both zeros one
    key and turns a median of -0.0 into +0.0 (sortable_f64 adds 0.0), numpy may keep the sign: the comparison is on values."""
    from remora_amd.engine import get_engine

    cases = mc.median_edge_sites()
    reads = [(False, 10 + s, np.array([base], np.int8), np.array([v])) for s, (_, base, vals, _) in enumerate(cases) for v in vals]
    order = np.random.default_rng(4).permutation(len(reads)).tolist()
    obs = _Batches(torch_cuda, get_engine(0), reads, [order[:20], order[20:]], 10 + len(cases))
    by_name = {c[0]: s for s, c in enumerate(cases)}
    for min_cov in (1, mc.MEDIAN_MIN_COV):
        want = mc.median_sites_expected(cases, min_cov)
        got = obs.one_shot((0, 0), min_cov)
        assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        assert got[3].dtype == np.float64 and got[2].dtype == np.int32
        _equals_numpy(got, obs.restated((0, 0), min_cov), 4)
        for b in range(4):  # ascending inside each k-mer, across the sign change and the subnormals
            assert (np.diff(got[3][got[2] == b]) >= 0).all()
        zeros = got[3][got[2] == 0]
        assert (zeros == 0.0).sum() == (3 if min_cov == 1 else 0)  # both zeros; zeros with a subnormal; -1e300 with 1e300
        ranged, acc = obs.ranged((0, 0), min_cov, 12)
        assert len(acc.range_sites) >= 5
        _same_bytes(ranged, got)
        # who is absent: the site of NaN only always, the twin with min_cov - 1 finite values under min_cov
        n_sites = sum(1 for c in cases if np.isfinite(c[2]).sum() >= max(1, min_cov))
        assert got[2].size == n_sites and n_sites == (len(cases) - 1 if min_cov == 1 else sum(np.isfinite(c[2]).sum() >= min_cov for c in cases))
    exact, twin = cases[by_name["exactly min_cov finite values"]], cases[by_name["min_cov - 1 finite values"]]
    with_cov = obs.one_shot((0, 0), mc.MEDIAN_MIN_COV)
    assert exact[3] in with_cov[3][with_cov[2] == exact[1]] and twin[3] not in with_cov[3][with_cov[2] == twin[1]]
    assert twin[3] in obs.one_shot((0, 0), 1)[3][obs.one_shot((0, 0), 1)[2] == twin[1]]


# ---- 3. the counting kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb_ka", [(2, 3), (3, 4)], ids=["k6_lds", "k8_global"])
def test_counting_routes_and_the_capped_grid(torch_cuda, kb_ka):
    """One read long enough for one rmr_site_medians call to append more than 1024 x 256 sites: kmer_count_kernel's grid is capped
    there, so its threads take a second trip.  k = 6 counts in LDS, k = 8 with global atomics."""
    from remora_amd.engine import get_engine
    from remora_amd.metrics import SiteLevels

    torch, eng = torch_cuda, get_engine(0)
    k = sum(kb_ka) + 1
    n = GRID_SITES + 300 + k - 1
    codes, vals = mc.long_read(n, k, SEED)
    kmer, level = mc.long_read_expected(codes, vals, *kb_ka)
    assert kmer.size == GRID_SITES + 300
    d_vals, d_codes = torch.from_numpy(vals).to(eng.torch_device), torch.from_numpy(codes).to(eng.torch_device)
    batch = (d_vals, d_codes, np.zeros(1, np.int64), np.array([n], np.int64))
    nk = 4**k
    order = np.lexsort((level, kmer))
    want_counts = np.bincount(kmer, minlength=nk)
    cuts = np.concatenate([[0], np.cumsum(want_counts)])
    by_level = level[order]
    want_levels = np.array([np.median(by_level[a:b]) if b > a else np.nan for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist())])

    acc = SiteLevels(eng, kb_ka, 1, max_resident_bases=n)
    acc.begin_range(0, n)
    acc.add(*batch)
    assert acc.end_range() == kmer.size > GRID_SITES
    assert np.array_equal(acc._site_counts.cpu().numpy(), want_counts)
    one_range = acc.levels(want_sites=True)
    assert np.array_equal(one_range[1], want_counts) and one_range[1].sum() == kmer.size
    assert np.array_equal(one_range[0], want_levels, equal_nan=True)
    assert np.array_equal(one_range[2], kmer[order]) and np.array_equal(one_range[3], by_level)

    # two calls on two halves of the key range, into the same lists and counts
    half = n // 2
    acc = SiteLevels(eng, kb_ka, 1, max_resident_bases=n)
    acc.begin_range(0, half)
    acc.add(*batch)
    assert acc.end_range() == half - kb_ka[0]
    first = np.bincount(kmer[: half - kb_ka[0]], minlength=nk)
    assert np.array_equal(acc._site_counts.cpu().numpy(), first)
    acc.begin_range(half, n)
    acc.add(*batch)
    assert acc.end_range() == kmer.size - (half - kb_ka[0])
    assert np.array_equal(acc._site_counts.cpu().numpy(), want_counts) and (want_counts > first).any() and first.any()  # incremented
    _same_bytes(acc.levels(want_sites=True), one_range)
    one_pass = SiteLevels(eng, kb_ka, 1)
    one_pass.add(*batch)
    _same_bytes(one_pass.levels(want_sites=True), one_range)


# ---- 4. list capacity -------------------------------------------------------------------------------------------------------------------------
def test_a_list_one_entry_short_is_refused_by_both_numbers(torch_cuda):
    from remora_amd import RemoraError
    from remora_amd import _lib as L
    from remora_amd.engine import get_engine

    torch, eng = torch_cuda, get_engine(0)
    dev = eng.torch_device
    kb, ka, n = 1, 1, 500
    codes, vals = mc.long_read(n, 3, SEED)
    kmer, level = mc.long_read_expected(codes, vals, kb, ka)
    sites = kmer.size
    d_vals, d_codes = torch.from_numpy(vals).to(dev), torch.from_numpy(codes).to(dev)
    d_off, d_key0 = torch.tensor([0, n], dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    before = np.arange(64, dtype=np.int64) * 3 + 1

    def call(capacity):
        list_kmer = torch.full((sites,), -5, dtype=torch.int32, device=dev)
        list_level = torch.full((sites,), -7.25, dtype=torch.float64, device=dev)
        counts = torch.from_numpy(before).to(dev)
        took = ctypes.c_int64(-1)
        torch.cuda.current_stream(dev).synchronize()
        rc = L.lib().rmr_site_medians(eng.handle, 1, d_off.data_ptr(), d_key0.data_ptr(), n, d_vals.data_ptr(), d_codes.data_ptr(), kb, ka, 1, 0, n,
                                      list_kmer.data_ptr(), list_level.data_ptr(), 0, capacity, counts.data_ptr(), ctypes.byref(took))
        return rc, took.value, list_kmer.cpu().numpy(), list_level.cpu().numpy(), counts.cpu().numpy()

    rc, took, list_kmer, list_level, counts = call(sites - 1)
    assert rc != 0
    with pytest.raises(RemoraError, match=f"the range reports {sites} sites, the lists have room for {sites - 1}"):
        L.check(rc)
    assert list_kmer[sites - 1] == -5 and list_level[sites - 1] == -7.25  # the entry at list_capacity
    assert np.array_equal(counts, before) and took == 0
    rc, took, list_kmer, list_level, counts = call(sites)
    assert rc == 0 and took == sites
    assert np.array_equal(counts, before + np.bincount(kmer, minlength=64))
    got, want = np.lexsort((list_level, list_kmer)), np.lexsort((level, kmer))
    assert np.array_equal(list_kmer[got], kmer[want]) and np.array_equal(list_level[got], level[want])
