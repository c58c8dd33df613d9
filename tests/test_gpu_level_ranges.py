"""k-mer levels in bounded device memory on the GPU: metrics.SiteLevels(max_resident_bases=...) over the ranges of
metrics.plan_level_ranges (rmr_site_medians per range, rmr_kmer_levels_from_sites over the lists) against the one pass
(rmr_site_kmer_levels) byte for byte and against a numpy restatement, and `analyze estimate_kmer_levels --levels-device-gib`
end to end."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DATA = os.path.join(GOLDEN, "data")
SHAPES = [((1, 2), 1), ((1, 2), 10), ((0, 0), 1), ((0, 0), 10)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


from metric_cases import region_kmer_levels as _region_kmer_levels  # noqa: E402  (the numpy restatement of io.get_region_kmers)


def _contig_reads(rng, n_reads, read_len, step, ctg_len, n_at, nan_at):
    """Reads of one contig in the style of test_gpu_metrics.site_reads: alternating strands, coverage that climbs and falls,
    NaN / inf values, an N in the reference, a forward site whose values are all NaN."""
    ref = rng.integers(0, 4, size=ctg_len)
    ref[n_at] = -1
    reads = []
    for i in range(n_reads):
        rev = bool(i % 2)
        start = step * (i // 2) + (3 if rev else 0)
        n = read_len - (i // 2)
        fwd = ref[start : start + n]
        assert fwd.size == n
        codes = np.where(fwd[::-1] >= 0, 3 - fwd[::-1], -1) if rev else fwd.copy()
        vals = rng.normal(size=n)
        vals[rng.random(n) < 0.05] = np.nan
        vals[rng.random(n) < 0.01] = np.inf
        if not rev and start <= nan_at < start + n:
            vals[nan_at - start] = np.nan
        reads.append((rev, start, codes.astype(np.int8), vals))
    return reads


class Observations:
    """Reads of several (sample, contig) pairs as SiteLevels takes them, in two batches resident on the device."""

    def __init__(self, torch, eng, groups, ctg_len):
        from remora_amd.metrics import site_key0

        self.groups, self.ctg_len, self.eng = groups, ctg_len, eng  # {(sample, contig): reads}
        rows = [(s, c) + r for (s, c), reads in groups.items() for r in reads]
        order = np.random.default_rng(3).permutation(len(rows))  # batches mix samples, contigs and strands
        rows = [rows[i] for i in order]
        self.key0 = np.concatenate([site_key0(s, [c], [rev], [start], [codes.size]) for s, c, rev, start, codes, _ in rows])
        self.lens = np.array([r[4].size for r in rows], np.int64)
        self.batches = []
        for part in (slice(0, len(rows) // 3), slice(len(rows) // 3, None)):
            self.batches.append((torch.from_numpy(np.concatenate([r[5] for r in rows[part]])).to(eng.torch_device),
                                 torch.from_numpy(np.concatenate([r[4] for r in rows[part]])).to(eng.torch_device),
                                 self.key0[part], self.lens[part]))
        self._one_shot, self._numpy = {}, {}

    def one_shot(self, kb_ka, min_cov):
        """levels, counts, site_kmer, site_level of the one pass; computed once per shape."""
        from remora_amd.metrics import SiteLevels

        if (kb_ka, min_cov) not in self._one_shot:
            acc = SiteLevels(self.eng, kb_ka, min_cov)
            for b in self.batches:
                acc.add(*b)
            self._one_shot[kb_ka, min_cov] = acc.levels(want_sites=True)
        return self._one_shot[kb_ka, min_cov]

    def restated(self, kb_ka, min_cov):
        if (kb_ka, min_cov) not in self._numpy:
            want = {}
            for reads in self.groups.values():
                for idx, lv in _region_kmer_levels(reads, self.ctg_len, kb_ka[0], kb_ka[1], min_cov).items():
                    want.setdefault(idx, []).extend(lv)
            self._numpy[kb_ka, min_cov] = want
        return self._numpy[kb_ka, min_cov]

    def ranged(self, kb_ka, min_cov, budget):
        """The same in ranges of at most `budget` resident bases.  -> (the four arrays, the SiteLevels)."""
        from remora_amd.metrics import SiteLevels, plan_level_ranges

        cuts = plan_level_ranges(self.key0, self.lens, budget, *kb_ka)
        acc = SiteLevels(self.eng, kb_ka, min_cov, max_resident_bases=budget)
        for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            acc.begin_range(a, b)
            for batch in self.batches:
                acc.add(*batch)
            acc.end_range()
        return acc.levels(want_sites=True), acc


def _same_bytes(got, want):
    assert len(got) == len(want) == 4
    for g, w, dt in zip(got, want, (np.float64, np.int64, np.int32, np.float64)):
        assert g.dtype == w.dtype == dt and g.shape == w.shape
        assert g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def obs(torch_cuda):
    """40 reads of about 150 bases on each of two samples x two contigs, both strands."""
    from remora_amd.engine import get_engine

    rng = np.random.default_rng(11)
    groups = {(s, c): _contig_reads(rng, 40, 150, 7, 300, 140, 100) for s in (0, 2) for c in (1, 6)}
    return Observations(torch_cuda, get_engine(0), groups, 300)


@pytest.fixture(scope="module")
def small_obs(torch_cuda):
    """12 reads of about 40 bases on one contig: few enough sites for a range per site."""
    from remora_amd.engine import get_engine

    return Observations(torch_cuda, get_engine(0), {(1, 4): _contig_reads(np.random.default_rng(12), 12, 40, 3, 70, 30, 20)}, 70)


@pytest.mark.parametrize("kb_ka,min_cov", SHAPES)
def test_ranges_give_the_bytes_of_the_one_pass(obs, kb_ka, min_cov):
    want = obs.one_shot(kb_ka, min_cov)
    total = int(obs.lens.sum())
    assert np.isfinite(want[0]).sum() >= (8 if kb_ka == (1, 2) else 4) and want[2].size == want[1].sum() > 0
    if min_cov == 1:  # the one pass itself against numpy
        exp = obs.restated(kb_ka, min_cov)
        nk = 4 ** (sum(kb_ka) + 1)
        assert np.array_equal(want[1], [len(exp.get(i, ())) for i in range(nk)])
        assert np.array_equal(want[3], np.concatenate([np.sort(exp[i]) for i in sorted(exp)]))
        assert np.array_equal(want[2], np.repeat(np.arange(nk), want[1]))
        med = np.array([np.median(exp[i]) if i in exp else np.nan for i in range(nk)])
        assert np.array_equal(want[0], med, equal_nan=True)
    for budget, n_ranges in ((total, 1), (total // 2 - 1, 3), (total // 7, None)):
        got, acc = obs.ranged(kb_ka, min_cov, budget)
        assert len(acc.range_sites) == n_ranges if n_ranges else len(acc.range_sites) >= 7
        _same_bytes(got, want)
        # every site is reported by exactly one range: a read that straddles a cut gives each of its bases to one of them
        assert sum(acc.range_sites) == acc.n_sites == want[2].size
        if n_ranges != 1:
            assert sum(1 for n in acc.range_sites if n) >= 2


def test_reads_straddle_the_cuts_and_margins_report_nothing(obs):
    """Where the cuts fall inside reads, and what a range alone reports: the sites of [a, b), none of the margins'."""
    from remora_amd.metrics import SiteLevels, plan_level_ranges, site_key0

    kb_ka, min_cov = (1, 2), 1
    total = int(obs.lens.sum())
    cuts = plan_level_ranges(obs.key0, obs.lens, total // 7, *kb_ka)
    inner = cuts[1:-1]
    inside = [(obs.key0 < c) & (obs.key0 + obs.lens > c) for c in inner.tolist()]
    assert sum(m.any() for m in inside) >= 5  # most cuts fall inside reads
    # range by range against the one pass over the reads clipped by hand to [a, b) with their margins
    a, b = int(cuts[2]), int(cuts[3])
    acc = SiteLevels(obs.eng, kb_ka, min_cov, max_resident_bases=total // 7)
    acc.begin_range(a, b)
    for batch in obs.batches:
        acc.add(*batch)
    held = sum(int(x.sum()) for x in acc._lens)
    assert held == int(np.clip(np.minimum(obs.key0 + obs.lens, b + 2) - np.maximum(obs.key0, a - 1), 0, None).sum()) <= total // 7
    n = acc.end_range()
    levels, counts, site_kmer, site_level = acc.levels(want_sites=True)
    assert n == counts.sum() == site_kmer.size and 0 < n <= b - a
    # the same sites from the numpy restatement, cut to the keys of [a, b)
    want = []
    for (s, c), reads in obs.groups.items():
        for rev in (False, True):
            origin =int(site_key0(s, [c], [rev], [0], [obs.ctg_len])[0])  # key of read-oriented offset 0
            k = sum(kb_ka) + 1
            mine = [r for r in reads if r[0] == rev]
            mat = np.full((len(mine), obs.ctg_len), np.nan)
            seq = np.full(obs.ctg_len + k - 1, -2, np.int64)
            for row, (_, start, codes, vals) in enumerate(mine):
                o0 = obs.ctg_len - (start + codes.size) if rev else start
                mat[row, o0 : o0 + codes.size] = vals
                seq[kb_ka[0] + o0 : kb_ka[0] + o0 + codes.size] = codes
            for offset in range(obs.ctg_len):
                if not a <= origin + offset < b or (seq[offset : offset + k] < 0).any():
                    continue
                site = mat[:, offset][np.isfinite(mat[:, offset])]
                if site.size >= min_cov:
                    want.append((int(sum(int(x) * 4 ** (k - 1 - j) for j, x in enumerate(seq[offset : offset + k]))), np.median(site)))
    want.sort()
    assert site_kmer.tolist() == [w[0] for w in want]
    assert site_level.tobytes() == np.array([w[1] for w in want]).tobytes()


def test_smallest_budget_gives_the_same_bytes_and_one_below_is_refused(small_obs):
    from remora_amd import RemoraError
    from remora_amd.metrics import LevelObservations, SiteLevels, plan_level_ranges

    o = small_obs
    for kb_ka in ((1, 2), (0, 0)):
        smallest, at = LevelObservations(o.key0, o.lens).largest_window(*kb_ka)
        cover = np.array([int(((o.key0 <= x) & (x < o.key0 + o.lens)).sum()) for x in range(at - kb_ka[0], at + kb_ka[1] + 1)])
        assert smallest == cover.sum() >= 4  # the fullest window of k sites: the largest pile x k, less where reads end inside it
        for min_cov in (1, 4):
            want = o.one_shot(kb_ka, min_cov)
            if kb_ka == (1, 2):
                got, acc = o.ranged(kb_ka, min_cov, smallest)
                assert len(acc.range_sites) > 15 and acc.n_kmer_groups >= 2
                _same_bytes(got, want)
            else:  # a range per site works; a 1-mer's sites then exceed what stage 2 may sort at once, which is said by name
                assert want[1].max() * 32 > smallest * 32
                with pytest.raises(RemoraError, match=r"k-mer [ACGT] \(index [0-3]\)"):
                    o.ranged(kb_ka, min_cov, smallest)
        o.eng.synchronize()
        o.eng.profile_enable(True)
        o.eng.profile_reset()
        try:
            with pytest.raises(RemoraError, match=f"needs room for {smallest} "):
                o.ranged(kb_ka, 1, smallest - 1)
            assert "site_kmer_levels" not in o.eng.profile()
            # (the slot does see these launches: a range that is run shows up in it)
            acc = SiteLevels(o.eng, kb_ka, 1, max_resident_bases=int(o.lens.sum()))
            cuts = plan_level_ranges(o.key0, o.lens, int(o.lens.sum()), *kb_ka)
            acc.begin_range(int(cuts[0]), int(cuts[1]))
            acc.add(*o.batches[0])
            acc.end_range()
            o.eng.synchronize()
            assert o.eng.profile()["site_kmer_levels"][1] >= 1
        finally:
            o.eng.profile_enable(False)


@pytest.mark.parametrize("kb_ka,min_cov", [((1, 2), 1), ((1, 2), 10)])
def test_kmer_groups_of_stage_two_give_the_same_bytes(obs, kb_ka, min_cov):
    """The budget bounds stage 2 as well: 32 bytes per site of sort buffers.  A budget under a third of the sites sorts the
    k-mers in at least 3 groups; the grouping shows in no output."""
    want = obs.one_shot(kb_ka, min_cov)
    n_sites = int(want[1].sum())
    budget = max(n_sites // 4, int(want[1].max()), 120)
    assert budget * 3 < n_sites  # so no 3 groups can hold the sites
    got, acc = obs.ranged(kb_ka, min_cov, budget)
    assert acc.n_kmer_groups >= 3 and len(acc.range_sites) >= 7
    _same_bytes(got, want)
    one, acc1 = obs.ranged(kb_ka, min_cov, int(obs.lens.sum()))
    assert acc1.n_kmer_groups == 1
    _same_bytes(one, want)


def test_range_protocol_is_checked(obs):
    from remora_amd import RemoraError
    from remora_amd.metrics import SiteLevels

    plain = SiteLevels(obs.eng, (1, 2), 1)
    with pytest.raises(RemoraError):
        plain.begin_range(0, 10)
    acc = SiteLevels(obs.eng, (1, 2), 1, max_resident_bases=100)
    with pytest.raises(RemoraError):
        acc.add(*obs.batches[0])  # no range begun
    acc.begin_range(int(obs.key0.min()), int(obs.key0.min()) + 200)
    with pytest.raises(RemoraError, match="planned for at most 100"):
        for batch in obs.batches:
            acc.add(*batch)


# ---- end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse_signal", [False, True])
def test_estimate_kmer_levels_in_ranges_writes_the_same_file(torch_cuda, tmp_path, reverse_signal):
    """`analyze estimate_kmer_levels` on the canonical reads of tests/golden/data: --levels-device-gib small enough for at
    least 3 ranges against the default (one range), byte for byte."""
    from remora_amd import io as rio
    from remora_amd.__main__ import main
    from remora_amd.metrics import LEVEL_BYTES_PER_BASE

    pod5, bam, table = (os.path.join(DATA, f) for f in ("can_reads.pod5", "can_mappings.bam", "levels_4mer.txt"))
    key0, span = rio.count_site_level_reads(bam)
    assert key0.size >= 10 and span.min() > 0
    gib = (int(span.sum()) // 2 - 1) * LEVEL_BYTES_PER_BASE / 2**30  # two ranges cannot hold the bases: three or more
    outs, ranges = [], []
    for name, extra in (("default", []), ("ranges", ["--levels-device-gib", repr(gib)])):
        out, log = tmp_path / f"{name}.txt", tmp_path / f"{name}.log"
        argv = ["analyze", "estimate_kmer_levels", "--pod5-and-bam", pod5, bam, "--refine-kmer-level-table", table, "--kmer-context-bases", "1", "2",
                "--min-coverage", "3", "--levels-filename", str(out), "--log-filename", str(log)] + extra
        assert main(argv + (["--reverse-signal"] if reverse_signal else [])) == 0
        outs.append(out.read_bytes())
        ranges.append(int(re.search(r"Aggregated in (\d+) ranges", log.read_text()).group(1)))
        assert re.search(r"k-mer levels aggregate in \S+ GiB of device memory \((\d+) bases at a time", log.read_text())
    assert ranges[0] == 1 and ranges[1] >= 3
    assert outs[0] == outs[1]
    levels = [ln.split("\t")[1] for ln in outs[0].decode().splitlines()]
    assert len(levels) == 256 and sum(lv != "nan" for lv in levels) >= 8


def test_get_site_kmer_levels_in_ranges(torch_cuda):
    from remora_amd import io as rio
    from remora_amd.refine_signal_map import SigMapRefiner

    pod5, bam, table = (os.path.join(DATA, f) for f in ("can_reads.pod5", "can_mappings.bam", "levels_4mer.txt"))
    refiner = SigMapRefiner(kmer_model_filename=table, scale_iters=0, do_fix_guage=True, sd_params=[4, 3, 0.5])
    want = rio.get_site_kmer_levels(pod5, bam, refiner, (1, 2), min_cov=3)
    _, span = rio.count_site_level_reads(bam)
    got = rio.get_site_kmer_levels(pod5, bam, refiner, (1, 2), min_cov=3, max_resident_bases=int(span.sum()) // 2 - 1)
    assert list(got) == list(want) and sum(v.size for v in want.values()) > 0
    for kmer in want:
        assert got[kmer].tobytes() == want[kmer].tobytes(), kmer
