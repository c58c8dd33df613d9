"""CPU-only: the generators and numpy restatements of tests/metric_cases.py are what they claim, so that the GPU tests built on
them (tests/test_gpu_region_kernels.py, tests/test_gpu_level_kernels.py) hold no case that numpy alone does not settle."""
import numpy as np
import pytest

import metric_cases as mc
from conftest import golden
from metrics_exact import N_READS, cases

SEED = 20


@pytest.fixture(scope="module")
def synth():
    return mc.synthetic_reads(SEED)


# ---- 1. the restatements ------------------------------------------------------------------------------------------------------
def test_per_base_exact_gives_the_base_lists_of_the_golden_cases():
    fx = golden("base_metrics.npz")
    seen = 0
    for case in cases(fx):
        i = case["read"]
        read = (fx[f"r{i}_dacs"], fx[f"r{i}_map"], float(fx["shift"][i]), float(fx["scale"][i]))
        dwell, bases = mc.per_base_exact(read, case["st"], case["en"])
        assert dwell.dtype == np.float32 and np.array_equal(dwell, fx[f"r{i}_dwell"])
        assert bases == case["bases"], (i, case["trim"], case["mean_name"])
        seen += len(bases)
    assert seen > 10000 and {c["read"] for c in cases(fx)} == set(range(N_READS))


def test_region_rows_expected_reproduces_golden_rows():
    """The reference's rows of region a_rev in read orientation, taken as whole per-base arrays of the covered bases, placed
    flipped with their lead: the reference's rows in reference orientation (NaN pattern, dwell, and the mean's bits)."""
    fx = golden("region_metrics.npz")
    read_rows, ref_rows = (fx[f"m_a_rev_can_dwell_mean_sd_{o}_s0_dwell"] for o in ("read", "ref"))
    assert fx["m_a_rev_can_dwell_mean_sd_read_s0_ids"].tolist() == fx["m_a_rev_can_dwell_mean_sd_ref_s0_ids"].tolist()
    n_rows, rlen = read_rows.shape
    leads = [int(np.nonzero(~np.isnan(r))[0][0]) for r in read_rows]
    assert max(leads) > 0 and min(leads) == 0  # a read that covers the region partly, and one that covers it all
    for key in ("dwell", "mean", "sd"):
        src, want = (fx[f"m_a_rev_can_dwell_mean_sd_{o}_s0_{key}"] for o in ("read", "ref"))
        per_base = [src[r, leads[r] :] for r in range(n_rows)]
        pairs = [[r, 0, rlen - leads[r], leads[r], n_rows - 1 - r, rlen, 1] for r in range(n_rows)]
        got = mc.region_rows_expected(per_base, pairs, n_rows + 1, rlen + 2)
        assert np.isnan(got[n_rows]).all() and np.isnan(got[:, rlen:]).all()
        assert np.array_equal(got[:n_rows, :rlen][::-1].view(np.uint64), np.asarray(want, np.float64).view(np.uint64)), key
    # forward and in place: lead 0, no flip
    got = mc.region_rows_expected([np.arange(10.0)], [[0, 2, 5, 1, 0, 6, 0]], 1, 7)
    assert np.array_equal(got, [[np.nan, 2.0, 3.0, 4.0, np.nan, np.nan, np.nan]], equal_nan=True)


def test_long_read_expectation_equals_the_region_restatement():
    for kb, ka in ((0, 0), (2, 2), (0, 5), (7, 0)):
        k = kb + ka + 1
        codes, vals = mc.long_read(300, k, 3)
        assert codes.min() == 0 and codes.max() == 3 and np.unique(vals).size == 300 and np.isfinite(vals).all()
        assert (vals < 0).any() and (vals > 0).any()
        kmer, level = mc.long_read_expected(codes, vals, kb, ka)
        assert kmer.size == level.size == 300 - k + 1
        want = mc.region_kmer_levels([(False, 0, codes, vals)], 300, kb, ka, 1)
        got = {}
        for m, lv in zip(kmer.tolist(), level.tolist()):
            got.setdefault(m, []).append(lv)
        assert got == want


# ---- 2. the inputs --------------------------------------------------------------------------------------------------------------
def test_synthetic_reads_are_what_they_claim(synth):
    reads, twins = synth
    assert [r[1].size - 1 for r in reads] == list(mc.READ_BASES) and {1, 63, 64, 65, 256, 257, 320} < set(mc.READ_BASES)
    dwells_seen = set()
    for i, (dacs, mp, shift, scale) in enumerate(reads):
        assert dacs.dtype == np.int16 and mp.dtype == np.int64 and scale > 0
        dw = np.diff(mp)
        assert dw.min() >= 0 and mp[0] >= 0 and mp[-1] <= dacs.size
        dwells_seen |= set(dw.tolist())
        for z in mc.ZERO_DWELL_BASES:
            if z < dw.size and (i, z) != (mc.LONG_BASE_READ, mc.LONG_BASE):
                assert dw[z] == 0, (i, z)
        if dacs.size >= 2:
            assert dacs.min() == -32768 and dacs.max() == 32767
        assert dw.max() <= 12 or i == mc.LONG_BASE_READ
    assert set(range(13)) <= dwells_seen
    dw = np.diff(reads[mc.LONG_BASE_READ][1])
    assert dw.size == 320 and dw[mc.LONG_BASE] == 5000 and np.delete(dw, mc.LONG_BASE).max() <= 12
    dacs, mp, _, _ = reads[mc.PADDED_READ]
    assert mp[0] == mc.PAD_LEAD and dacs.size - mp[-1] == mc.PAD_TAIL
    for j in (mc.ENDS_TWIN_OF, mc.BACK_TWIN_OF):
        assert reads[j][1][0] == 0 and reads[j][1][-1] == reads[j][0].size
    # the twins: only the named entries differ
    assert [t[0] for t in twins] == [mc.ENDS_TWIN_OF, mc.BACK_TWIN_OF]
    for of, (dacs, mp, shift, scale), changed in twins:
        c_dacs, c_mp, c_shift, c_scale = reads[of]
        assert np.array_equal(dacs, c_dacs) and (shift, scale) == (c_shift, c_scale) and mp.shape == c_mp.shape
        assert np.nonzero(mp != c_mp)[0].tolist() == sorted(changed)
    ends, back = twins[0][1][1], twins[1][1][1]
    assert ends[0] == -3 and ends[-1] == twins[0][1][0].size + 5
    j = mc.BACK_AT
    assert 0 < j and j + 3 < back.size and np.diff(back)[j : j + 2].tolist() == [-2 - int(back[j]), -2] and back[j] > 0
    assert (np.diff(back)[[j, j + 1]] < 0).all() and back[j + 2] < 0  # backwards across two bases, and back from outside the signal
    # what the exact statistics see of the twins: the bases a changed entry bounds have none, every other base the clean read's
    for of, dirty, changed in twins:
        clean_list = {b[0]: b for b in mc.per_base_exact(reads[of], 0, 0)[1]}
        dirty_list = {b[0]: b for b in mc.per_base_exact(dirty, 0, 0)[1]}
        touched = {b for e in changed for b in (e - 1, e) if 0 <= b < dirty[1].size - 1}
        assert not touched & set(dirty_list) and dirty_list == {b: v for b, v in clean_list.items() if b not in touched}


def test_region_pairs_cover_every_listed_combination(synth):
    reads, _ = synth
    pairs, rows, width = mc.region_pairs(reads)
    read, first, last, lead, row, rlen, flip = pairs.T
    nb = np.array([r[1].size - 1 for r in reads])
    n = last - first
    assert (first >= 0).all() and (n > 0).all() and (last <= nb[read]).all() and (lead >= 0).all() and (lead + n <= rlen).all()
    assert rows == len(pairs) and sorted(row.tolist()) == list(range(rows)) and row.tolist() != sorted(row.tolist())
    assert width > rlen.max()
    have = set(zip(first.tolist(), n.tolist()))
    assert {(f, s) for f in mc.FIRSTS for s in mc.SPANS} <= have and {(63, 66), (63, 258), (127, 258)} <= have
    assert set(flip.tolist()) == {0, 1}
    for fl in (0, 1):  # every kind of lead and of region length, forward and flipped
        m = flip == fl
        spare = rlen[m] - n[m]
        assert (spare == 0).any() and ((spare > 1) & (lead[m] == 0)).any() and ((spare > 1) & (lead[m] == 1)).any()
        assert ((spare > 1) & (lead[m] == spare)).any()
    groups = np.array([mc.groups_touched(f, la) for f, la in zip(first.tolist(), last.tolist())])
    assert {1, 2, 3, 5, 6} <= set(groups.tolist()) and groups.max() >= 9
    bound = (n + 62) // 64 + 1
    assert (groups <= bound).all() and (groups == bound).any()
    for s in (66, 258):  # the worst case of the bound: 3 and 6 groups
        m = (first % 64 == 63) & (n == s)
        assert m.any() and (groups[m] == bound[m]).all() and set(bound[m].tolist()) == {(s + 62) // 64 + 1}
    # a fifth group that (n + 62) / 64 alone would not launch, and blockIdx.y of 1 and 2 in a launch of the pair alone
    assert ((groups == 5) & ((n + 62) // 64 == 4)).any()
    assert {2, 3} <= set(((bound + 3) // 4).tolist()) and ((n == 513) & (groups == 9)).any()
    assert (last == nb[read]).any()
    on_long = read == mc.LONG_BASE_READ
    holds = on_long & (first <= mc.LONG_BASE) & (last > mc.LONG_BASE)
    beside = on_long & ~holds & (first // 64 == mc.LONG_BASE // 64) & ((last - 1) // 64 == mc.LONG_BASE // 64)
    assert holds.any() and beside.any()
    assert ((n == 1) & (nb[read] == 1)).any()


def test_signal_pairs_realise_every_planned_count(synth):
    reads, _ = synth
    pairs = mc.signal_pairs(reads)
    n_sig = np.array([int(reads[p[0]][1][p[2]] - reads[p[0]][1][p[1]]) for p in pairs])
    n_map = pairs[:, 2] - pairs[:, 1] + 1
    for fl in (0, 1):
        m = pairs[:, 6] == fl
        assert set(mc.SIGNAL_SAMPLE_COUNTS) <= set(n_sig[m].tolist()) and n_sig[m].max() > 5000
        assert set(mc.SIGNAL_MAP_ENTRIES) <= set(n_map[m].tolist()) and n_map[m].max() > 2048
    zero = pairs[n_sig == 0][0]
    assert zero[2] - zero[1] == 2  # a run of zero-dwell bases, not an empty span
    for p in pairs:
        sig, entries, start = mc.signals_expected(reads[p[0]], p, False)
        raw = mc.signals_expected(reads[p[0]], p, True)[0]
        assert sig.dtype == np.float64 and raw.dtype == np.int16 and sig.size == raw.size == entries[-1] and entries[0] == 0
        assert entries.size == p[2] - p[1] + 1 and (np.diff(entries) >= 0).all() and start == reads[p[0]][1][p[1]]
    # the header's rule on a hand-made read
    read = (np.array([5, 6, 7, 8, 9, 10], np.int16), np.array([1, 1, 3, 6], np.int64), 1.0, 2.0)
    sig, entries, start = mc.signals_expected(read, [0, 0, 3, 0, 0, 0, 0], True)
    assert (sig.tolist(), entries.tolist(), start) == ([6, 7, 8, 9, 10], [0, 0, 2, 5], 1)
    sig, entries, start = mc.signals_expected(read, [0, 1, 3, 0, 0, 0, 1], False)
    assert (sig.tolist(), entries.tolist(), start) == ([4.5, 4.0, 3.5, 3.0, 2.5], [0, 3, 5], 1)


def _splits(k):
    return sorted({(0, k - 1), (k - 1, 0), ((k - 1) // 2, k - 1 - (k - 1) // 2)})


def test_kmer_reads_report_sites_at_every_length_and_reach_across_reads():
    assert (2, 2) in _splits(5)
    for k in range(1, 9):
        reads, batches = mc.kmer_reads(SEED, k)
        assert sorted(batches[0] + batches[1]) == list(range(len(reads)))
        for batch in batches:  # empty reads at the front, in the middle and at the end
            empty = [reads[j][2].size == 0 for j in batch]
            assert empty[0] and empty[1] and empty[-1] and any(empty[3:-2]) and not all(empty)
        assert any(r[0] for r in reads) and any(not r[0] for r in reads)
        fwd_nan = [r[3][mc.NAN_AT - r[1]] for r in reads if not r[0] and r[1] <= mc.NAN_AT < r[1] + r[2].size]
        assert len(fwd_nan) >= 3 and np.isnan(fwd_nan).all()
        assert any((r[2] == -1).any() for r in reads)
        total = sum(r[2].size for r in reads)
        for kb, ka in _splits(k):
            for min_cov in (1, 3):
                want = mc.region_kmer_levels(reads, mc.CTG_LEN, kb, ka, min_cov)
                n_sites = sum(len(v) for v in want.values())
                assert n_sites >= 20, (k, kb, ka, min_cov)
                if k >= 6:  # stage 2 cannot sort the sites in one group at a seventh of the bases
                    assert n_sites > total // 7, (k, min_cov, n_sites, total)
        if k >= 5:
            # the two reads that abut, alone on their stretch of the strand: together they report k - 1 sites more than each does
            # alone - the sites beside the seam, whose windows take bases that only the other read covers
            (a, seam), (_, b) = mc.LONE
            n_of = lambda rs, kb, ka: sum(len(v) for v in mc.region_kmer_levels(rs, mc.CTG_LEN, kb, ka, 1).values())  # noqa: E731
            for kb, ka in _splits(k):
                for rev in (False, True):
                    mine = [r for r in reads if r[0] == rev and r[2].size]
                    cover = np.zeros(mc.CTG_LEN, int)
                    for r in mine:
                        cover[r[1] : r[1] + r[2].size] += 1
                    assert (cover[a:b] == 1).all() and (cover[a - 8 : a] == 0).all() and (cover[b : b + 8] == 0).all()
                    first, second = ([r for r in mine if r[1] == s and r[1] + r[2].size <= b] for s in (a, seam))
                    assert len(first) == len(second) == 1
                    assert n_of(first + second, kb, ka) - n_of(first, kb, ka) - n_of(second, kb, ka) == k - 1, (k, kb, ka, rev)
                    assert n_of(first + second, kb, ka) == b - a - (k - 1)


# ---- 3. the median cases --------------------------------------------------------------------------------------------------------
def test_median_edge_sites_are_settled_by_numpy():
    cases_ = mc.median_edge_sites()
    names = [c[0] for c in cases_]
    assert len(set(names)) == len(names)
    counts = set()
    for name, base, vals, want in cases_:
        v = np.asarray(vals, np.float64)
        finite = v[np.isfinite(v)]
        assert 0 <= base <= 3
        if want is None:
            assert finite.size == 0 and v.size > 0, name
            continue
        with np.errstate(over="raise"):
            med = np.median(finite)
        assert np.isfinite(med) and med == want and np.sign(med) == np.sign(want), (name, med, want)
        s = np.sort(finite)
        assert np.isfinite(s[(s.size - 1) // 2] + s[s.size // 2]), name  # the two middle values' sum does not overflow
        if name.endswith(" values") and name[0].isdigit():
            counts.add(v.size)
    assert counts == set(range(1, 10))
    by_name = {c[0]: c for c in cases_}
    assert by_name["mixed signs, even count"][3] == 0.5 and by_name["both zeros"][3] == 0.0
    assert np.signbit(by_name["both zeros"][2][0]) and not np.signbit(by_name["both zeros"][2][1])
    sub = by_name["subnormals of both signs, even count"][3]
    assert sub < 0 and abs(sub) < 2.3e-308 and 0 < by_name["subnormals of both signs, odd count"][3] < 2.3e-308
    assert np.isfinite(by_name["exactly min_cov finite values"][2]).sum() == mc.MEDIAN_MIN_COV
    assert np.isfinite(by_name["min_cov - 1 finite values"][2]).sum() == mc.MEDIAN_MIN_COV - 1
    # one k-mer's site levels cross the sign change: negative, negative subnormal, zero, subnormal, positive
    for min_cov in (1, mc.MEDIAN_MIN_COV):
        levels, n, site_kmer, site_level = mc.median_sites_expected(cases_, min_cov)
        assert n.sum() == site_kmer.size == site_level.size and np.isfinite(levels[n > 0]).all()
        for b in range(4):
            assert (np.diff(site_level[site_kmer == b]) >= 0).all()
    levels, n, site_kmer, site_level = mc.median_sites_expected(cases_, 1)
    zero = site_level[site_kmer == 0]
    assert (zero < -1.0).any() and ((zero < 0) & (zero > -1e-300)).any() and (zero == 0).sum() == 3 and ((zero > 0) & (zero < 1e-300)).any()
    assert n.sum() == len(cases_) - 1  # all but the NaN-only site
    assert mc.median_sites_expected(cases_, mc.MEDIAN_MIN_COV)[1].sum() == sum(np.isfinite(c[2]).sum() >= mc.MEDIAN_MIN_COV for c in cases_)
