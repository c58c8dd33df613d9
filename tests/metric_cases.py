"""Inputs and numpy restatements for the tests that drive the kernels of csrc/k_metrics.hip directly
(tests/test_gpu_region_kernels.py, tests/test_gpu_level_kernels.py); tests/test_host_metric_cases.py holds them to what they
claim without a GPU.  numpy only: no GPU, no torch.

A read here is the tuple (dacs int16, seq_to_sig int64, shift, scale); a region pair the seven int64 the device takes:
read, first, last, lead, row, region length, flip (remora_amd/region_metrics.py)."""
import numpy as np

from metrics_exact import exact_stats

# ---- reads ----------------------------------------------------------------------------------------------------------------
READ_BASES = (1, 63, 64, 65, 256, 257, 320, 705, 2100)  # 2100: the only read with more than 2048 mapping entries (signal_pairs)
ZERO_DWELL_BASES = (63, 64, 127, 128, 255, 256)
LONG_BASE_READ, LONG_BASE, LONG_BASE_SAMPLES = 6, 64, 5000  # base 64 of the 320-base read
PADDED_READ, PAD_LEAD, PAD_TAIL = 3, 17, 23                  # the read with unmapped signal in front of and behind its mapping
ENDS_TWIN_OF, BACK_TWIN_OF, BACK_AT = 5, 7, 317              # the dirty twins' clean reads; the first of the two backward bases
FIRSTS = (0, 1, 63, 64, 65, 127, 191, 255, 256)
SPANS = (1, 2, 63, 64, 65, 66, 255, 256, 257, 513)
SIGNAL_SAMPLE_COUNTS = (0, 1, 255, 256, 2047, 2048, 2049)  # and one above 5000
SIGNAL_MAP_ENTRIES = (2, 256, 257)                         # and one above 2048


def synthetic_reads(seed):
    """-> (reads, twins).  reads: nine clean reads of READ_BASES bases, dwells drawn from 0 to 12, a zero dwell at every base of
    ZERO_DWELL_BASES a read has, one base of 5000 samples (base 64 of the 320-base read, in place of the zero dwell), one read
    (PADDED_READ) whose mapping starts at sample 17 and ends 23 samples before its signal does, the samples -32768 and 32767 in
    every read that has two samples.  twins: [(index of the clean read, dirty read, changed mapping entries)]:
      - of read ENDS_TWIN_OF, a mapping that starts at -3 and whose last entry is sig_len + 5;
      - of read BACK_TWIN_OF, entries BACK_AT + 1 and BACK_AT + 2 set to -2 and -4: the mapping runs backwards across bases
        BACK_AT and BACK_AT + 1 and comes back from outside the signal on base BACK_AT + 2, so each of the three bases a changed
        entry bounds has no samples of its own (k_metrics.hip: "a mapping that leaves the signal: NaN, nothing half-summed").
    Everything else of a twin is its clean read's.  The three bases are the last of their 64-base group (317 .. 319): a wave sums
    the samples of its 64 bases 64 at a time, so where a base's samples are split between two rounds - and with it the last bit
    of its sums - depends on the dwells of the bases in front of it in the group; the bases behind a changed dwell would not
    have to keep the clean read's bits, the bases in front of it do."""
    rng = np.random.default_rng(seed)
    reads = []
    for i, nb in enumerate(READ_BASES):
        dw = rng.integers(0, 13, size=nb)
        if nb == 1:
            dw[0] = 5
        for z in ZERO_DWELL_BASES:
            if z < nb:
                dw[z] = 0
        if i == LONG_BASE_READ:
            dw[LONG_BASE] = LONG_BASE_SAMPLES
        lead, tail = (PAD_LEAD, PAD_TAIL) if i == PADDED_READ else (0, 0)
        mp = (lead + np.concatenate([[0], np.cumsum(dw)])).astype(np.int64)
        dacs = rng.integers(-600, 1600, size=int(mp[-1]) + tail).astype(np.int16)
        if dacs.size >= 2:
            at = rng.choice(dacs.size, size=2, replace=False)
            dacs[at[0]], dacs[at[1]] = -32768, 32767
        reads.append((dacs, mp, float(rng.uniform(300, 500)), float(rng.uniform(50, 150))))
    twins = []
    dacs, mp, sh, sc = reads[ENDS_TWIN_OF]
    dirty = mp.copy()
    dirty[0], dirty[-1] = -3, dacs.size + 5
    twins.append((ENDS_TWIN_OF, (dacs, dirty, sh, sc), (0, mp.size - 1)))
    dacs, mp, sh, sc = reads[BACK_TWIN_OF]
    dirty = mp.copy()
    dirty[BACK_AT + 1], dirty[BACK_AT + 2] = -2, -4
    twins.append((BACK_TWIN_OF, (dacs, dirty, sh, sc), (BACK_AT + 1, BACK_AT + 2)))
    return reads, twins


def per_base_exact(read, st, en):
    """-> (dwell float32[bases], [(base, n, mean, var, sum|x|, sum x^2)]) for every base that has samples left after the trims and
    whose mapping entries lie in order inside the read's signal: metrics_exact.exact_stats of (dacs - shift) / scale in float64,
    the construction metrics_exact.cases uses for the golden reads."""
    dacs, mp, shift, scale = read
    mp = np.asarray(mp, np.int64)
    sig = ((dacs - float(shift)) / float(scale)).tolist()
    bases = []
    for base in range(mp.size - 1):
        ms, me = int(mp[base]), int(mp[base + 1])
        if ms < 0 or me > len(sig) or me - ms - st - en <= 0:
            continue
        x = sig[ms + st : me - en]
        bases.append((base, len(x)) + exact_stats(x))
    return np.diff(mp).astype(np.float32), bases


# ---- region pairs -----------------------------------------------------------------------------------------------------------
def groups_touched(first, last):
    """64-base groups, counted from the read's first base, that bases [first, last) meet."""
    return (last - 1) // 64 - first // 64 + 1


def region_pairs(reads):
    """-> (pairs int64[n, 7], rows, width) over the clean `reads`: every (first, last - first) of FIRSTS x SPANS on a read it
    fits, first % 64 == 63 with 66 and 258 bases (3 and 6 groups: the bound (n + 62) / 64 + 1 met with equality), a span that
    ends on its read's last base, a pair inside the group of the 5000-sample base that leaves it out, pairs that hold it; flip,
    lead (0, 1, region length - covered) and the region length (the covered span, or longer) take turns.  Rows are distinct and
    in no order; `width` is three columns more than the longest region."""
    nb = [r[1].size - 1 for r in reads]
    spans = [(f, n) for f in FIRSTS for n in SPANS] + [(63, 258), (127, 258)]
    table = []
    for i, (first, n) in enumerate(spans):
        fit = [r for r in range(len(reads)) if first + n <= nb[r]]
        assert fit, (first, n)
        table.append([fit[i % len(fit)], first, first + n, i])
    k = len(table)
    table.append([LONG_BASE_READ, 64, nb[LONG_BASE_READ], k])        # ends on the read's last base
    table.append([LONG_BASE_READ, LONG_BASE + 1, LONG_BASE + 3, k + 1])  # beside the 5000-sample base, inside its group
    table.append([LONG_BASE_READ, LONG_BASE, LONG_BASE + 1, k + 2])  # the 5000-sample base alone
    table.append([LONG_BASE_READ, 1, 130, k + 3])                    # ... and in the middle of three groups
    table.append([0, 0, 1, k + 4])                                   # the whole one-base read
    pairs = []
    for read, first, last, i in table:
        covered = last - first
        flip, how = i % 2, (i // 2) % 4
        rlen = covered if how == 0 else covered + 1 + i % 5
        lead = (0, 0, 1, rlen - covered)[how]
        pairs.append([read, first, last, lead, 0, rlen, flip])
    pairs = np.asarray(pairs, np.int64)
    pairs[:, 4] = np.random.default_rng(len(pairs)).permutation(len(pairs))
    return pairs, len(pairs), int(pairs[:, 5].max()) + 3


def region_rows_expected(per_base_arrays, pairs, rows, width):
    """float64 [rows, width]: base first + i of a pair's read at column lead + i of the pair's row, or, flipped, at column region
    length - 1 - (lead + i); NaN everywhere else.  per_base_arrays[read]: that read's whole per-base array (float32 is widened)."""
    out = np.full((rows, width), np.nan, np.float64)
    for read, first, last, lead, row, rlen, flip in np.asarray(pairs, np.int64)[:, :7].tolist():
        vals = np.asarray(per_base_arrays[read][first:last], np.float64)
        cols = lead + np.arange(last - first)
        out[row, rlen - 1 - cols if flip else cols] = vals
    return out


def _span_with_samples(mp, n_samples, taken):
    """(first, last) with mp[last] - mp[first] == n_samples, the shortest such span that is not in `taken`."""
    best = None
    for first in range(mp.size - 1):
        last = int(np.searchsorted(mp, mp[first] + n_samples, "left"))
        last = max(last, first + 1)
        if last < mp.size and mp[last] - mp[first] == n_samples and (first, last) not in taken:
            if best is None or last - first < best[1] - best[0]:
                best = (first, last)
    return best


def signal_pairs(reads):
    """-> pairs int64[n, 7] (lead, row and region length 0: rmr_region_signals does not look at them) over the clean `reads`: spans
    of SIGNAL_SAMPLE_COUNTS samples and one that holds the 5000-sample base, spans of SIGNAL_MAP_ENTRIES mapping entries and the
    whole 2100-base read, the padded read from end to end; each forward and flipped.  A count no span has is an AssertionError."""
    nb = [r[1].size - 1 for r in reads]
    zero_read = next(r for r in range(len(reads)) if r != LONG_BASE_READ and nb[r] > 65)
    spans = [(zero_read, 63, 65)]  # two zero-dwell bases: no sample at all
    big = len(reads) - 1
    taken = set()
    for n in SIGNAL_SAMPLE_COUNTS[1:]:
        got = _span_with_samples(reads[big][1], n, taken)
        assert got is not None, f"no span of {n} samples"
        taken.add(got)
        spans.append((big,) + got)
    spans.append((LONG_BASE_READ, 60, 70))
    for entries in SIGNAL_MAP_ENTRIES:
        spans.append((BACK_TWIN_OF, 65, 65 + entries - 1))
    spans.append((big, 0, nb[big]))
    spans.append((PADDED_READ, 0, nb[PADDED_READ]))
    return np.asarray([[r, f, la, 0, 0, 0, flip] for r, f, la in spans for flip in (0, 1)], np.int64)


def signals_expected(read, pair, raw):
    """-> (samples, mapping entries, sig_start) as include/remora_hip.h states them: the samples [map[first], map[last]) as
    (dacs - shift) / scale in float64 (`raw`: the int16 samples), map[first : last + 1] - map[first]; flipped: the samples back to
    front and map[last] - map[first : last + 1][::-1]; sig_start = map[first]."""
    dacs, mp, shift, scale = read
    first, last, flip = int(pair[1]), int(pair[2]), int(pair[6])
    ms, me = int(mp[first]), int(mp[last])
    sig = dacs[ms:me].copy() if raw else (dacs[ms:me] - float(shift)) / float(scale)
    entries = mp[first : last + 1]
    if flip:
        return sig[::-1].copy(), (me - entries[::-1]).astype(np.int64), ms
    return sig, (entries - ms).astype(np.int64), ms


# ---- k-mer levels -------------------------------------------------------------------------------------------------------------
CTG_LEN, N_AT, NAN_AT = 400, 140, 100
PILE_READS, PILE_LEN, PILE_STEP = 28, 100, 14
LONE = ((300, 340), (340, 380))  # two reads per strand that abut, with nobody else there: a window across the seam takes bases
                                 # only the other read covers


def region_kmer_levels(reads, ctg_len, kb, ka, min_cov):
    """numpy restatement of io.get_region_kmers (src/remora/io.py:966-982; the metrics matrix of get_ref_reg_sample_metrics
    :864-886 with ref_orient=False and the sequence of get_ref_int_seq_from_reads :671-695), one region per strand spanning
    the contig.  reads: (is_reverse, ref_start, read-oriented base codes, read-oriented trimmean).  -> {k-mer index: levels}."""
    k = kb + ka + 1
    out = {}
    for rev in (False, True):
        mine = [r for r in reads if r[0] == rev]
        mat = np.full((len(mine), ctg_len), np.nan)
        seq = np.full(ctg_len + kb + ka, -2, np.int64)  # read-oriented; [kb + o] is the base of read-oriented offset o
        for row, (_, start, codes, vals) in enumerate(mine):
            o0 = ctg_len - (start + codes.size) if rev else start  # read-oriented offset of the read's first base
            mat[row, o0 : o0 + codes.size] = vals
            seq[kb + o0 : kb + o0 + codes.size] = codes
        for offset in range(ctg_len):
            kmer = seq[offset : offset + k]
            if (kmer < 0).any():
                continue
            site = mat[:, offset]
            site = site[np.isfinite(site)]
            if site.size < min_cov:
                continue
            idx = int(sum(int(b) * 4 ** (k - 1 - j) for j, b in enumerate(kmer)))
            out.setdefault(idx, []).append(np.median(site))
    return out


def kmer_reads(seed, k_total):
    """-> (reads, batches) on one contig of CTG_LEN bases: reads (is_reverse, ref_start, read-oriented codes int8, read-oriented
    values) as region_kmer_levels takes them; batches: two lists of indices into `reads`, together every read once.
    A pile of PILE_READS reads on alternating strands whose coverage climbs and falls (NaN and inf among the values), an N in
    the reference at N_AT, a forward site (NAN_AT) whose values are all NaN, two reads per strand that abut (LONE), and empty
    reads at the front, in the middle and at the end of each batch.  The layout is the same for every k-mer length; `k_total`
    only enters the random stream, so that every length sees bases and values of its own."""
    rng = np.random.default_rng([seed, k_total])
    ref = rng.integers(0, 4, size=CTG_LEN)
    ref[N_AT] = -1

    def read(rev, start, n):
        fwd = ref[start : start + n]
        assert fwd.size == n
        codes = np.where(fwd[::-1] >= 0, 3 - fwd[::-1], -1) if rev else fwd.copy()
        vals = rng.normal(size=n)
        vals[rng.random(n) < 0.05] = np.nan
        vals[rng.random(n) < 0.01] = np.inf
        if not rev and start <= NAN_AT < start + n:
            vals[NAN_AT - start] = np.nan
        return (rev, start, codes.astype(np.int8), vals)

    full = [read(bool(i % 2), PILE_STEP * (i // 2) + (3 if i % 2 else 0), PILE_LEN - (i // 2)) for i in range(PILE_READS)]
    for rev in (False, True):
        for a, b in LONE:
            r = read(rev, a, b - a)
            r[3][:] = np.where(np.isfinite(r[3]), r[3], 0.25)  # every base of the seam's reads is a site
            full.append(r)
    order = rng.permutation(len(full)).tolist()
    empty = lambda j: (bool(j % 2), (7 * j) % 390, np.zeros(0, np.int8), np.zeros(0, np.float64))  # noqa: E731
    reads, batches = [], []
    for part in (order[: len(order) // 3], order[len(order) // 3 :]):
        mid = len(part) // 2
        seq = ["e", "e"] + part[:mid] + ["e"] + part[mid:] + ["e"]
        batch = []
        for item in seq:
            batch.append(len(reads))
            reads.append(empty(len(reads)) if item == "e" else full[item])
        batches.append(batch)
    return reads, batches


MEDIAN_MIN_COV = 4


def median_edge_sites():
    """-> [(name, base code, values, median)] for k = 1, one site each; `median` is what the case was built for (None: the site
    is not reported with min_cov 1).  Sites of base 0 hold negative medians, both zeros, subnormals and positive ones, so that
    the site levels of one k-mer ascend across the sign change.  No two middle values have a sum that overflows."""
    nan, inf, tiny = float("nan"), float("inf"), 5e-324
    cases = [
        ("mixed signs, even count", 0, [-1.0, 2.0], 0.5),
        ("both zeros", 0, [-0.0, 0.0], 0.0),
        ("zeros and the smallest subnormal", 0, [0.0, -0.0, tiny], 0.0),
        ("four equal values", 0, [2.5, 2.5, 2.5, 2.5], 2.5),
        ("large magnitudes among non-finite values", 0, [-1e300, 1e300, nan, inf, -inf], 0.0),
        ("subnormals of both signs, odd count", 0, [-1e-310, -tiny, tiny, 3e-310, 2e-310], tiny),
        ("subnormals of both signs, even count", 0, [-3e-310, -1e-310, -tiny, 2e-310], (-1e-310 + -tiny) / 2.0),
        ("negative values", 0, [-3.0, -2.0, -1.0], -2.0),
        ("one negative subnormal", 0, [-tiny], -tiny),
        ("large negative values", 0, [-1e300, -1e299], (-1e300 + -1e299) / 2.0),
        ("ties around the middle", 1, [1.0, -1.0, 1.0, -1.0, 1.0, 7.0], 1.0),
        ("exactly min_cov finite values", 1, [4.0, nan, 1.0, 3.0, nan, 2.0], 2.5),
        ("min_cov - 1 finite values", 1, [4.0, nan, 1.0, nan, 3.0, nan], 3.0),
        ("NaN only", 1, [nan, nan, nan], None),
    ]
    assert sum(np.isfinite(cases[-3][2])) == MEDIAN_MIN_COV and sum(np.isfinite(cases[-2][2])) == MEDIAN_MIN_COV - 1
    rng = np.random.default_rng(17)
    for count in range(1, 10):  # odd and even counts, values of both signs in no order
        vals = (rng.permutation(19)[:count] - 9) * 0.375
        cases.append((f"{count} values", 2 + count % 2, vals.tolist(), float(np.median(vals))))
    return cases


def median_sites_expected(cases, min_cov):
    """-> (levels[4], counts[4], site_kmer, site_level) of the cases at k = 1 as numpy has them."""
    per = {b: [] for b in range(4)}
    for _, base, vals, _ in cases:
        v = np.asarray(vals, np.float64)
        v = v[np.isfinite(v)]
        if v.size >= max(1, min_cov):
            per[base].append(np.median(v))
    levels = np.array([np.median(per[b]) if per[b] else np.nan for b in range(4)])
    counts = np.array([len(per[b]) for b in range(4)], np.int64)
    return levels, counts, np.repeat(np.arange(4, dtype=np.int32), counts), np.concatenate([np.sort(per[b]) for b in range(4)])


def long_read(n, k_total, seed):
    """One read of n bases on site 0: (codes int8[n] of 0..3, values float64[n], distinct and finite, of both signs)."""
    rng = np.random.default_rng([seed, k_total, n])
    return rng.integers(0, 4, size=n).astype(np.int8), (rng.permutation(n) - n // 2) * 0.25


def long_read_expected(codes, vals, kb, ka):
    """With min_cov 1 every site whose window lies inside the read is reported: -> (k-mer index int64, level) of the sites
    kb .. n - ka - 1, in site order.  The level of a site is its one value, its k-mer the window's index."""
    k, n = kb + ka + 1, codes.size
    kmer = np.zeros(n - k + 1, np.int64)
    for j in range(k):
        kmer = kmer * 4 + codes[j : j + n - k + 1]
    return kmer, vals[kb : n - ka].copy()
