"""CPU checks of tests/data_cases.py, which tests/test_gpu_data_kernels.py relies on: every encode case takes, by the restated
choice of launch_encode, the kernel it is there for; the choice as it was sends shapes to an unrolled kernel that is wrong for
them and the present one sends none; and the numpy restatements the GPU tests compare with agree with the oracle, np.argmax, a
float64 cross entropy and Motif.findall."""
import numpy as np
import pytest

import data_cases as D


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


# ---- launch_encode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.ENCODE_CASES, ids=lambda c: c.name)
def test_every_encode_case_takes_its_path(case):
    K = case.kb + case.ka + 1
    seq_w, map_w = case.max_len + K - 1, case.max_len + 1
    p = D.encode_plan(K, case.L, seq_w, map_w)
    old = D.encode_plan(K, case.L, seq_w, map_w, rule="nst")
    assert p.pf == 1 and p.valid and p.lds <= D.ENCODE_LDS_LIMIT and 4 * K * case.L < D.ENCODE_MAX_FLOATS, (case, p)
    if case.path.startswith("unrolled"):
        assert p.NST == int(case.path[8:]) == p.nst and p.code_form and old == p, (case, p)
    elif case.path.startswith("collide"):  # the old rule: an unrolled kernel, its code form wrong for the shape; now the general form
        assert old.NST == int(case.path[7:]) and old.code_form and not old.valid, (case, old)
        assert p.NST == 0 and not p.code_form, (case, p)
    else:
        assert p.NST == 0 and p.code_form == (case.path == "code") and old == p, (case, p)
    for form in (1, 0):  # RMR_ENCODE_FORM 1 and 0: no unrolled kernel, the plain loop's own rule; 0: no prefetch either
        q = D.encode_plan(K, case.L, seq_w, map_w, form=form)
        assert q.NST == 0 and q.valid and q.pf == form and q.lds <= D.ENCODE_LDS_LIMIT, (case, form, q)


def test_encode_cases_cover_what_they_must():
    cases = {c.name: c for c in D.ENCODE_CASES}
    assert len(cases) == len(D.ENCODE_CASES) and set(D.HOST_FORM_CASES) <= set(cases)
    # the shipped pairs keep their unrolled kernels
    shipped = {(c.kb + c.ka + 1, c.L): D.encode_plan(c.kb + c.ka + 1, c.L, 28, 21).NST for c in D.ENCODE_CASES if c.name.startswith("shipped")}
    assert shipped == dict(zip(D.SHIPPED, D.UNROLLED_NST))
    for nst in D.UNROLLED_NST:  # three or more colliding pairs each: an L % 4 == 2, an odd L and a K > 10 among them
        cs = [c for c in D.ENCODE_CASES if c.path == f"collide{nst}"]
        assert len(cs) >= 3, nst
        assert any(c.L % 4 == 2 for c in cs) and any(c.L % 2 for c in cs) and any(c.kb + c.ka + 1 > 10 for c in cs), nst
    k10, k11 = cases["k10-code-limit"], cases["k11-past-code-limit"]
    assert (k10.kb + k10.ka + 1, k11.kb + k11.ka + 1) == (10, 11) and k10.L % 4 == 0 == k11.L % 4
    assert D.encode_plan(10, k10.L, 29, 21).nst not in D.UNROLLED_NST and D.encode_plan(11, k11.L, 30, 21).nst not in D.UNROLLED_NST
    ks, ls = {c.kb + c.ka + 1 for c in D.ENCODE_CASES}, {c.L for c in D.ENCODE_CASES}
    assert {1, 21} <= ks and {4, 5, 7, 8, 94, 1000} <= ls and ((94 + 7) & ~7) - 94 < 3
    assert sum(c.kb != c.ka for c in D.ENCODE_CASES) >= 10
    # the LDS limit: the longest chunk that is launched fills it exactly, the refused one needs one padded row more
    c = cases["lds-limit"]
    assert D.encode_plan(1, c.L, c.max_len, c.max_len + 1).lds == D.ENCODE_LDS_LIMIT
    kb, ka, L, ml = D.ENCODE_REFUSED
    assert D.encode_plan(kb + ka + 1, L, ml + kb + ka, ml + 1).lds > D.ENCODE_LDS_LIMIT and 4 * (kb + ka + 1) * L < D.ENCODE_MAX_FLOATS
    # the width cases: every prefetch form and the unprefetched one, either side of each step
    pfs = [D.encode_plan(kb + ka + 1, L, w, w).pf for w in D.WIDTHS for kb, ka, L in [D.WIDTH_SHAPES[w]]]
    assert pfs == [1, 2, 2, 4, 4, 0]
    for cus in (256, 304):
        assert D.second_trip_chunks(cus) > 4 * 8 * cus  # more chunks than waves: every wave hands its prefetched rows over


def test_the_store_count_alone_sent_wrong_shapes_to_the_unrolled_kernels_and_the_fixed_rule_sends_none():
    """Why launch_encode keys on more than nst: by nst alone (the rule as it was), 60 and more (K, L) with K <= 21, L <= 256 take
    each unrolled kernel although its code form is wrong for them - the colliding cases of the table among them.  The rule as
    it is: none, for K = 1 .. 21 and L = 4 .. 1000."""
    found = {nst: D.colliding_pairs("nst", nst) for nst in D.UNROLLED_NST}
    print({nst: len(v) for nst, v in found.items()})
    for nst, pairs in found.items():
        assert 60 <= len(pairs) <= 114, (nst, len(pairs))
        for c in D.ENCODE_CASES:
            if c.path == f"collide{nst}" and c.L <= 256:
                assert (c.kb + c.ka + 1, c.L) in pairs, c
    for ex in ((6, 150), (10, 90), (12, 75), (15, 60)):
        assert ex in found[15]
    assert (9, 202) in found[29]
    for nst in D.UNROLLED_NST:
        assert D.colliding_pairs("fixed", nst, 21, 4, 1000) == []
    for K in range(1, 22):
        for L in range(4, 1001):
            for form in (2, 1, 0):
                assert D.encode_plan(K, L, 64, 64, form).valid
    for K, L in D.SHIPPED:
        assert D.encode_plan(K, L, 64, 64) == D.encode_plan(K, L, 64, 64, rule="nst")


# ---- the restatements the GPU tests compare with -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in D.ENCODE_CASES if c.L <= 202], ids=lambda c: c.name)
def test_encode_inputs_and_the_gather_restatement_against_the_oracle(O, case):
    """The inputs are what they say (chunks of 0, 1 and max_len bases, -1 inside the context, non-decreasing rows), and the
    oracle's scatter loops give on them what the gather form gives that the kernel uses."""
    seqs, maps, lens = D.encode_inputs(case.kb, case.ka, case.L, D.N_SWEEP, case.max_len)
    K = case.kb + case.ka + 1
    assert list(lens[1:4]) == [0, 1, case.max_len] and lens[0] >= 1 and maps[0, lens[0]] == case.L
    for c in range(D.N_SWEEP):
        row = maps[c, : lens[c] + 1]
        assert np.all(np.diff(row) >= 0) and row[-1] == case.L and (row[0] == 0 or lens[c] == 0)
    inside = np.arange(seqs.shape[1])[None, :] < (lens[:, None] + K - 1)
    assert (seqs[inside] == -1).any() and seqs.min() >= -1 and seqs.max() <= 3
    ref = O.compute_encoded_kmer_batch(case.kb, case.ka, seqs, maps, lens)
    assert ref.shape == (D.N_SWEEP, 4 * K, case.L) and ref[1].sum() == 0 and ref.sum() > 0
    assert np.array_equal(ref, D.encode_ref(case.kb, case.ka, seqs, maps, lens))


def test_width_padding_changes_nothing_for_the_oracle(O):
    for w in D.WIDTHS:
        kb, ka, L = D.WIDTH_SHAPES[w]
        a = D.encode_inputs(kb, ka, L, 50, 20, seed=w)
        b = D.encode_inputs(kb, ka, L, 50, 20, seq_w=w, map_w=w, seed=w)
        assert b[0].shape == (50, w) and b[1].shape == (50, w) and np.array_equal(a[2], b[2])
        ra, rb = O.compute_encoded_kmer_batch(kb, ka, *a), O.compute_encoded_kmer_batch(kb, ka, *b)
        assert rb.shape == (50, 4 * (kb + ka + 1), L) and rb.sum() > 0 and ra.shape == rb.shape


@pytest.mark.parametrize("kf", D.NUM_LABELS)
def test_tally_restatement(O, kf):
    """tally_ref against add_unmodeled_labels, oracle.softmax_axis1, np.argmax and torch's float64 cross entropy; and its
    float32 probabilities within (num_labels + 4) 2^-24 of the float64 ones (one rounding of the difference, an exp within
    1 ulp or so, num_labels - 1 additions, a division)."""
    import torch

    from remora_amd.validate import add_unmodeled_labels

    n = 4000
    for form, loc in D.label_maps(kf).items():
        km = int((loc >= 0).sum())
        assert sorted(loc[loc >= 0]) == list(range(km)) and 1 <= km <= kf
        rng = np.random.default_rng([kf, km])
        labels = rng.integers(0, kf, n)
        x = D.tally_logits(n, km, 1)
        t = D.tally_ref(x, labels, kf, loc)
        wide = D.widen(x, kf, loc)
        if form in ("middle", "end"):  # the product's own widening (label 0 modelled, columns in order, as the reference has it)
            assert np.array_equal(wide, add_unmodeled_labels(x, np.flatnonzero(loc < 0)))
        assert t.finite.all()
        assert np.array_equal(t.call, np.argmax(wide, axis=1)) and t.confusion.sum() == n
        for i in range(kf):
            for j in range(kf):
                assert t.confusion[i, j] == np.sum((labels == i) & (t.call == j))
        p64 = O.softmax_axis1(wide.astype(np.float64))
        win64 = p64[np.arange(n), t.call]
        assert np.allclose(t.win64, win64, rtol=1e-14, atol=0) and np.all(win64 == p64.max(axis=1))
        # the float32 softmax of the reference: the same call wherever the two best logits are apart, the same probability to rounding
        p32 = O.softmax_axis1(wide)
        assert p32.dtype == np.float32
        top2 = np.sort(wide, axis=1)[:, -2:] if kf > 1 else None
        apart = np.ones(n, bool) if kf == 1 else (top2[:, 1] - top2[:, 0]) > 1e-3
        assert np.array_equal(np.argmax(p32, axis=1)[apart], t.call[apart])
        rel = np.abs(t.win32.astype(np.float64) - win64) / win64
        rel_np = np.abs(p32[np.arange(n), t.call].astype(np.float64) - win64) / win64
        print(f"kf {kf} {form}: float32 softmax worst relative error {rel.max() * 2**24:.2f} x 2^-24 (np.sum order: {rel_np.max() * 2**24:.2f})")
        assert rel.max() <= (kf + 4) * 2.0**-24 and rel_np.max() <= (kf + 4) * 2.0**-24
        ce = torch.nn.functional.cross_entropy(torch.from_numpy(wide.astype(np.float64)), torch.from_numpy(labels), reduction="none").numpy()
        assert np.allclose(t.terms, ce, rtol=1e-12, atol=1e-12)
        # special rows: ties, an unmodelled column winning, a tie with it
        assert (np.sum(wide == wide.max(axis=1, keepdims=True), axis=1) > 1).sum() >= n // 16 or km == 1
        if km < kf:
            assert np.isin(t.call[np.arange(n) % 16 == 7], np.flatnonzero(loc < 0)).all()


def test_tally_and_count_restatements_on_non_finite_rows():
    """np.argmax calls the first NaN, else the first +inf; the probabilities of such rows are NaN in float32 and float64 alike;
    rows whose only non-finite entries are -inf (not all of them) keep finite probabilities."""
    assert list(np.argmax(np.array([[1, np.nan, 5, np.nan], [np.inf, np.nan, 1, 2], [1, np.inf, np.inf, 0], [-np.inf, -np.inf, -3e38, 0],
                                    [-np.inf] * 4], np.float32), axis=1)) == [1, 1, 1, 3, 0]
    for kf, form in ((16, "equal"), (5, "middle"), (3, "permuted")):
        loc = D.label_maps(kf)[form]
        km = int((loc >= 0).sum())
        x = D.tally_logits(2048, km, 2, nonfinite=True)
        labels = np.random.default_rng(kf).integers(0, kf, 2048)
        t = D.tally_ref(x, labels, kf, loc)
        wide = D.widen(x, kf, loc)
        nan_row, inf_row = np.isnan(wide).any(axis=1), np.isposinf(wide).any(axis=1)
        assert nan_row.sum() >= 200 and (inf_row & ~nan_row).sum() >= 100 and (~t.finite).sum() >= 500 and t.finite.sum() >= 1000
        assert np.isnan(wide[nan_row, t.call[nan_row]]).all()
        first_nan = np.argmax(np.isnan(wide), axis=1)
        assert np.array_equal(t.call[nan_row], first_nan[nan_row])
        assert np.isposinf(wide[inf_row & ~nan_row, t.call[inf_row & ~nan_row]]).all()
        assert np.array_equal(np.isnan(t.win32), np.isnan(t.win64))
        all_neg = np.isneginf(wide).all(axis=1)
        assert np.array_equal(np.isnan(t.win64), nan_row | inf_row | all_neg)
        assert np.array_equal(D.count_ref(wide, kf), np.bincount(t.call, minlength=kf))
        assert (t.call[nan_row] > 0).any()  # rows that a `v > best` scan would call 0 or the largest number


@pytest.mark.parametrize("stored,kept", D.TRIM_CONTEXTS)
def test_trim_inputs_keep_the_oracle_inside_its_rows(O, stored, kept):
    """trim_ref asserts every index of the reference's unguarded loops; the oracle gives the same arrays."""
    for n in D.TRIM_SIZES:
        seqs, maps, lens = D.trim_inputs(stored, kept, n)
        r = np.arange(n)
        (sb, sa), (cb, ca) = stored, kept
        assert (lens[r % 8 == 5] == 1).all() and maps.shape[1] == 25 and lens.max() == 24
        left = (r % 8 == 1) & (lens > 1)
        assert all((maps[c, : lens[c]] <= 0).all() for c in np.flatnonzero(left))
        right = (r % 8 == 3) & (lens > 1)
        assert all((maps[c, 1 : lens[c] + 1] >= cb + ca).all() for c in np.flatnonzero(right))
        want = D.trim_ref(stored, kept, D.TRIM_SEQ_CONTEXT, seqs, maps, lens)
        got = [a.copy() for a in (seqs, maps, lens)]
        O.trim_sb_chunk_context_core(sb, sa, cb, ca, D.TRIM_SEQ_CONTEXT, *got)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        changed = not np.array_equal(want[2], lens) or not np.array_equal(want[1], maps)
        assert changed == (stored != kept)
        if sb > cb:   # the start clip at its limit: one base left
            assert (want[2][left] == 1).all() and left.sum() >= 20
        if sa > ca:
            assert (want[2][right] == 1).all() and right.sum() >= 20


def test_motif_flags_restatement_and_the_reads():
    """Read boundaries where the kernel's 16-base groups and 4096-base blocks end, empty reads first, twice in the middle and
    last; the flags are Motif.findall's hits per read; a motif over a boundary is a hit of the concatenation and of no read."""
    from remora_amd.util import Motif

    reads = D.motif_reads()
    seq, off = D.concat_reads(reads)
    assert [r.size for r in reads] == list(D.MOTIF_READ_LENGTHS)
    assert {15, 16, 17, 4095, 4096, 4097} <= set(off.tolist()) and off[-1] % 16 != 0 and off[-1] > 4096
    sizes = [r.size for r in reads]
    assert sizes[0] == 0 and sizes[-1] == 0 and any(a == 0 == b for a, b in zip(sizes[1:-1], sizes[2:-1]))
    assert (seq == -1).sum() > 20
    for name, motifs in D.MOTIF_SETS.items():
        want = D.motif_flags_ref(reads, motifs)
        assert 0 < want.sum() < seq.size, name
        slow = np.zeros(seq.size, np.uint8)  # the same by Motif.match's rule on every base: the whole motif inside the read
        for r, o in zip(reads, off):
            for raw, focus in motifs:
                mot = Motif(raw, focus)
                for st in range(r.size - len(mot.raw_motif) + 1):
                    if all(r[st + k] in allowed for k, allowed in enumerate(mot.int_pattern)) and 0 <= st + mot.focus_pos < r.size:
                        slow[o + st + mot.focus_pos] = 1
        assert np.array_equal(want, slow), name
    assert len(D.MOTIF_SETS["eight"]) == 8 and len(Motif(*D.MOTIF_SETS["len16"][0]).raw_motif) == 16
    assert Motif(*D.MOTIF_SETS["negative-focus"][0]).focus_pos == -2 and "N" in D.MOTIF_SETS["iupac-n"][0][0]
    for motif, base in D.STRADDLES:
        assert D.motif_flags_ref([seq], (motif,))[base] == 1 and D.motif_flags_ref(reads, (motif,))[base] == 0, (motif, base)


def test_extraction_reads_and_the_oracle(O):
    """The oracle extracts every chunk of the batch's reads (a read of one base and focus bases on first and last bases among
    them) and the batch has the signal lengths and the reads without focus bases where the kernels' groups need them."""
    reads = D.extract_reads()
    sig = [r["dacs"].size for r in reads]
    assert {1, 7, 8, 9, 2049} == set(sig) and {s % 8 for s in sig} == {0, 1, 7}
    nofocus = [r["focus_bases"] is None for r in reads]
    assert nofocus[0] and nofocus[-1] and any(a and b for a, b in zip(nofocus[1:-1], nofocus[2:-1]))
    assert any(r["int_seq"].size == 1 and r["focus_bases"] is not None for r in reads)
    assert D.EXTRACT_CONTEXT[0] != D.EXTRACT_CONTEXT[1]
    n = 0
    for r in reads:
        assert r["seq_to_sig_map"].size == r["int_seq"].size + 1 and np.all(np.diff(r["seq_to_sig_map"]) >= 1)
        if r["focus_bases"] is None:
            continue
        assert r["focus_bases"][0] == 0 and r["focus_bases"][-1] == r["int_seq"].size - 1
        osig = O.normalise_signal(r["dacs"], r["shift"], r["scale"])
        ch = O.extract_chunks(osig, r["seq_to_sig_map"], r["int_seq"], r["focus_bases"], D.EXTRACT_CONTEXT, D.EXTRACT_KMER)
        assert ch["signal"].shape == (r["focus_bases"].size, 1, sum(D.EXTRACT_CONTEXT)) and (ch["sequence_lengths"] >= 1).all()
        n += r["focus_bases"].size
    assert n == 12
