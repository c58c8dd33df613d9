"""CPU checks of tests/vbz_cases.py, which tests/test_gpu_vbz_paths.py relies on: with the oracle alone, every valid case
decodes (C and numpy restatement) to the samples that were encoded and every corrupt stream is refused; and plan(), the
restatement of vbz_decode_kernel's control flow, places every case in the class it was built for: each (mis, first or later
step) pair, each output residue, the vector store under each key pattern, each nv of a partial lane, the 513-dword step, each
refusal site at each position.  A GPU test can then never pass on an empty class: it runs every case listed here, none left out."""
import numpy as np
import pytest

import vbz_cases as C
from oracle import oracle as O

_plans = {}


def _plan(case, as_built=False):
    """The case's plan with the pointers aligned (host pointers, io.vbz_decode_batch) or as the device-pointer entry offsets them."""
    key = (case.name, as_built)
    if key not in _plans:
        _plans[key] = C.plan(C.pairs(case), case.svb_mod4 if as_built else 0, case.out_mod8 if as_built else 0, row_off=case.row_off)
    return _plans[key]


def _both(case):
    return (_plan(case), _plan(case, True)) if (case.svb_mod4 or case.out_mod8) else (_plan(case),)


def _steps(cases=C.VALID, as_built=(False, True)):
    """(case, row, row plan, step index, step plan) over the cases' plans (a case without pointer offsets has one plan)."""
    for c in cases:
        for b in sorted({b and bool(c.svb_mod4 or c.out_mod8) for b in as_built}):
            for r, rp in zip(c.rows, _plan(c, b).rows):
                for k, s in enumerate(rp.steps):
                    yield c, r, rp, k, s


def test_encoder_is_the_one_the_suite_has_always_used():
    """encode() without its options is _svb16_encode of test_gpu_parity.py (moved): canonical keys, no padding bits; with them
    the decoded samples stay what they were."""
    rng = np.random.default_rng(0)
    s = rng.integers(-300, 300, 21).astype(np.int16)
    raw = np.frombuffer(C.encode(s), np.uint8)
    wide = C.zigzag_of(s) > 0xFF
    assert raw.size == 3 + 21 + int(wide.sum()) and np.array_equal(np.unpackbits(raw[:3], bitorder="little")[:21], wide)
    assert raw[2] >> 5 == 0
    padded = np.frombuffer(C.encode(s, pad_bits=0xFF), np.uint8)
    assert padded[2] >> 5 == 7 and np.array_equal(padded[:2], raw[:2]) and np.array_equal(padded[3:], raw[3:])
    forced = C.encode(s, two=np.ones(21, bool))
    assert len(forced) == 3 + 42
    for b in (C.encode(s), padded.tobytes(), forced):
        np.testing.assert_array_equal(O.vbz_decode(b, 21), s)
    assert np.array_equal(C.samples_of_zigzag(C.zigzag_of(s)), s)


@pytest.mark.parametrize("case", C.VALID, ids=lambda c: c.name)
def test_the_reference_alone_passes_every_valid_case(case):
    for i, r in enumerate(case.rows):
        for dec in (O.vbz_decode, O.vbz_decode_numpy):
            got = dec(r.data, r.n)
            assert got.dtype == np.int16 and got.tobytes() == r.samples.tobytes(), (case.name, i, r.tag, dec.__name__)
    p = _plan(case, True)
    assert p.site is None and len(p.rows) == len(case.rows)
    assert all(s.dwords <= C.LDS_DWORDS for rp in p.rows for s in rp.steps)


def test_case_names_are_unique_and_all_rows_small():
    names = [c.name for c in C.VALID + C.CORRUPT]
    assert len(set(names)) == len(names)
    assert max(r.n for c in C.VALID + C.CORRUPT for r in c.rows) == C.LONGEST == 3073
    assert {c.cls for c in C.VALID} == {"lengths", "values", "align", "pointers", "shape", "noncanon"}
    assert set(C.SHUFFLED) <= set(names)


@pytest.mark.parametrize("case", C.CORRUPT, ids=lambda c: c.name)
def test_corrupt_cases_are_refused_where_they_were_built_to_be(case):
    for p in _both(case):
        assert (p.site, p.row) == (case.site, case.bad), case.name
    if not case.arg_error:
        for i, r in enumerate(case.rows):   # the oracle refuses the bad rows and no other
            bad_row = i == case.bad or (case.name == "corrupt/two-bad-rows" and i == 3)
            if bad_row:
                with pytest.raises(O.OracleError):
                    O.vbz_decode(r.data, r.n)
                with pytest.raises(O.OracleError):
                    O.vbz_decode_numpy(r.data, r.n)
            else:
                assert O.vbz_decode(r.data, r.n).tobytes() == r.samples.tobytes()


def test_every_refusal_site_at_every_position():
    seen = {(c.site, c.bad) for c in C.CORRUPT if not c.arg_error and c.name != "corrupt/two-bad-rows"}
    assert seen == {(s, at) for s in C.SITES for at in C.POSITIONS}
    assert C.POSITIONS == (0, 2, len(C.GOOD_ROWS) - 1)
    arg = {(c.name.split("/")[1].split("@")[0], c.bad) for c in C.CORRUPT if c.arg_error}
    assert arg == {(k, at) for k in ("negative-n", "decreasing-row-off") for at in C.POSITIONS}
    # what each kernel check has let through before it fires: nothing, nothing or one step, the whole row
    stored = {}
    for c in C.CORRUPT:
        p = _plan(c)
        if p.site != "api":
            stored.setdefault(p.site, set()).add(p.rows[p.row].stored)
    assert stored == {"first": {0}, "prefetch": {0, 1}, "trailing": {1, 3}}
    for kind, (site, row) in C.BAD_ROWS.items():   # the bytes are what the issue of each kind says
        nkeys, size = (row.n + 7) // 8, len(row.data)
        if kind == "short":
            assert size == nkeys + row.n - 1
        elif kind == "bytes-without-samples":
            assert row.n == 0 and size > 0
        else:
            assert size >= nkeys + row.n
    full = C.pattern_row("p50", 2 * C.STEP + 1, 3002)
    assert len(C.BAD_ROWS["short-in-step2"][1].data) == len(full.data) - 1
    assert {k: len(r.data) - len(C.encode(r.samples)) for k, (s, r) in C.BAD_ROWS.items() if s == "trailing"} == {
        "extra1-1step": 1, "extra5-1step": 5, "extra1-3steps": 1, "extra5-3steps": 5}
    assert [len(C.plan([(C.encode(r.samples), r.n)]).rows[0].steps) for k, (s, r) in C.BAD_ROWS.items() if s == "trailing"] == [1, 1, 3, 3]


def test_lengths_and_lane_counts():
    for pat in C.PATTERNS:
        case = next(c for c in C.VALID if c.name == f"lengths/{pat}")
        assert tuple(r.n for r in case.rows) == C.LENGTHS
    assert C.LENGTHS == (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 1007, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073)
    lengths = [c for c in C.VALID if c.cls == "lengths"]
    # the last lane with samples: every nv, in a first step and in a third one; one key byte (nv <= 8) and two (9 .. 15)
    last_nv = {}
    for c, r, rp, k, s in _steps(lengths):
        if k == len(rp.steps) - 1:
            last_nv.setdefault(k, set()).add([v for v in s.nv if v][-1])
    assert last_nv[0] == set(range(1, 17)) and last_nv[2] == set(range(1, 17))
    # prefetches: a row of 1024 asks for nothing ahead, 1025 for data, 2049 for keys two steps ahead
    ahead = {r.n: tuple((s.data_ahead, s.keys_ahead) for s in rp.steps) for c, r, rp, k, s in _steps(lengths)}
    assert ahead[1024] == ((False, False),) and ahead[1025] == ((True, False), (False, False))
    assert ahead[2048] == ahead[1025] and ahead[2049] == ((True, True), (True, False), (False, False)) and len(ahead[3073]) == 4
    # lanes without samples in a step that others decode, and rows without steps
    assert any("none" in s.path and "scalar" in s.path for c, r, rp, k, s in _steps(lengths))
    assert all(len(rp.steps) == (r.n + C.STEP - 1) // C.STEP for c in C.VALID for r, rp in zip(c.rows, _plan(c).rows))


def test_key_patterns_at_every_multi_step_length():
    assert C.MULTI_STEP == (1025, 2047, 2048, 2049, 3072, 3073)
    for pat in C.PATTERNS:
        case = next(c for c in C.VALID if c.name == f"lengths/{pat}")
        for r in case.rows:
            wide = C.zigzag_of(r.samples) > 0xFF
            i = np.arange(r.n)
            want = {"one": i < 0, "two": i >= 0, "alt": i % 2 == 1, "last16": i % 16 == 15, "lane0": i % 16 == 0, "first": i == 0}.get(pat)
            if want is not None:
                assert np.array_equal(wide, want), (pat, r.n)
            elif r.n > C.STEP:
                share = wide.mean()
                assert abs(share - int(pat[1:]) / 100) < 0.05, (pat, r.n, share)
            keys = np.unpackbits(np.frombuffer(r.data, np.uint8)[: (r.n + 7) // 8], bitorder="little")[: r.n]
            assert np.array_equal(keys, wide)   # canonical: the keys are the pattern


def test_every_mis_in_a_first_and_in_a_later_step():
    want = {(m, later) for m in range(4) for later in (False, True)}
    by_rows = {(s.mis, k > 0) for c, r, rp, k, s in _steps([c for c in C.VALID if c.cls == "align"])}
    by_pointer = {(s.mis, k > 0) for c, r, rp, k, s in _steps([c for c in C.VALID if c.cls == "pointers"], as_built=(True,))}
    assert by_rows == want and by_pointer == want
    assert {c.svb_mod4 for c in C.VALID if c.cls == "pointers"} == {0, 1, 2, 3}


def test_every_output_residue_for_a_row_of_two_full_steps():
    by_rows = {rp.out_res for c, r, rp, k, s in _steps([c for c in C.VALID if c.name.startswith("align/out")]) if r.n >= 2 * C.STEP}
    by_pointer = {rp.out_res for c, r, rp, k, s in _steps([c for c in C.VALID if c.cls == "pointers"], as_built=(True,))
                  if r.n >= 2 * C.STEP}
    assert by_rows == by_pointer == set(range(8))
    # residue 0 takes the vector store in every full lane, every other residue in none
    for c, r, rp, k, s in _steps():
        assert all((p == "vector") == (v == C.PER and rp.out_res == 0) for p, v in zip(s.path, s.nv))


def test_the_vector_store_under_every_key_pattern_and_value_class():
    tags = {}
    for c, r, rp, k, s in _steps():
        if "vector" in s.path:
            tags.setdefault(r.tag, set()).add(k)
    for tag in C.PATTERNS + ("ramp+32767", "zero-step-sum", "uniform", "delta0", "delta-1", "delta-32768", "forced", "forced-all", "pad"):
        assert tags.get(tag, set()) >= {0, 1}, tag   # in a first step and in one that a carry enters
    # the carries that enter those steps: large under the ramp, zero by construction, anything otherwise
    vec = next(c for c in C.VALID if c.name == "align/vector")
    carries = {r.tag: [s.carry for s in rp.steps] for r, rp in zip(vec.rows, _plan(vec).rows)}
    assert carries["ramp+32767"] == [0, 64512, 63488] and carries["zero-step-sum"] == [0, 0]
    assert carries["two"][1] != 0 and carries["p50"][1] != 0 and carries["uniform"][1] != 0
    # the same values with partial lanes and four steps
    val = next(c for c in C.VALID if c.name == "values/3073")
    carries = {r.tag: [s.carry for s in rp.steps] for r, rp in zip(val.rows, _plan(val).rows)}
    assert carries["ramp+32767"] == [0, 64512, 63488, 62464] and carries["zero-step-sum"] == [0, 0, 0, 0]
    assert carries["delta-1"] == [0, 64512, 63488, 62464] and carries["delta0"] == [0, 0, 0, 0] and carries["delta-32768"] == [0, 0, 0, 0]
    assert set(C.zigzag_of(val.rows[3].samples)) == {0xFFFF}
    # a carry is the sample before the step
    for c, r, rp, k, s in _steps():
        assert s.carry == (int(r.samples[k * C.STEP - 1]) & 0xFFFF if k else 0)


def test_the_largest_step():
    most = C.STEP * 2 // 4 + 1
    hits = {(c.name, as_built) for as_built in (False, True) for c, r, rp, k, s in _steps(as_built=(as_built,)) if s.dwords == most}
    assert hits >= {("align/513-dwords", False), ("pointers/513-dwords", True)}   # built for it: by a filler of 3 bytes, by the pointer
    for name in ("align/513-dwords", "pointers/513-dwords"):
        c = next(c for c in C.VALID if c.name == name)
        s, = _plan(c, True).rows[-1].steps
        assert (c.rows[-1].n, s.mis, s.total, s.dwords) == (C.STEP, 3, 2 * C.STEP, most)
    for c, r, rp, k, s in _steps():
        assert s.dwords == (s.mis + s.total + 3) >> 2 <= most
    for c in C.VALID:   # the steps' bytes are the row's
        for r, rp in zip(c.rows, _plan(c).rows):
            assert sum(s.total for s in rp.steps) == len(r.data) - (r.n + 7) // 8


def test_batch_shapes():
    shape = {c.name: c for c in C.VALID if c.cls == "shape"}
    assert [len(shape[f"shape/{k}-rows"].rows) for k in (1, 2, 3, 4, 5, 8)] == [1, 2, 3, 4, 5, 8]
    assert [r.n for r in shape["shape/uneven-block"].rows] == [1, 3073, 0, 17]
    assert {rp.block for rp in _plan(shape["shape/uneven-block"]).rows} == {0}
    ns = [r.n for r in shape["shape/empty-rows"].rows]
    assert ns[0] == ns[-1] == 0 and 0 in ns[1:-1] and any(ns) and all(len(r.data) == 0 for r in shape["shape/empty-rows"].rows if r.n == 0)
    big = shape["shape/1001-rows"]
    assert len(big.rows) == 1001 and {r.n for r in big.rows} == set(range(1, 41))
    p = _plan(big)
    assert [(rp.block, rp.wave) for rp in p.rows] == [(i // 4, i % 4) for i in range(1001)] and p.rows[-1][:2] == (250, 0)
    assert {len(c.rows) % 4 for c in C.VALID} == {0, 1, 2, 3}


def test_non_canonical_streams():
    forced = next(c for c in C.VALID if c.name == "noncanon/forced-two-byte")
    n_forced = 0
    for r in forced.rows:
        keys = np.unpackbits(np.frombuffer(r.data, np.uint8)[: (r.n + 7) // 8], bitorder="little")[: r.n]
        assert not (C.zigzag_of(r.samples) > 0xFF).any()   # every value fits one byte
        n_forced += int(keys.sum())
        assert len(r.data) == (r.n + 7) // 8 + r.n + int(keys.sum())
    assert n_forced > 5000
    pad = next(c for c in C.VALID if c.name == "noncanon/pad-bits")
    assert [r.n for r in pad.rows] == [2049] + [n for n in C.LENGTHS for _ in range(2)]
    for r in pad.rows:
        if r.n % 8:
            assert np.frombuffer(r.data, np.uint8)[(r.n + 7) // 8 - 1] >> (r.n % 8) == 0xFF >> (r.n % 8)
    assert sum(r.n % 8 != 0 and r.n % 16 < 8 for r in pad.rows) > 4 and sum(r.n % 16 > 8 for r in pad.rows) > 4   # in either key byte


def test_what_test_vbz_decode_kernel_reaches():
    """The gap that vbz_cases.py closes, as plan() sees it on the row list of test_gpu_parity.py::test_vbz_decode_kernel."""
    rows = C.parity_test_rows()
    p = C.plan([(r.data, r.n) for r in rows])
    assert [r.n for r in rows] == [1, 7, 8, 9, 255, 2048, 2049, 4096, 40000, 102400, 150001, 5000, 5000, 9000]
    assert [rp.out_res for rp in p.rows] == [0, 1, 0, 0, 1, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    vector_rows = [i for i, rp in enumerate(p.rows) if any("vector" in s.path for s in rp.steps)]
    assert vector_rows == [5, 6]   # the rows of 2048 and 2049 samples
    wide = [C.zigzag_of(r.samples) > 0xFF for r in rows]
    assert all(w[0] and not w[1:].any() for w in wide[:11]) and not wide[11].any()   # one byte per delta after the first sample
    # rows 12 (deltas 0 and +-20000: half of them fit one byte) and 13 (a few of its deltas do) mix the two codings inside a
    # step, but on scalar stores alone: the vector store sees one-byte deltas only
    assert 0.4 < wide[12].mean() < 0.6 and 0 < (~wide[13]).sum() < 100
    assert not any("vector" in s.path for i in (12, 13) for s in p.rows[i].steps)
    assert len(rows) % 4 == 2 and all(r.n > 0 for r in rows)
    assert not {15, 16, 17, 1023, 1024, 1025} & {r.n for r in rows}
    # its corrupt input (three bytes off the end of row 4, as row 1 of 2) never reaches a kernel check
    bad = C.plan([(rows[0].data, rows[0].n), (rows[4].data[:-3], rows[4].n)])
    assert (bad.site, bad.row) == ("api", 1)
