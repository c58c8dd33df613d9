"""The case lists of tests/test_gpu_vbz_paths.py: small signal rows that take, one path each, every route through
vbz_decode_kernel (remora_amd/csrc/k_vbz.hip, behind rmr_vbz_decode), the encoder that makes them, and plan(), which restates
the kernel's control flow on the CPU and so shows which route a row takes.

What decides a row's route, restated from the kernel file and from rmr_vbz_decode (remora_amd/csrc/api_data.hip):
  * row r is decoded by wave r % 4 of block r // 4 (kVbzWaves = 4), alone, in steps of 1024 samples (kVbzStep), lane l of a
    step owning samples 16 l .. 16 l + 15 (kVbzPer = 16) and the two key bytes that belong to them;
  * a lane with nv of its 16 samples inside the row loads one key byte when nv <= 8 and two otherwise, and masks them to nv bits;
  * a step's `total` data bytes start `mis` = address & 3 bytes into an aligned dword; (mis + total + 3) >> 2 dwords are staged
    in the wave's LDS slice of 1024 * 2 / 4 + 4 = 516 dwords;
  * while step k is decoded the data of step k + 1 and the keys of step k + 2 are requested, when those steps exist;
  * a lane stores its samples as two 16-byte vectors when nv == 16 and its destination is 16-byte aligned, one by one otherwise;
  * the running sum of the steps before (mod 2^16) enters a step as `carry`;
  * a row is refused by the API before any launch ("api": fewer bytes than ceil(n / 8) + n, bytes but no samples, n < 0,
    decreasing row_off), by the
    kernel before its first step ("first": the keys of step 0 ask for more bytes than the row has), before a later step
    ("prefetch": the keys of step k + 1 do, seen while step k waits in LDS: steps 0 .. k - 1 are stored by then) or after its
    last step ("trailing": bytes are left over; the whole row is stored by then).

tests/test_host_vbz_cases.py asserts, without a GPU, that the oracle decodes every valid case to the samples that were encoded,
refuses every corrupt one, and that plan() finds every class below populated; the GPU test then runs every case.

A plain module (no tests in it), like refine_cases.py, data_cases.py and stream_cases.py."""
from collections import namedtuple

import numpy as np

WAVES = 4            # kVbzWaves: rows per workgroup
PER = 16             # kVbzPer: samples per lane and step
STEP = 64 * PER      # kVbzStep
LDS_DWORDS = STEP * 2 // 4 + 4   # a wave's LDS slice (sdata_all[wave])
SLACK = 16           # bytes io.py leaves behind the last row for the kernel's whole-dword reads


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------
def zigzag_of(samples):
    """int16 samples -> the zigzag-coded wrapping deltas (0 .. 0xFFFF) that the stream carries."""
    sig = np.asarray(samples, np.int16)
    d = np.diff(np.concatenate([[0], sig.astype(np.int64)])).astype(np.int16)  # wraps like the decoder's sum
    return ((d.astype(np.int32) << 1) ^ (d.astype(np.int32) >> 15)).astype(np.uint32) & 0xFFFF


def encode(samples, two=None, pad_bits=0):
    """Test-side encoder of the VBZ layer below zstd: int16 samples -> deltas -> zigzag -> streamvbyte16.  `two` (bool per
    sample) forces the two-byte coding on values that fit one byte (non-canonical, valid); `pad_bits` is OR-ed into the unused
    high bits of the last key byte."""
    zz = zigzag_of(samples)
    wide = zz > 0xFF
    if two is not None:
        wide = wide | np.asarray(two, bool)
    keys = np.packbits(wide, bitorder="little")
    if pad_bits and zz.size % 8:
        keys[-1] |= (int(pad_bits) << (zz.size % 8)) & 0xFF
    data = np.empty(zz.size + int(wide.sum()), np.uint8)
    offs = np.cumsum(wide + 1) - (wide + 1)
    data[offs] = zz & 0xFF
    data[offs[wide] + 1] = zz[wide] >> 8
    return keys.tobytes() + data.tobytes()


def samples_of_zigzag(zz):
    """The int16 samples whose stream carries exactly these zigzag values."""
    zz = np.asarray(zz, np.int64)
    d = (zz >> 1) ^ -(zz & 1)
    return np.cumsum(d).astype(np.int16)   # int64 sum, low 16 bits: the decoder's wrap


# ---- plan(): the kernel's control flow without its arithmetic --------------------------------------------------------------------------
StepPlan = namedtuple("StepPlan", "mis total dwords keys_ahead data_ahead nv path carry")
RowPlan = namedtuple("RowPlan", "block wave n out_res steps refusal stored")   # refusal: None or a site; stored: steps written
Plan = namedtuple("Plan", "site row rows")   # site: None, "api", "first", "prefetch", "trailing"; row: the first refused row

SITES = ("api", "first", "prefetch", "trailing")


def _row_plan(r, raw, n, addr_mod4, out_res):
    block, wave = r // WAVES, r % WAVES
    if n <= 0:
        return RowPlan(block, wave, n, out_res, (), None, 0)   # the wave returns before it reads anything
    raw = np.frombuffer(raw, np.uint8)
    nkeys = (n + 7) // 8
    avail = raw.size - nkeys
    nsteps = (n + STEP - 1) // STEP
    bits = np.zeros(nsteps * STEP, np.int64)
    bits[:n] = np.unpackbits(raw[:nkeys], bitorder="little")[:n]   # masked to the samples of the row, like `k &= ...`
    nv = np.clip(n - np.arange(nsteps * 64) * PER, 0, PER).reshape(nsteps, 64)
    totals = (nv + bits.reshape(nsteps, 64, PER).sum(2)).sum(1)
    data = raw[nkeys:]
    steps, refusal, data_pos, carry = [], None, 0, 0
    if totals[0] > avail:
        return RowPlan(block, wave, n, out_res, (), "first", 0)
    for k in range(nsteps):
        more = (k + 1) * STEP < n
        if more and data_pos + totals[k] + totals[k + 1] > avail:
            refusal = "prefetch"
            break
        total = int(totals[k])
        mis = (addr_mod4 + nkeys + data_pos) % 4
        path = tuple("none" if v == 0 else "vector" if v == PER and (out_res + k * STEP + PER * lane) % 8 == 0 else "scalar"
                     for lane, v in enumerate(nv[k]))
        steps.append(StepPlan(mis, total, (mis + total + 3) >> 2, (k + 2) * STEP < n, more, tuple(int(v) for v in nv[k]), path, carry))
        # the step's sum, for the carry that enters the next one (its bytes are inside the row: the checks above saw to that)
        cnt = min(STEP, n - k * STEP)
        b = bits[k * STEP : k * STEP + cnt]
        offs = data_pos + np.cumsum(b + 1) - (b + 1)
        zz = data[offs].astype(np.int64) | np.where(b == 1, data[np.minimum(offs + 1, data.size - 1)].astype(np.int64) << 8, 0)
        carry = int((carry + ((zz >> 1) ^ -(zz & 1)).sum()) & 0xFFFF)
        data_pos += total
    else:
        if data_pos != avail:
            refusal = "trailing"
    return RowPlan(block, wave, n, out_res, tuple(steps), refusal, len(steps))


def plan(rows, svb_mod4=0, out_mod8=0, row_off=None):
    """What rmr_vbz_decode and vbz_decode_kernel do with `rows` = [(bytes, n)] laid back to back, `svb` being svb_mod4 bytes
    past a dword boundary and `out` out_mod8 samples past a 16-byte boundary: a Plan.  An explicit row_off is taken for the
    API's pre-check alone, which then has to refuse it (the kernel is never launched on offsets that disagree with the bytes)."""
    sizes = [len(b) for b, _ in rows]
    explicit = row_off is not None
    if not explicit:
        row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    for r, (_, n) in enumerate(rows):
        size = int(row_off[r + 1] - row_off[r])
        if n < 0 or size < 0 or size < (n + 7) // 8 + n or (n == 0 and size):
            return Plan("api", r, ())
    if explicit:
        raise ValueError("plan() follows an explicit row_off only as far as the API's refusal")
    out, out_at = [], 0
    for r, (raw, n) in enumerate(rows):
        out.append(_row_plan(r, raw, n, (svb_mod4 + int(row_off[r])) % 4, (out_mod8 + out_at) % 8))
        out_at += n
    bad = [r for r, p in enumerate(out) if p.refusal]
    return Plan(out[bad[0]].refusal if bad else None, bad[0] if bad else None, tuple(out))


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
Row = namedtuple("Row", "samples data n tag")   # samples: what a decoder must return (for a refused row: what the bytes hold)

PATTERNS = ("one", "two", "p10", "p50", "p90", "alt", "last16", "lane0", "first")


def key_mask(pattern, n, rng):
    """Which samples of a row of n take two bytes: all / none, a random share, every other one, sample 15 of every lane (the
    `sb[pj + 1]` read at a lane's last byte), sample 0 of every lane, sample 0 of the row."""
    i = np.arange(n)
    if pattern in ("one", "two"):
        return np.full(n, pattern == "two")
    if pattern[0] == "p":
        return rng.random(n) < int(pattern[1:]) / 100
    return {"alt": i % 2 == 1, "last16": i % PER == PER - 1, "lane0": i % PER == 0, "first": i == 0}[pattern]


def pattern_row(pattern, n, seed):
    rng = np.random.default_rng(seed)
    mask = key_mask(pattern, n, rng)
    zz = np.where(mask, rng.integers(0x100, 0x10000, n), rng.integers(0, 0x100, n))
    s = samples_of_zigzag(zz)
    return Row(s, encode(s), n, pattern)


def value_row(samples, tag, **kw):
    s = np.asarray(samples, np.int16)
    return Row(s, encode(s, **kw), int(s.size), tag)


def _const_delta(d, n):
    return (np.arange(1, n + 1, dtype=np.int64) * d).astype(np.int16)


def zero_step_sum_row(n, seed):
    """Random deltas, the last one of every step of 1024 chosen so that the step sums to 0 mod 2^16."""
    rng = np.random.default_rng(seed)
    d = rng.integers(-32768, 32768, n)
    for s0 in range(0, n, STEP):
        e = min(s0 + STEP, n) - 1
        d[e] = 0
        d[e] = ((-int(d[s0 : e + 1].sum()) + 32768) % 65536) - 32768
    return value_row(np.cumsum(d).astype(np.int16), "zero-step-sum")


EMPTY = Row(np.zeros(0, np.int16), b"", 0, "empty")

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 1007, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073)
MULTI_STEP = tuple(n for n in LENGTHS if n > STEP)
LONGEST = 3 * STEP + 1

Case = namedtuple("Case", "name cls rows svb_mod4 out_mod8 row_off site bad arg_error")


def _case(name, cls, rows, svb_mod4=0, out_mod8=0, row_off=None, site=None, bad=None, arg_error=False):
    return Case(name, cls, tuple(rows), svb_mod4, out_mod8, row_off, site, bad, arg_error)


def _filler(n):
    """n samples of one byte each: ceil(n / 8) + n bytes, n samples of output."""
    return value_row(np.full(n, 3, np.int16) if n else np.zeros(0, np.int16), f"filler{n}")


def _valid_cases():
    cases = []
    # lengths: every length under every key pattern, one call per pattern; then every nv of a last lane, short and in a third step
    for pi, pat in enumerate(PATTERNS):
        cases.append(_case(f"lengths/{pat}", "lengths", [pattern_row(pat, n, 100 * pi + i) for i, n in enumerate(LENGTHS)]))
    cases.append(_case("lengths/last-lane", "lengths", [pattern_row("p50", base + k, 1000 + base + k) for base in (0, 2 * STEP)
                                                        for k in range(1, PER + 1)]))
    # values
    n = LONGEST
    rng = np.random.default_rng(77)
    cases.append(_case("values/3073", "values", [
        value_row(np.zeros(n, np.int16), "delta0"), value_row(_const_delta(-1, n), "delta-1"),
        value_row(_const_delta(32767, n), "ramp+32767"), value_row(_const_delta(-32768, n), "delta-32768"),
        zero_step_sum_row(n, 5), value_row(rng.integers(-32768, 32768, n), "uniform")]))
    cases.append(_case("values/17", "values", [
        value_row(np.zeros(17, np.int16), "delta0"), value_row(_const_delta(-1, 17), "delta-1"),
        value_row(_const_delta(32767, 17), "ramp+32767"), value_row(_const_delta(-32768, 17), "delta-32768"),
        value_row(rng.integers(-32768, 32768, 17), "uniform")]))
    # alignment by the rows in front: the output residue (a filler of r samples), mis (fillers of 2, 3, 4 and 5 bytes)
    for r in range(8):
        cases.append(_case(f"align/out{r}", "align", ([_filler(r)] if r else []) + [pattern_row("p50", 2 * STEP + 1, 200 + r)]))
    for f in range(1, 5):
        cases.append(_case(f"align/mis-after-{f + 1}-bytes", "align", [_filler(f), pattern_row("p50", 2 * STEP + 1, 210 + f),
                                                                       pattern_row("p10", STEP + 1, 220 + f)]))
    # the vector store under every key pattern and under wrapping sums: rows whose lengths are multiples of 8 keep every row aligned
    cases.append(_case("align/vector", "align", [pattern_row(pat, 2 * STEP, 300 + i) for i, pat in enumerate(PATTERNS)]
                       + [value_row(_const_delta(32767, 3 * STEP), "ramp+32767"), zero_step_sum_row(2 * STEP, 6),
                          value_row(np.zeros(2 * STEP, np.int16), "delta0"), value_row(_const_delta(-1, 2 * STEP), "delta-1"),
                          value_row(_const_delta(-32768, 2 * STEP), "delta-32768"),
                          value_row(np.random.default_rng(78).integers(-32768, 32768, 2 * STEP), "uniform")]))
    # the most a step can stage: 1024 two-byte samples that begin 3 bytes into a dword (a filler of 3 bytes in front)
    cases.append(_case("align/513-dwords", "align", [_filler(2), pattern_row("two", STEP, 400)]))
    # the same through the pointers themselves (the device-pointer entry applies the offsets; the others run the rows as they are)
    for r in range(8):
        cases.append(_case(f"pointers/out{r}-svb{r % 4}", "pointers", [pattern_row("p50", 2 * STEP + 1, 500 + r),
                                                                       pattern_row("two", 2 * STEP, 510 + r), pattern_row("p90", 17, 520 + r)],
                           svb_mod4=r % 4, out_mod8=r))
    cases.append(_case("pointers/513-dwords", "pointers", [pattern_row("two", STEP, 401)], svb_mod4=3))
    # batch shapes
    short = [pattern_row("p50", n, 600 + n) for n in (17, 5, 33, 1, 40, 9, 16, 1025)]
    for k in (1, 2, 3, 4, 5, 8):
        cases.append(_case(f"shape/{k}-rows", "shape", short[:k]))
    cases.append(_case("shape/uneven-block", "shape", [pattern_row("p50", 1, 700), pattern_row("p50", LONGEST, 701), EMPTY,
                                                       pattern_row("p50", 17, 702)]))
    cases.append(_case("shape/empty-rows", "shape", [EMPTY, pattern_row("p50", 17, 710), EMPTY, EMPTY, pattern_row("p10", STEP + 1, 711),
                                                     pattern_row("two", 9, 712), EMPTY]))
    cases.append(_case("shape/only-empty-rows", "shape", [EMPTY, EMPTY, EMPTY]))
    rng = np.random.default_rng(79)
    cases.append(_case("shape/1001-rows", "shape", [pattern_row("p50", int(n), 2000 + i) for i, n in enumerate(rng.integers(1, 41, 1001))]))
    # non-canonical but valid: two-byte codings of values below 256, padding bits set in the last key byte
    forced = [value_row(np.zeros(2 * STEP, np.int16), "forced-all", two=np.ones(2 * STEP, bool))]   # aligned: the vector store
    for i, n in enumerate((2 * STEP,) + LENGTHS):
        rng = np.random.default_rng(800 + i)
        s = samples_of_zigzag(rng.integers(0, 0x100, n))
        forced.append(value_row(s, "forced", two=rng.random(n) < 0.5))
    cases.append(_case("noncanon/forced-two-byte", "noncanon", forced))
    cases.append(_case("noncanon/pad-bits", "noncanon", [Row(r.samples, encode(r.samples, pad_bits=0xFF), r.n, "pad") for r in
                                                         [pattern_row("p50", 2 * STEP + 1, 899)]
                                                         + [pattern_row(pat, n, 900 + n) for n in LENGTHS for pat in ("one", "p50")]]))
    return tuple(cases)


VALID = _valid_cases()
SHUFFLED = ("lengths/p50", "shape/uneven-block", "shape/empty-rows", "shape/1001-rows", "align/vector")   # order independence


# ---- corrupt rows ----------------------------------------------------------------------------------------------------------------------
def _cut(row, nbytes, tag):
    return Row(row.samples, row.data[:nbytes], row.n, tag)


def _step_bytes(row):
    """Data bytes of each step of a row."""
    wide = zigzag_of(row.samples) > 0xFF
    return [int((wide[s0 : s0 + STEP] + 1).sum()) for s0 in range(0, row.n, STEP)]


def _bad_rows():
    nk = lambda n: (n + 7) // 8  # noqa: E731
    one40, two40 = pattern_row("one", 40, 3000), pattern_row("two", 40, 3001)
    r2049 = pattern_row("p50", 2 * STEP + 1, 3002)
    t = _step_bytes(r2049)
    r100, r3000 = pattern_row("p50", 100, 3003), pattern_row("p50", 3000, 3004)
    bad = {
        "short": ("api", _cut(one40, nk(40) + 40 - 1, "short")),                          # fewer bytes than nkeys + n
        "keys-ask-more": ("first", _cut(two40, nk(40) + 40 + 3, "keys-ask-more")),         # the pre-check is content; the keys want 80
        "short-in-step1": ("prefetch", _cut(r2049, nk(2049) + t[0] + t[1] - 1, "short-in-step1")),
        "short-in-step2": ("prefetch", _cut(r2049, len(r2049.data) - 1, "short-in-step2")),
    }
    bad["bytes-without-samples"] = ("api", Row(EMPTY.samples, bytes([0, 7, 9]), 0, "bytes-without-samples"))   # no kernel check sees it
    for name, row in (("1step", r100), ("3steps", r3000)):
        for extra in (1, 5):
            bad[f"extra{extra}-{name}"] = ("trailing", Row(row.samples, row.data + bytes(range(7, 7 + extra)), row.n, "extra"))
    return bad


BAD_ROWS = _bad_rows()
GOOD_ROWS = (pattern_row("p50", 17, 3100), pattern_row("p10", STEP + 1, 3101), pattern_row("two", 9, 3102),
             pattern_row("p90", 2 * STEP, 3103), pattern_row("one", 33, 3104))
POSITIONS = (0, 2, 4)   # first, a middle one, last of five


def _corrupt_cases():
    cases = []
    for kind, (site, row) in BAD_ROWS.items():
        for at in POSITIONS:
            rows = list(GOOD_ROWS)
            rows[at] = row
            cases.append(_case(f"corrupt/{kind}@{at}", "corrupt", rows, svb_mod4=at % 4, out_mod8=at, site=site, bad=at))
    for at in POSITIONS:
        rows = list(GOOD_ROWS)
        rows[at] = Row(rows[at].samples, rows[at].data, -1, "negative-n")
        cases.append(_case(f"corrupt/negative-n@{at}", "corrupt", rows, site="api", bad=at, arg_error=True))
        sizes = [len(r.data) for r in GOOD_ROWS]
        off = 8 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)   # 8 bytes in front, so that row 0 can end before it begins
        off[at + 1] = off[at] - 1
        cases.append(_case(f"corrupt/decreasing-row-off@{at}", "corrupt", GOOD_ROWS, row_off=off, site="api", bad=at, arg_error=True))
    # two refused rows in one call: the error names the first
    rows = list(GOOD_ROWS)
    rows[1], rows[3] = BAD_ROWS["extra1-1step"][1], BAD_ROWS["keys-ask-more"][1]
    cases.append(_case("corrupt/two-bad-rows", "corrupt", rows, site="trailing", bad=1))
    return tuple(cases)


CORRUPT = _corrupt_cases()


def pairs(case):
    """[(bytes, n)] of a case, as plan() takes them."""
    return [(r.data, r.n) for r in case.rows]


def written(case, p):
    """The samples a refused call may leave in `out`, row by row (None: the row's span is untouched), given its plan: nothing at
    all when the API refuses; otherwise every good row whole, and of a refused row the steps stored before its check fired."""
    if p.site == "api":
        return [None] * len(case.rows)
    return [r.samples[: min(r.n, rp.stored * STEP)] if rp.refusal else r.samples for r, rp in zip(case.rows, p.rows)]


# ---- the row list of test_gpu_parity.py::test_vbz_decode_kernel ----------------------------------------------------------------------------
def parity_test_rows():
    """The synthetic rows of test_vbz_decode_kernel, in its order, from its seed."""
    rng = np.random.default_rng(8)
    rows = []
    for n in (1, 7, 8, 9, 255, 2048, 2049, 4096, 40000, 102400, 150001):
        walk = np.cumsum(rng.integers(-40, 41, n)) + 500
        rows.append(walk.astype(np.int16))
    rows.append(np.full(5000, 77, np.int16))
    rows.append((rng.integers(0, 2, 5000) * 20000 - 10000).astype(np.int16))
    rows.append(np.cumsum(rng.integers(-30000, 30000, 9000)).astype(np.int16))
    return [value_row(r, f"parity{i}") for i, r in enumerate(rows)]
