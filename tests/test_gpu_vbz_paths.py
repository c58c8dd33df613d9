"""vbz_decode_kernel (remora_amd/csrc/k_vbz.hip) on every path its waves can take: every case of tests/vbz_cases.py through
rmr_vbz_decode with host pointers, with device pointers (offset by the case's 0..3 bytes and 0..7 samples, between sentinel
guards) and through io.vbz_decode_batch, each compared byte for byte with the samples that were encoded; every corrupt case
refused with the index of its first bad row, with everything the call may have written accounted for; the same rows in
another order.

tests/test_host_vbz_cases.py shows on the CPU that each case has the property it is used for here (which store, which mis,
which refusal site), and that the oracle decodes what the encoder of vbz_cases.py made.  No case is left out: every function
below walks the whole of C.VALID or C.CORRUPT."""
import ctypes
import re

import numpy as np
import pytest

import vbz_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -21846   # 0xAAAA
GUARD = 64          # samples in front of and behind `out` that a call must leave alone
CLASSES = ("lengths", "values", "align", "pointers", "shape", "noncanon")


@pytest.fixture(scope="module", autouse=True)
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def eng():
    from remora_amd.engine import get_engine

    return get_engine(0)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _layout(rows, row_off=None):
    """(svb bytes with the slack io.py leaves, row_off, row_samples, out_off) of rows laid back to back."""
    sizes = [len(r.data) for r in rows]
    if row_off is None:
        row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        body = b"".join(r.data for r in rows)
    else:
        body = bytes(int(row_off[0])) + b"".join(r.data for r in rows)   # explicit offsets: the rows begin where the first one says
    buf = np.zeros(len(body) + C.SLACK, np.uint8)
    buf[: len(body)] = np.frombuffer(body, np.uint8)
    rn = np.asarray([r.n for r in rows], np.int32)
    out_off = np.concatenate([[0], np.cumsum(np.maximum(rn, 0))]).astype(np.int64)
    return buf, np.ascontiguousarray(row_off, np.int64), rn, out_off


def _decode_host(eng, rows, row_off=None):
    """rmr_vbz_decode on host arrays -> the whole of `out`, guards included (the copy back must stay inside sum(n) too)."""
    from remora_amd import _lib as L

    buf, ro, rn, oo = _layout(rows, row_off)
    out = np.full(int(oo[-1]) + 2 * GUARD, SENTINEL, np.int16)
    L.check(L.lib().rmr_vbz_decode(eng.handle, _p(buf), _p(ro), _p(rn), len(rows), _p(out[GUARD:]), L.MEM_HOST))
    return out, oo


def _decode_device(torch, eng, rows, svb_mod4=0, out_mod8=0, row_off=None):
    """rmr_vbz_decode on device arrays, `svb` svb_mod4 bytes past torch's alignment and `out` GUARD + out_mod8 samples past it
    -> (the whole output allocation as numpy, out_off, the error or None).  The allocation is returned after a refusal too."""
    from remora_amd import RemoraError
    from remora_amd import _lib as L

    buf, ro, rn, oo = _layout(rows, row_off)
    dev = eng.torch_device
    d_buf = torch.from_numpy(np.concatenate([np.zeros(svb_mod4, np.uint8), buf])).to(dev)
    d_ro, d_rn = torch.from_numpy(ro).to(dev), torch.from_numpy(rn).to(dev)
    d_out = torch.full((GUARD + out_mod8 + int(oo[-1]) + GUARD,), SENTINEL, dtype=torch.int16, device=dev)
    assert d_buf.data_ptr() % 4 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()   # the copies and the fill ran on torch's stream, the kernel runs on the engine's own
    err = None
    try:
        L.check(L.lib().rmr_vbz_decode(eng.handle, d_buf.data_ptr() + svb_mod4, d_ro.data_ptr(), d_rn.data_ptr(), len(rows),
                                       d_out.data_ptr() + 2 * (GUARD + out_mod8), L.MEM_DEVICE))
    except RemoraError as e:
        err = e
    eng.synchronize()
    return d_out.cpu().numpy(), oo, err


def _decode_io(eng, rows):
    import pyarrow as pa

    from remora_amd import io as rio

    blobs = [pa.compress(r.data, codec="zstd", asbytes=True) for r in rows]
    flat, off = rio.vbz_decode_batch(blobs, [r.n for r in rows], engine=eng, to_host=False)
    return flat.cpu().numpy(), off


def _expected(rows, oo, lead, written=None):
    """The output allocation a call must leave: sentinels, and each row's samples (or what `written` says of it) in its span."""
    want = np.full(lead + int(oo[-1]) + GUARD, SENTINEL, np.int16)
    for i, r in enumerate(rows):
        s = r.samples if written is None else written[i]
        if s is not None:
            want[lead + int(oo[i]) : lead + int(oo[i]) + s.size] = s
    return want


def _check(got, want, rows, oo, lead, what):
    if got.tobytes() == want.tobytes():
        return
    at = int(np.flatnonzero(got != want)[0]) - lead
    row = int(np.searchsorted(oo, at, side="right")) - 1
    where = "the guard in front" if at < 0 else "the guard behind" if at >= oo[-1] else f"row {row} ({rows[row].tag}, n = {rows[row].n}) sample {at - int(oo[row])}"
    raise AssertionError(f"{what}: first difference in {where}: got {got[at + lead]}, want {want[at + lead]}; "
                         f"{int((got != want).sum())} samples differ")


ENTRIES = ("host", "device", "io")


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_valid_case_decodes_to_what_was_encoded(torch_cuda, eng, entry, cls):
    cases = [c for c in C.VALID if c.cls == cls]
    assert cases
    for c in cases:
        rows = c.rows
        if entry == "host":
            got, oo = _decode_host(eng, rows)
            _check(got, _expected(rows, oo, GUARD), rows, oo, GUARD, f"{c.name} host")
        elif entry == "device":
            lead = GUARD + c.out_mod8
            got, oo, err = _decode_device(torch_cuda, eng, rows, c.svb_mod4, c.out_mod8)
            assert err is None, (c.name, err)
            _check(got, _expected(rows, oo, lead), rows, oo, lead, f"{c.name} device svb+{c.svb_mod4} out+{c.out_mod8}")
        else:
            got, oo = _decode_io(eng, rows)
            assert got.dtype == np.int16 and got.size == oo[-1]
            _check(got, _expected(rows, oo, 0)[: got.size], rows, oo, 0, f"{c.name} io")


@pytest.mark.parametrize("out_mod8", range(8))
def test_every_pointer_offset_on_one_batch(torch_cuda, eng, out_mod8):
    """The rows of align/vector (every key pattern and value class, two and three full steps) with `out` at each of the eight
    residues and `svb` at each of the four: residue 0 stores vectors, the others the same samples one by one."""
    rows = next(c for c in C.VALID if c.name == "align/vector").rows
    for svb_mod4 in range(4):
        lead = GUARD + out_mod8
        got, oo, err = _decode_device(torch_cuda, eng, rows, svb_mod4, out_mod8)
        assert err is None
        _check(got, _expected(rows, oo, lead), rows, oo, lead, f"svb+{svb_mod4} out+{out_mod8}")


def _kinds():
    return sorted({c.name.split("@")[0] for c in C.CORRUPT})


@pytest.mark.parametrize("kind", _kinds())
def test_corrupt_rows_are_refused_and_nothing_else_is_touched(torch_cuda, eng, kind):
    """Every corrupt case raises with the index of its first bad row, through host and device pointers (and through
    io.vbz_decode_batch where the case can be put to it).  After the device-pointer call the whole output allocation is
    accounted for: the guards and the spans of rows the call never stored are sentinels, every good row holds its samples or
    (when the API refused before any launch) nothing, and a refused row holds exactly the steps that the kernel stores before
    the check that refuses it fires: none before the first-step check, those before the step whose prefetch fails, the whole
    row when bytes are left over.  Nothing lies outside a row's own span.  A valid call on the same engine then decodes."""
    from remora_amd import RemoraError

    cases = [c for c in C.CORRUPT if c.name.split("@")[0] == kind]
    assert cases
    good = next(c for c in C.VALID if c.name == "shape/uneven-block")
    for c in cases:
        msg = rf"corrupt VBZ signal block \(row {c.bad}\)"
        with pytest.raises(RemoraError, match=msg):
            _decode_host(eng, c.rows, c.row_off)
        got, oo, err = _decode_device(torch_cuda, eng, c.rows, c.svb_mod4, c.out_mod8, c.row_off)
        assert err is not None and re.search(msg, str(err)), (c.name, err)
        p = C.plan(C.pairs(c), c.svb_mod4, c.out_mod8, row_off=c.row_off)
        assert p.site == c.site
        lead = GUARD + c.out_mod8
        _check(got, _expected(c.rows, oo, lead, C.written(c, p)), c.rows, oo, lead, f"{c.name} after the refusal")
        if c.row_off is None:
            with pytest.raises(RemoraError, match=msg):
                _decode_io(eng, c.rows)
        # no state is left behind
        got, oo, err = _decode_device(torch_cuda, eng, good.rows)
        assert err is None
        _check(got, _expected(good.rows, oo, GUARD), good.rows, oo, GUARD, f"valid call after {c.name}")


@pytest.mark.parametrize("name", C.SHUFFLED)
def test_a_rows_result_depends_on_the_row_alone(torch_cuda, eng, name):
    """The rows of a batch in three other orders (other blocks, waves, byte and output alignments): the same bytes per row."""
    rows = next(c for c in C.VALID if c.name == name).rows
    base, oo = _decode_host(eng, rows)
    per_row = [base[GUARD + int(oo[i]) : GUARD + int(oo[i + 1])].tobytes() for i in range(len(rows))]
    assert per_row == [r.samples.tobytes() for r in rows]
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(len(rows)) if seed else np.arange(len(rows))[::-1]
        shuffled = [rows[i] for i in order]
        for entry in ("host", "device"):
            if entry == "host":
                got, so = _decode_host(eng, shuffled)
            else:
                got, so, err = _decode_device(torch_cuda, eng, shuffled)
                assert err is None
            for j, i in enumerate(order):
                assert got[GUARD + int(so[j]) : GUARD + int(so[j + 1])].tobytes() == per_row[i], (name, seed, entry, int(i))
            assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + int(so[-1]) :] == SENTINEL).all()
