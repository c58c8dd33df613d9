"""The read-id index of a POD5 dataset alone (rmr_read_index_create / _lookup / _destroy, csrc/k_read_index.hip) against a
Python dict over the same keys: which ids survive the build (of equal ids the one given first), what every name resolves to -
present ids in either letter case, absent ids around the present ones, every malformed text - at the sizes where the sort, the
scan and the launch grids change shape (one entry, one block of 256 and its neighbours, many blocks) and with keys that differ
in one word or one byte only."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _text(key):
    h = bytes(key).hex()
    return f"{h[:8]}-{h[8:12]}-{h[12:16]}-{h[16:20]}-{h[20:]}".encode()


def _mixed(t):
    return bytes(c - 32 if (97 <= c <= 102 and k % 2) else c for k, c in enumerate(t))


class _Index:
    def __init__(self, keys, values):
        from remora_amd import _lib as L
        from remora_amd.engine import get_engine

        self.L, self.lib, self.eng = L, L.lib(), get_engine(0)
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 16)
        values = np.ascontiguousarray(values, np.int64)
        self.h, nd = ctypes.c_void_p(), ctypes.c_int64(-7)
        L.check(self.lib.rmr_read_index_create(self.eng.handle, keys.ctypes.data_as(ctypes.c_void_p), values.ctypes.data_as(ctypes.c_void_p),
                                               keys.shape[0], ctypes.byref(self.h), ctypes.byref(nd)))
        self.n_distinct = nd.value

    def lookup(self, names):
        off = np.zeros(len(names) + 1, np.int64)
        np.cumsum([len(t) for t in names], out=off[1:])
        blob = b"".join(names)
        out = np.full(len(names), -99, np.int64)
        self.L.check(self.lib.rmr_read_index_lookup(self.h, blob, off.ctypes.data_as(ctypes.c_void_p), len(names),
                                                    out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def close(self):
        self.lib.rmr_read_index_destroy(self.h)
        self.h = None


def _keys(kind, n, rng):
    k = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    if kind == "equal":
        k[:] = k[0]
    elif kind == "low_shared":  # bytes 8-15, the word the first sort orders by, are the same everywhere
        k[:, 8:] = k[0, 8:]
    elif kind == "high_shared":
        k[:, :8] = k[0, :8]
    elif kind in ("byte0", "byte15"):
        k[:] = k[0]
        k[:, 0 if kind == "byte0" else 15] = rng.permutation(256)[:n]
    elif kind == "few":  # many entries over few ids, in no order
        k = k[rng.integers(0, 40, n)]
    return k


SHAPES = [("random", 0), ("random", 1), ("random", 2), ("equal", 2), ("random", 255), ("random", 256), ("random", 257), ("random", 100_003),
          ("low_shared", 4096), ("high_shared", 4096), ("byte0", 256), ("byte15", 256), ("equal", 1000), ("few", 257)]


def _neighbour(key, step):
    v = int.from_bytes(bytes(key), "big") + step
    return None if v < 0 or v >= 1 << 128 else v.to_bytes(16, "big")


@pytest.mark.parametrize("kind,n", SHAPES, ids=[f"{k}{n}" for k, n in SHAPES])
def test_build_and_lookup_equal_a_dict(kind, n):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    rng = np.random.default_rng(1000 + n)
    keys = _keys(kind, n, rng)
    values = rng.integers(0, 1 << 62, n, dtype=np.int64)
    want = {}
    for k, v in zip(map(bytes, keys), values.tolist()):
        want.setdefault(k, v)  # the entry given first survives
    ix, again = _Index(keys, values), _Index(keys, values)
    try:
        assert ix.n_distinct == len(want) == again.n_distinct
        present = sorted(want)
        names, expect = [], []
        for k in present:  # every present id, in the three spellings
            t = _text(k)
            for spelled in (t, t.upper(), _mixed(t)):
                names.append(spelled)
                expect.append(want[k])
        # absent ids: below the smallest, above the largest, between neighbours (one above / one below every 97th id)
        probes = present[::97] + present[-1:] if present else [bytes(16), bytes([255]) * 16, bytes(range(16))]
        for k in probes:
            for step in (-1, 1):
                other = _neighbour(k, step)
                if other is not None:
                    names.append(_text(other))
                    expect.append(want.get(other, -1))
        if present:
            assert _neighbour(present[0], -1) is None or want.get(_neighbour(present[0], -1)) is None
        # malformed texts made from a present id (or any id): only the flaw keeps them from resolving
        t = _text(present[len(present) // 2]) if present else _text(bytes(range(16)))
        flawed = [b"", t[:35], t + b"0", t[:3] + b"g" + t[4:], t[:35] + b"G", t[:7] + b"-" + t[7:8] + t[9:], t[:8] + t[9:10] + b"-" + t[10:],
                  b" " * 36, t.replace(b"-", b"0"), t[:20] + b"\x00" + t[21:], b"{" + t[1:], t[:-1] + b"`"]
        assert all(len(f) in (0, 35, 36, 37) for f in flawed)
        names.extend(flawed)
        expect.extend([-1] * len(flawed))
        got = ix.lookup(names)
        assert np.array_equal(got, np.asarray(expect, np.int64))
        assert np.array_equal(again.lookup(names), got)  # two builds of the same input: the same answers
        # m = 0 launches nothing and touches nothing; m = 1; m = 257 (a block and one)
        assert ix.lookup([]).size == 0
        assert ix.lookup(names[:1])[0] == expect[0]
        some = (names * (257 // max(len(names), 1) + 1))[:257]
        assert np.array_equal(ix.lookup(some), np.asarray((expect * (257 // max(len(names), 1) + 1))[:257], np.int64))
    finally:
        ix.close()
        again.close()


def test_names_inside_a_larger_buffer_are_read_from_their_offsets():
    """name_off need not start at 0 (a BAM batch's name blob is searched as it stands): only [name_off[0], name_off[m]) is read."""
    from remora_amd import _lib as L

    rng = np.random.default_rng(3)
    keys = _keys("random", 300, rng)
    ix = _Index(keys, np.arange(300))
    try:
        texts = [_text(k) for k in keys[:50]]
        blob = b"#" * 1000 + b"".join(texts)
        off = 1000 + 36 * np.arange(51, dtype=np.int64)
        out = np.full(50, -99, np.int64)
        L.check(ix.lib.rmr_read_index_lookup(ix.h, blob, off.ctypes.data_as(ctypes.c_void_p), 50, out.ctypes.data_as(ctypes.c_void_p)))
        assert np.array_equal(out, np.arange(50))
        bad = off.copy()
        bad[7] = bad[6] - 1
        assert ix.lib.rmr_read_index_lookup(ix.h, blob, bad.ctypes.data_as(ctypes.c_void_p), 50, out.ctypes.data_as(ctypes.c_void_p)) != 0
        assert b"not ascending" in ix.lib.rmr_last_error()
    finally:
        ix.close()


def test_too_many_reads_are_refused_with_the_bytes_needed():
    from remora_amd import _lib as L
    from remora_amd.engine import get_engine

    lib, eng = L.lib(), get_engine(0)
    h, nd = ctypes.c_void_p(), ctypes.c_int64(0)
    dummy = np.zeros(16, np.uint8)  # refused before a byte of it is read
    n = 1 << 31
    rc = lib.rmr_read_index_create(eng.handle, dummy.ctypes.data_as(ctypes.c_void_p), dummy.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(h),
                                   ctypes.byref(nd))
    assert rc != 0 and not h.value
    msg = lib.rmr_last_error().decode()
    assert str(n) in msg and str(n * 80) in msg and "bytes" in msg
