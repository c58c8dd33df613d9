"""The read-id index of a POD5 dataset (rmr_read_index_create / _lookup, csrc/k_read_index.hip) beside the single-file reader's
way of indexing the same ids ({str(uuid.UUID(bytes=b)): row}, io.Pod5File) and of resolving a BAM batch's names (the `ids`
section of io._ingest_batch: a Python loop over the records), on synthetic random ids.

    python tools/prof_read_index.py [N ...] [--repeats 5] [--batch 512]        (default N: 1000000 10000000)

One JSON line per N: medians of `repeats` builds (wall seconds around the call, which ends in a stream synchronise), the bytes
the table keeps on the device, the resident-set growth of the Python dict, and microseconds per batch of `batch` names for the
lookup kernel (upload, launch, copy back) and for the dict loop."""
import argparse
import ctypes
import gc
import json
import os
import statistics
import sys
import time
import uuid

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from remora_amd import _lib as L  # noqa: E402
from remora_amd.engine import get_engine  # noqa: E402


def rss_bytes():
    with open("/proc/self/statm") as fh:
        return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="*", type=int, default=[1_000_000, 10_000_000])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lib, eng = L.lib(), get_engine(0)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for n in args.n:
        rng = np.random.default_rng(n)
        keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        values = np.arange(n, dtype=np.int64)

        def build():
            h, nd = ctypes.c_void_p(), ctypes.c_int64(0)
            L.check(lib.rmr_read_index_create(eng.handle, p(keys), p(values), n, ctypes.byref(h), ctypes.byref(nd)))
            return h, nd.value

        h, nd = build()  # warm-up: code objects, rocPRIM's first launches
        lib.rmr_read_index_destroy(h)
        t_dev = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info(0)[0]
            t0 = time.perf_counter()
            h, nd = build()
            t_dev.append(time.perf_counter() - t0)
            resident = free0 - torch.cuda.mem_get_info(0)[0]
            lib.rmr_read_index_destroy(h)
            print(f"# n={n} device build {t_dev[-1]:.4f} s", flush=True)
        # the single-file reader's index of the same ids (io.Pod5File.__init__): the column as a list of bytes, then the two comprehensions
        as_bytes = [row.tobytes() for row in keys]
        t_dict, grow = [], []
        for _ in range(args.repeats):
            gc.collect()
            r0 = rss_bytes()
            t0 = time.perf_counter()
            read_ids = [str(uuid.UUID(bytes=b)) for b in as_bytes]
            row_of = {rid: r for r, rid in enumerate(read_ids)}
            t_dict.append(time.perf_counter() - t0)
            grow.append(rss_bytes() - r0)
            print(f"# n={n} dict build {t_dict[-1]:.3f} s", flush=True)
            if _ + 1 < args.repeats:
                del read_ids, row_of
        # one batch of names: present ids, as a BAM batch holds them (a blob and offsets)
        h, nd = build()
        m = args.batch
        pick = rng.integers(0, n, m)
        texts = [read_ids[i].encode() for i in pick.tolist()]
        blob, off = b"".join(texts), 36 * np.arange(m + 1, dtype=np.int64)
        out = np.empty(m, np.int64)
        t_look, t_loop = [], []
        for k in range(220):
            t0 = time.perf_counter()
            L.check(lib.rmr_read_index_lookup(h, blob, p(off), m, p(out)))
            t_look.append(time.perf_counter() - t0)
        assert np.array_equal(out, pick)
        offs = off.tolist()
        for k in range(220):
            t0 = time.perf_counter()
            kept, rows = [], []
            for i in range(m):  # the `ids` section of io._ingest_batch
                rid = blob[offs[i] : offs[i + 1]].decode("latin-1")
                r = row_of.get(rid)
                if r is not None:
                    kept.append(i)
                    rows.append(r)
            t_loop.append(time.perf_counter() - t0)
        assert rows == pick.tolist()
        lib.rmr_read_index_destroy(h)
        del read_ids, row_of, as_bytes
        print(json.dumps({
            "n": n, "n_distinct": nd, "repeats": args.repeats,
            "device_build_s_median": statistics.median(t_dev), "device_build_s_all": [round(t, 4) for t in t_dev],
            "device_table_bytes": 24 * nd, "device_bytes_held_after_build": int(resident),
            "dict_build_s_median": statistics.median(t_dict), "dict_build_s_all": [round(t, 3) for t in t_dict],
            "dict_rss_growth_bytes_median": int(statistics.median(grow)),
            "batch": m, "lookup_us_per_batch_median": 1e6 * statistics.median(t_look[20:]),
            "dict_loop_us_per_batch_median": 1e6 * statistics.median(t_loop[20:])}), flush=True)


if __name__ == "__main__":
    main()
