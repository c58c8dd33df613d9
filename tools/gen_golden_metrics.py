"""Writes tests/golden/base_metrics.npz: synthetic reads and what the reference's five per-base metric functions
(remora.metrics.METRIC_FUNCS) return for them - data only.

    python tools/gen_golden_metrics.py --reference-src <checkout of nanoporetech/remora>/src

The reads sit where a segmented reduction can go wrong: 1, 63, 64, 65 and 4097 bases (one group of 64, its edges, many
groups), a read whose whole signal is one sample, dwells of 0, 1, 2, 3 and 5000 inside one read, and a mapping that neither
starts at sample 0 nor ends at the last one (clip_sig).  Every read is evaluated at the trims (1, 1), (2, 2), (0, 0) and
(6000, 6000) - larger than every dwell: all-NaN trimmed metrics.  The signal handed to the reference is (dacs - shift) / scale
in float64, as io.Read.norm_signal computes it."""
import argparse
import importlib.util
import json
import os

import numpy as np

TRIMS = ((1, 1), (2, 2), (0, 0), (6000, 6000))


def _reads(rng):
    reads = []

    def add(dwells, lead=0, tail=0):
        dwells = np.asarray(dwells, np.int64)
        seq_to_sig = lead + np.concatenate([[0], np.cumsum(dwells)])
        n = int(seq_to_sig[-1]) + tail
        dacs = rng.integers(-600, 1400, size=n).astype(np.int16)
        reads.append((dacs, seq_to_sig.astype(np.int64), float(rng.uniform(350, 450)), float(rng.uniform(60, 140))))

    for nb in (1, 63, 64, 65):
        add(rng.integers(1, 16, size=nb))
    add(rng.integers(1, 7, size=4097))
    add([1])                                                        # the whole signal is one sample
    add([5, 0, 1, 2, 3, 5000, 0, 0, 7, 3, 1, 0, 4, 9, 2, 2, 0, 11])  # 3 = start + end trim + 1 at trims (1, 1)
    add(rng.integers(0, 12, size=130), lead=17, tail=23)            # clipped at both ends, zero dwells at group edges
    return reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference-src", required=True, help="src/ of the reference checkout (remora/metrics.py needs numpy only)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "base_metrics.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_metrics", os.path.join(args.reference_src, "remora", "metrics.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(20)
    out = {"trims": np.asarray(TRIMS, np.int64)}
    reads = _reads(rng)
    out["shift"] = np.asarray([r[2] for r in reads])
    out["scale"] = np.asarray([r[3] for r in reads])
    keys = {}
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)  # noqa: E731
    for i, (dacs, seq_to_sig, shift, scale) in enumerate(reads):
        sig = (dacs - shift) / scale
        assert sig.dtype == np.float64
        out[f"r{i}_dacs"], out[f"r{i}_map"] = dacs, seq_to_sig
        with np.errstate(all="ignore"):
            res = {name: func(sig, seq_to_sig) for name, func in ref.METRIC_FUNCS.items() if "trim" not in name}
            out[f"r{i}_dwell"], out[f"r{i}_mean"], out[f"r{i}_sd"] = res["dwell"]["dwell"], res["dwell_mean_sd"]["mean"], res["dwell_mean_sd"]["sd"]
            assert same(res["dwell_mean"]["mean"], out[f"r{i}_mean"]) and same(res["dwell_mean"]["dwell"], out[f"r{i}_dwell"])
            for t, (st, en) in enumerate(TRIMS):
                a = ref.METRIC_FUNCS["dwell_trimmean"](sig, seq_to_sig, start_trim=st, end_trim=en)
                b = ref.METRIC_FUNCS["dwell_trimmean_trimsd"](sig, seq_to_sig, start_trim=st, end_trim=en)
                assert same(a["trimmean"], b["trimmean"]) and same(a["dwells"], out[f"r{i}_dwell"]) and same(b["dwell"], out[f"r{i}_dwell"])
                out[f"r{i}_t{t}_trimmean"], out[f"r{i}_t{t}_trimsd"] = b["trimmean"], b["trimsd"]
                res["dwell_trimmean"], res["dwell_trimmean_trimsd"] = a, b
        keys = {name: list(v) for name, v in res.items()}
    out["returned_keys"] = np.frombuffer(json.dumps(keys, sort_keys=True).encode(), np.uint8)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {len(reads)} reads, {os.path.getsize(args.out):,} bytes")


if __name__ == "__main__":
    main()
