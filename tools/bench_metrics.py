"""One measurement of the per-base metrics kernel (rmr_base_metrics, csrc/k_metrics.hip): 2048 synthetic reads of 5 kb,
all five outputs, HIP events around the launch (the library's per-kernel profiler), median of nine runs after three warm-up
runs.  Prints one JSON line: time, bases/s, the bytes the algorithm has to move (2 B per sample and 8 B per mapping entry in,
36 B per base out) over that time, and its share of the HBM peak (8.0 TB/s specified for the MI355X).

    python tools/bench_metrics.py [--reads 2048] [--bases 5000] [--out profiles/<name>.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--bases", type=int, default=5000)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch

    from remora_amd import _lib as L
    from remora_amd import synth
    from remora_amd.data_chunks import DeviceReads, RemoraRead
    from remora_amd.engine import get_engine

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    distinct = [synth.synth_read(args.bases, seed=s) for s in range(64)]
    reads = [RemoraRead(dacs=r["dacs"], shift=r["shift"], scale=r["scale"], seq_to_sig_map=r["seq_to_sig_map"], int_seq=r["int_seq"],
                        read_id=str(i)) for i, r in ((i, distinct[i % 64]) for i in range(args.reads))]
    eng = get_engine(0)
    dr = DeviceReads(reads, eng)
    n_bases, n_samples = int(dr.seq_off[-1]), int(dr.sig_off[-1])
    dev = eng.torch_device
    dwell = torch.empty(n_bases, dtype=torch.float32, device=dev)
    outs = [torch.empty(n_bases, dtype=torch.float64, device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    eng.profile_enable(True)
    times = []
    for run in range(args.warmup + args.runs):
        eng.profile_reset()
        L.check(L.lib().rmr_base_metrics(eng.handle, dr.n_reads, dr.dacs.data_ptr(), dr.d_sig_off.data_ptr(), dr.s2s.data_ptr(),
                                         dr.d_seq_off.data_ptr(), dr.shift.data_ptr(), dr.scale.data_ptr(), int(np.diff(dr.seq_off).max()),
                                         1, 1, dwell.data_ptr(), *(ctypes.c_void_p(o.data_ptr()) for o in outs)))
        ms, n = eng.profile()["base_metrics"]
        assert n == 1
        if run >= args.warmup:
            times.append(ms)
    eng.profile_enable(False)
    assert torch.isfinite(outs[2]).float().mean().item() > 0.5  # the trimmed means were computed
    med = float(np.median(times))
    nbytes = 2 * n_samples + 8 * (n_bases + dr.n_reads) + 36 * n_bases
    res = {"kernel": "base_metrics", "reads": dr.n_reads, "bases": n_bases, "samples": n_samples, "runs_ms": [round(t, 4) for t in times],
           "median_ms": round(med, 4), "bases_per_s": round(n_bases / (med * 1e-3)), "samples_per_s": round(n_samples / (med * 1e-3)),
           "algorithmic_bytes": nbytes, "bytes_per_s": round(nbytes / (med * 1e-3)), "hbm_peak_bytes_per_s": HBM_PEAK,
           "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 4),
           "roofline_ms": round(nbytes / HBM_PEAK * 1e3, 4)}  # the least time that traffic allows; what limits the kernel is another matter
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
