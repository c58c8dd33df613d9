#!/usr/bin/env python3
"""Reads/s of `infer from_pod5_and_bam`, one process, for a model whose signal-mapping refiner iterates (rough re-scale, then
scale_iters = 2 rounds of banded DP and Theil-Sen re-scale): (b) on the batch ingest, where every round runs on the resident
batch, (p) with RMR_INFER_BATCH_INGEST=0, the per-read path (Python read objects per record, refined on the resident batch as
well), and (h) that path with the refinement it had before the rounds ran on the device - SigMapRefiner.refine_reads on the
read objects, float64 numpy `rescale` per read and round, the batch uploaded afterwards - patched in for the measurement: what
a commit without rescale_device does with such a model (two orders of magnitude slower on these reads: give it one run).  Input and command line of
tests/manual/prof_reverse_signal_infer.py (the 14 test alignments REP times over; the input BAM is written at level 1).  The
cases run in the order given, alternating, so that the spread shows.  The reads of this file have more than 1000 re-scaling
points, so every round draws its Theil-Sen sub-samples from numpy's global generator, which the command does not seed: two
runs differ in the calls of those reads whatever the path (the script says how two runs of one path and of both paths compare;
tests/test_gpu_rescale_device.py holds the two paths to the same bytes under one seed).  With a directory as third
argument the batch case runs once more, alone, under `rocprofv3 --kernel-trace --stats`, and the kernels' shares are
printed.  Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_iterative_refiner.py [REP=2000] [order=b,p,b,p,h] [directory for the kernel trace]"""
import csv
import glob
import gzip
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from oracle import oracle as O  # noqa: E402
from oracle import torch_ref  # noqa: E402
from remora_amd import io as rio  # noqa: E402
from remora_amd.refine_signal_map import SigMapRefiner  # noqa: E402

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
ORDER = (sys.argv[2] if len(sys.argv) > 2 else "b,p,b,p,h").split(",")
TRACE_DIR = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
SCALE_ITERS = 2


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


data = os.path.join(ROOT, "tests", "golden", "data")
pod5, bam = os.path.join(data, "can_reads.pod5"), os.path.join(data, "can_mappings.bam")
tmp = tempfile.mkdtemp()
big = os.path.join(tmp, "big.bam")
recs = [bytes(r.raw) for r in rio.iter_bam_records(bam, want_ref=False)]
blob = b"".join(struct.pack("<i", len(raw)) + raw for raw in recs)
t0 = time.perf_counter()
with rio.BamWriter(big, rio.read_bam_header_bytes(bam), level=1) as w:
    for _ in range(REP):
        w.write(blob)
n = REP * len(recs)
say(f"{n} records, {os.path.getsize(big) / 1e6:.0f} MB BAM written in {time.perf_counter() - t0:.1f} s")
g = np.load(os.path.join(ROOT, "tests", "golden", "real_reads_can.npz"))
net = torch.jit.script(torch_ref.from_state(O.state_from_npz(g)))
meta = json.loads(str(g["meta_txt"]))
# the refiner travels in the metadata as the reference writes it (model_util.add_derived_metadata reads it back)
ref = SigMapRefiner(kmer_model_filename=os.path.join(data, "levels_4mer.txt"), do_rough_rescale=True, scale_iters=SCALE_ITERS, do_fix_guage=True)
meta.update(refine_kmer_levels=np.asarray(ref.levels_array, np.float32).tobytes().decode("cp437"), refine_kmer_center_idx=int(ref.center_idx),
            refine_do_rough_rescale=True, refine_scale_iters=SCALE_ITERS, refine_algo=ref.algo, refine_half_bandwidth=int(ref.half_bandwidth),
            refine_sd_arr=np.asarray(ref.sd_arr, np.float32).tobytes().decode("cp437"))
meta.setdefault("base_start_justify", False)
meta.setdefault("offset", 0)
pt = os.path.join(tmp, "iterative.pt")
torch.jit.save(net, pt, _extra_files={"meta.txt": json.dumps(meta)})
CASES = {"b": ("batch ingest", {}), "p": ("per-read path (RMR_INFER_BATCH_INGEST=0)", {"RMR_INFER_BATCH_INGEST": "0"}),
         "h": ("per-read path, host refinement (refine_reads)", {"RMR_INFER_BATCH_INGEST": "0"})}
# case h: the command with the resident refinement replaced by the host one
HOST_REFINEMENT = """
import sys
from remora_amd.data_chunks import DeviceReads
from remora_amd.refine_signal_map import SigMapRefiner
def refine(self, dr, reads, errors="raise"):
    errs = self.refine_reads(reads)
    dr.__dict__.update(DeviceReads(reads, dr.engine).__dict__)
    for e in errs:
        if e is not None and errors == "raise":
            raise e
    return errs if errors == "collect" else None
SigMapRefiner.rough_rescale_device = lambda self, dr, reads, *a, **k: None  # (refine_reads does it)
SigMapRefiner.refine_device_reads = refine
from remora_amd.__main__ import main
sys.exit(main(sys.argv[1:]))
"""


def command(out, host_refinement=False):
    return [sys.executable] + (["-c", HOST_REFINEMENT] if host_refinement else ["-m", "remora_amd"]) + ["infer", "from_pod5_and_bam", pod5, big, "--model", pt, "--out-bam", out, "--dtype", "fp32",
            "--procs-per-gpu", "1", "--reads-per-batch", "512", "--bam-level", "1"]


rates, outs = {k: [] for k in CASES}, {k: [] for k in CASES}
for i, case in enumerate(ORDER):
    title, env = CASES[case]
    out = os.path.join(tmp, f"out_{case}{i}.bam")
    cmd = command(out, host_refinement=case == "h")
    if i == 0:
        say("python " + " ".join(os.path.basename(c) if os.sep in c else c for c in cmd[1:]))
    t = time.perf_counter()
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=1500, env=dict(os.environ, PYTHONPATH=ROOT, **env))  # (h: 12 ms a read)
    wall = time.perf_counter() - t
    m = re.search(r"= (\d+) reads/s", r.stderr)
    if r.returncode != 0 or not m:
        say(f"({case}) FAILED rc={r.returncode}: {r.stderr[-1500:]}")
        sys.exit(1)
    rates[case].append(int(m.group(1)))
    say(f"({case}) {title}: {m.group(1)} reads/s (models loaded), {n / wall:.0f} incl. start-up ({wall:.1f} s)")
    for ln in r.stderr.splitlines():
        if ln.startswith("["):
            say("      " + ln)
    outs[case].append(out)


def differing_records(a, b):
    """(records that differ, records) of two output BAMs with the same records in the same order."""
    ra, rb = ([bytes(r.raw) for r in rio.iter_bam_records(f, want_ref=False)] for f in (a, b))
    return (sum(x != y for x, y in zip(ra, rb)) + abs(len(ra) - len(rb)), max(len(ra), len(rb)))


for title, pair in (("two runs of (b)", outs["b"][:2]), ("two runs of (p)", outs["p"][:2]), ("(b) and (p)", outs["b"][:1] + outs["p"][:1])):
    if len(pair) == 2:
        if gzip.decompress(open(pair[0], "rb").read()) == gzip.decompress(open(pair[1], "rb").read()):
            say(f"{title}: identical output")
        else:
            say(f"{title}: %d of %d records differ (unseeded sub-samples)" % differing_records(*pair))
shares = {}
if TRACE_DIR:
    os.makedirs(TRACE_DIR, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", TRACE_DIR, "--"] + command(os.path.join(tmp, "out_trace.bam"))
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        say(f"(trace) FAILED rc={r.returncode}: {r.stderr[-1500:]}")
        sys.exit(1)
    rows = []
    for path in glob.glob(os.path.join(TRACE_DIR, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    total = sum(float(row["TotalDurationNs"]) for row in rows) or 1.0
    rows.sort(key=lambda row: -float(row["TotalDurationNs"]))
    say(f"kernel time under the trace: {total / 1e6:.1f} ms in {len(rows)} kernels")
    for k, row in enumerate(rows):
        name = row["Name"]
        share = float(row["TotalDurationNs"]) / total
        new = any(s in name for s in ("rescale_points_kernel", "theil_sen_kernel"))
        if k < 10 or new:
            say(f"   {100 * share:5.1f} %  {float(row['TotalDurationNs']) / 1e6:9.2f} ms  {int(float(row['Calls'])):7d} calls  {name[:110]}")
        if new:
            shares["rescale_points" if "rescale_points" in name else "theil_sen_fit"] = round(share, 4)
say("RESULT " + json.dumps({"records": n, "scale_iters": SCALE_ITERS, "reads_per_s": rates, "kernel_share": shares}))
