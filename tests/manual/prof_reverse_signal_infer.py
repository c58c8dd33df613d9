#!/usr/bin/env python3
"""Reads/s of `infer from_pod5_and_bam`, one process, for a reverse-signal model against the forward-signal model on the same
file: (b) this tree with the model's metadata saying reverse_signal, (c) this tree with the forward model, and - when a
checkout of another commit with its library built is given - (a) that tree with the reverse-signal model.  Input and command
line of tests/manual/prof_infer_cli.py (the 14 test alignments REP times over; the input BAM is written at level 1).  The
cases run in the order given, alternating, so that the spread shows.  Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_reverse_signal_infer.py [REP=24000] [order=c,b,c,b,c,b] [other tree for case a]"""
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

REP = int(sys.argv[1]) if len(sys.argv) > 1 else 24000
ORDER = (sys.argv[2] if len(sys.argv) > 2 else "c,b,c,b,c,b").split(",")
PARENT = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else None
if "a" in ORDER and PARENT is None:
    sys.exit("case a needs the other tree")


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
pts = {}
for name, rev in (("fwd", False), ("rev", True)):
    meta["reverse_signal"] = rev
    pts[name] = os.path.join(tmp, f"{name}.pt")
    torch.jit.save(net, pts[name], _extra_files={"meta.txt": json.dumps(meta)})
CASES = {"a": ("other tree, reverse-signal model", PARENT, "rev"),
         "b": ("this tree, reverse-signal model (batch ingest)", ROOT, "rev"),
         "c": ("this tree, forward-signal model (batch ingest)", ROOT, "fwd")}
rates, outs = {k: [] for k in CASES}, {}
for i, case in enumerate(ORDER):
    title, cwd, which = CASES[case]
    out = os.path.join(tmp, f"out_{case}.bam")
    cmd = [sys.executable, "-m", "remora_amd", "infer", "from_pod5_and_bam", pod5, big, "--model", pts[which], "--out-bam", out, "--dtype", "fp32",
           "--procs-per-gpu", "1", "--reads-per-batch", "512", "--bam-level", "1"]
    if i < 3:
        say(f"({case}) cwd={'<other tree>' if cwd == PARENT else '<this tree>'}: " + " ".join(["python"] + [os.path.basename(c) if os.sep in c else c for c in cmd[1:]]))
    t = time.perf_counter()
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=400)
    wall = time.perf_counter() - t
    m = re.search(r"= (\d+) reads/s", r.stderr)
    if r.returncode != 0 or not m:
        say(f"({case}) FAILED rc={r.returncode}: {r.stderr[-1500:]}")
        sys.exit(1)
    timing = [ln for ln in r.stderr.splitlines() if ln.startswith("[")]
    rates[case].append(int(m.group(1)))
    say(f"({case}) {title}: {m.group(1)} reads/s (models loaded), {n / wall:.0f} incl. start-up ({wall:.1f} s)")
    for ln in timing:
        say("      " + ln)
    outs[case] = out
if "a" in outs and "b" in outs:
    same = gzip.decompress(open(outs["a"], "rb").read()) == gzip.decompress(open(outs["b"], "rb").read())
    say(f"output of (b) identical to (a) after decompression: {same}")
say("RESULT " + json.dumps({"records": n, "reads_per_s": rates}))
