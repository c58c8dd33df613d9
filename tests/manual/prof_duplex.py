#!/usr/bin/env python3
"""Alignments/s and DP cell updates/s of the simplex-to-duplex aligner (rmr_duplex_align, csrc/k_duplex.hip) for PAIRS duplex pairs
(two alignments each) of LEN bases, simplex reads = mutated copies of the duplex sequence at the reference fuzz's rates (5 %
substitutions, 10 % indels); the split of the wall time between the DP kernel, the traceback kernel and the rest of the call
from the engine's event timing (Engine.profile) - for rocprofv3's view run the script alone under
`rocprofv3 --kernel-trace --stats -- python tests/manual/prof_duplex.py ...` -; and, for orientation, the single-thread rate of the
C++ restatement (tests/c/duplex_restate.cpp) on SAMPLE of the same alignments on the same box.  Test infrastructure; run by hand.

    python tests/manual/prof_duplex.py [PAIRS=512] [LEN=5000] [SAMPLE=2] [BUDGET_GIB=16]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import duplex_restate as R  # noqa: E402

from remora_amd import duplex_utils as DU  # noqa: E402
from remora_amd.engine import get_engine  # noqa: E402
from remora_amd.io import revcomp  # noqa: E402

PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 512
LEN = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
SAMPLE = int(sys.argv[3]) if len(sys.argv) > 3 else 2
BUDGET = int(float(sys.argv[4]) * (1 << 30)) if len(sys.argv) > 4 else None

rng = np.random.default_rng(42)
NUCS = np.array(list("ACGT"))


def mutate(seq, p_err=0.05, p_indel=0.1):
    seq = np.array(list(seq))
    sub = rng.uniform(size=seq.size) <= p_err
    seq[sub] = rng.choice(NUCS, int(sub.sum()))
    indel = rng.uniform(size=seq.size) <= p_indel
    ins = indel & (rng.uniform(size=seq.size) > 0.5)
    out = []
    for b, i, k in zip(seq.tolist(), indel.tolist(), ins.tolist()):
        if not i:
            out.append(b)
        elif k:
            out += [b, str(rng.choice(NUCS))]
    return "".join(out)


aligns = []
for _ in range(PAIRS):
    duplex = "".join(rng.choice(NUCS, LEN))
    aligns += [(mutate(duplex), duplex), (mutate(revcomp(duplex)), revcomp(duplex))]
cells = float(sum(len(s) * len(d) for s, d in aligns))
eng = get_engine(0)
DU.align_batch(aligns[:2], eng)  # warm-up: library load, arenas
eng.profile_enable(True)
eng.profile_reset()
t0 = time.perf_counter()
res = DU.align_batch(aligns, eng, BUDGET)
dt = time.perf_counter() - t0
prof = eng.profile()
eng.profile_enable(False)
assert not res.status.any()
out = dict(pairs=PAIRS, length=LEN, alignments=len(aligns), groups=res.n_groups, wall_s=round(dt, 4), alignments_per_s=round(len(aligns) / dt, 1),
           cell_updates_per_s=float(f"{cells / dt:.4g}"), dp_ms=round(prof.get("duplex_dp", (0, 0))[0], 2),
           traceback_ms=round(prof.get("duplex_traceback", (0, 0))[0], 2))
out["rest_ms"] = round(dt * 1e3 - out["dp_ms"] - out["traceback_ms"], 2)  # copies, allocation of the trace, host sorting
out["dp_cell_updates_per_s"] = float(f"{cells / max(out['dp_ms'], 1e-9) * 1e3:.4g}")
if SAMPLE > 0:
    rate = []
    want = R.align_cpp(aligns[:SAMPLE], R.build_cpp(tempfile.mkdtemp()), rate)
    for a, w in enumerate(want):
        assert (int(res.score[a]), int(res.end_row[a])) == (w["score"], w["end_row"])
    out["cpp_restatement_cell_updates_per_s_one_thread"] = rate[0]
print(json.dumps(out), flush=True)
