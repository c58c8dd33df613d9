#!/usr/bin/env python3
"""Alignments/s and DP cell updates/s of the simplex-to-duplex aligner in its two memory forms (rmr_duplex_align_mode,
csrc/k_duplex.hip): "full" (the 4-bit trace of every cell stored) and "checkpoint" (one DP line per strip kept, the trace
recomputed strip by strip while walking back), at SHAPES = N x LEN: N alignments (N / 2 duplex sequences of LEN random bases, per
sequence two simplex reads = mutated copies of it and of its reverse complement at the reference fuzz's rates, as
tests/manual/prof_duplex.py makes them).  Per shape: one warm-up call per mode at the shape itself, then REPEATS timed calls per
mode, the modes alternating; wall time around duplex_utils.align_batch (which ends in a device synchronise), the kernel times
from the engine's events; median, lowest and highest of the repeats.  The two forms must return the same bytes: asserted on the
first repeat of every shape.  Test infrastructure; run by hand.

    python tests/manual/prof_duplex_modes.py [SHAPES=1024x5000,64x25000,1024x25000] [REPEATS=5] [BUDGET_GIB=16] [MODES=full,checkpoint]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NUCS = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[NUCS] = NUCS[::-1]


def mutate(rng, seq, p_err=0.05, p_indel=0.1):
    """tests/manual/prof_duplex.py's mutation on a uint8 array: 5 % substitutions; 10 % indels, half of them a random base
    inserted behind the base, half the base deleted."""
    seq = seq.copy()
    sub = rng.uniform(size=seq.size) <= p_err
    seq[sub] = rng.choice(NUCS, int(sub.sum()))
    indel = rng.uniform(size=seq.size) <= p_indel
    ins = indel & (rng.uniform(size=seq.size) > 0.5)
    copies = np.where(indel, np.where(ins, 2, 0), 1)
    out = np.repeat(seq, copies)
    out[np.cumsum(copies)[ins] - 1] = rng.choice(NUCS, int(ins.sum()))
    return out


def make_alignments(n, length, seed=42):
    """[(simplex, duplex)] * n as str."""
    rng = np.random.default_rng(seed)
    aligns = []
    for _ in range((n + 1) // 2):
        duplex = rng.choice(NUCS, length)
        rc = COMP[duplex[::-1]]
        for d in (duplex, rc):
            aligns.append((mutate(rng, d).tobytes().decode(), d.tobytes().decode()))
    return aligns[:n]


def _spread(values):
    v = sorted(values)
    return dict(median=float(f"{v[len(v) // 2]:.4g}"), low=float(f"{v[0]:.4g}"), high=float(f"{v[-1]:.4g}"))


def measure(aligns, eng, modes, repeats, budget):
    """{mode: dict} for one shape."""
    from remora_amd import duplex_utils as DU

    cells = float(sum(len(s) * len(d) for s, d in aligns))
    first = {}
    for mode in modes:  # warm-up at the shape itself: code objects, the staging arena, the allocator
        first[mode] = DU.align_batch(aligns, eng, budget, mode)
        assert not first[mode].status.any(), (mode, np.unique(first[mode].status))
    for mode in modes[1:]:
        a, b = first[modes[0]], first[mode]
        assert all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("score", "end_row", "query_start", "ref_start", "ref_end", "n_runs"))
        assert all(a.words[a.run_off[k]:a.run_off[k] + a.n_runs[k]].tobytes() == b.words[b.run_off[k]:b.run_off[k] + b.n_runs[k]].tobytes()
                   for k in range(len(aligns)))
    walls = {m: [] for m in modes}
    kernels = {m: [] for m in modes}
    eng.profile_enable(True)
    for _ in range(repeats):
        for mode in modes:
            eng.profile_reset()
            t0 = time.perf_counter()
            DU.align_batch(aligns, eng, budget, mode)
            walls[mode].append(time.perf_counter() - t0)
            prof = eng.profile()
            kernels[mode].append({k: prof[k][0] for k in ("duplex_dp", "duplex_traceback", "duplex_lines", "duplex_backtrack") if k in prof})
    eng.profile_enable(False)
    out = {}
    for mode in modes:
        res = first[mode]
        out[mode] = dict(groups=res.n_groups, checkpointed=res.n_checkpointed, wall_s=_spread(walls[mode]),
                         alignments_per_s=_spread([len(aligns) / w for w in walls[mode]]),
                         cell_updates_per_s=_spread([cells / w for w in walls[mode]]),
                         kernel_ms={k: _spread([r[k] for r in kernels[mode]])["median"] for k in kernels[mode][0]})
    return out


def main(argv):
    sys.path.insert(0, ROOT)
    from remora_amd.engine import get_engine

    shapes = [tuple(int(x) for x in s.split("x")) for s in (argv[1] if len(argv) > 1 else "1024x5000,64x25000,1024x25000").split(",")]
    repeats = int(argv[2]) if len(argv) > 2 else 5
    budget = int(float(argv[3]) * (1 << 30)) if len(argv) > 3 else None
    modes = (argv[4] if len(argv) > 4 else "full,checkpoint").split(",")
    eng = get_engine(0)
    for n, length in shapes:
        aligns = make_alignments(n, length)
        res = measure(aligns, eng, modes, repeats, budget)
        for mode in modes:
            print(json.dumps(dict(alignments=n, length=length, cells=float(sum(len(s) * len(d) for s, d in aligns)), mode=mode,
                                  repeats=repeats, **res[mode])), flush=True)


if __name__ == "__main__":
    main(sys.argv)
