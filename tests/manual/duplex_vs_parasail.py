#!/usr/bin/env python3
"""Where parasail is installed: the GPU aligner (duplex_utils.map_simplex_to_duplex) against the reference's
parasail.sg_qx_trace_scan_32(simplex, duplex, 10, 2, dnafull) + trim_parasail_alignment on the reference's fuzz inputs
(tests/test_duplex.py:14-54: 75 duplex sequences of 5 kb, a mutated simplex copy, T-overhangs on either side).  The optimal
score must be equal on every input; the mapping is guaranteed equal only where the optimum is unique (README.md, "Duplex"), so
the script REPORTS the share of identical mappings and the largest coordinate difference.  Never run by the suite.

    python tests/manual/duplex_vs_parasail.py [CASES=75]"""
import os
import sys
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

try:
    import parasail
except ImportError:
    sys.exit("parasail is not installed: nothing to compare with")

from remora_amd import data_chunks as DC  # noqa: E402
from remora_amd import duplex_utils as DU  # noqa: E402

CASES = int(sys.argv[1]) if len(sys.argv) > 1 else 75
OPS = {"=": 0, "X": 0, "M": 0, "I": 1, "D": 2}


def parasail_mapping(simplex, duplex):
    res = parasail.sg_qx_trace_scan_32(simplex, duplex, DU.GAP_OPEN, DU.GAP_EXTEND, parasail.dnafull)
    cig, num = deque(), ""
    for ch in res.cigar.decode.decode():
        if ch.isdigit():
            num += ch
        else:
            cig.append((OPS[ch], int(num)))
            num = ""
    query_start = ref_start = 0
    while cig and cig[0][0] != 0:
        op, ln = cig.popleft()
        query_start, ref_start = query_start + (ln if op == 1 else 0), ref_start + (ln if op == 2 else 0)
    while cig and cig[-1][0] != 0:
        cig.pop()
    merged = []
    for op, ln in cig:  # = and X folded into M
        if merged and merged[-1][0] == op:
            merged[-1] = (op, merged[-1][1] + ln)
        else:
            merged.append((op, ln))
    return res.score, ref_start, DC.make_sequence_coordinate_mapping(merged).astype(int) + query_start


rng = np.random.RandomState(42)
nucs = ["A", "C", "G", "T"]


def mutate(seq, p_err=0.05, p_indel=0.1):
    out = []
    for base in seq:
        if rng.uniform() <= p_err:
            base = rng.choice(nucs)
        if rng.uniform() <= p_indel:
            if np.random.uniform() > 0.5:
                out += [base, rng.choice(nucs)]
            continue
        out.append(base)
    return "".join(out)


inputs = []
for _ in range(CASES):
    duplex = "".join(np.random.choice(nucs, size=5000))
    simplex = mutate(duplex)
    overhang = "T" * int(np.floor(rng.uniform(low=5, high=100)))
    inputs += [(simplex, duplex), (simplex, overhang + duplex + overhang), (overhang + simplex + overhang, duplex)]
res = DU.align_batch(inputs)
same = worst = 0
for a, (simplex, duplex) in enumerate(inputs):
    score, ref_start, mapping = parasail_mapping(simplex, duplex)
    assert int(res.status[a]) == 0 and int(res.score[a]) == score, (a, int(res.score[a]), score)
    got = DU.mapping_from_alignment(res.pairwise_alignment(a), duplex)
    if got.duplex_offset == ref_start and got.duplex_to_simplex_mapping.size == mapping.size:
        diff = int(np.abs(got.duplex_to_simplex_mapping - mapping).max())
        same += diff == 0
        worst = max(worst, diff)
    else:
        worst = max(worst, abs(got.duplex_offset - ref_start))
        print(f"input {a}: the trimmed duplex range differs (offset {got.duplex_offset} vs {ref_start})")
print(f"{len(inputs)} inputs, equal scores on all; identical mappings on {same} ({100.0 * same / len(inputs):.1f} %); "
      f"largest coordinate difference {worst}")
