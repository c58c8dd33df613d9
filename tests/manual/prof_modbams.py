#!/usr/bin/env python3
"""Records/s of validate.parse_mod_bam on a synthesised BAM of tagged records, its stages timed apart (BAM reader alone,
reader + tokeniser, everything), and records/s of the plain-Python restatement of the reference's per-read loop
(tests/modbam_restate.py: modified_bases, get_aligned_pairs and the dictionary lookups per aligned pair) on a sample of the same
records on the same box - the parent commit has no path of its own to compare with.  512 distinct records of LEN bases with
a C+hm? entry on every third C, a tenth of them reverse, CIGARs with I / D / S; repeated to RECORDS.  The
kernels' share of the wall time is printed from the engine's event timing (Engine.profile); for rocprofv3's view run the script under
`rocprofv3 --kernel-trace --stats -- python tests/manual/prof_modbams.py ...`.  Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_modbams.py [RECORDS=200000] [LEN=2000] [SAMPLE=400]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import modbam_restate as mr  # noqa: E402

from remora_amd import io as rio  # noqa: E402
from remora_amd import validate as rv  # noqa: E402
from remora_amd.engine import get_engine  # noqa: E402

RECORDS = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
LEN = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
SAMPLE = int(sys.argv[3]) if len(sys.argv) > 3 else 400
REFS = [("chr1", 10_000_000)]
ALPHABET = ["C", "h", "m"]


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


rng = np.random.default_rng(1)
distinct = []
for i in range(512):
    seq = "".join(rng.choice(list("ACGT"), LEN))
    rev = i % 10 == 0
    n_c = (mr.original_sequence(seq, rev)).count("C")
    ords = list(range(0, n_c, 3))
    mm = "C+hm?" + "".join(f",{d}" for d in [0] + [2] * (len(ords) - 1)) + ";"
    cigar = [("S", 20), ("M", LEN // 2 - 30), ("I", 3), ("M", 200), ("D", 5), ("M", LEN - LEN // 2 - 193 - 10), ("S", 10)]
    distinct.append(dict(name=f"r{i}", seq=seq, flag=16 if rev else 0, ref_id=0, ref_name="chr1", pos=int(rng.integers(1000, 9_000_000)),
                         cigar=cigar, mm=mm, ml=rng.integers(0, 256, 2 * len(ords)).tolist(), has_md=True))
gt_sites = {("chr1", s): {} for s in "+-"}
for rec in distinct:  # truth: every fourth reference position of every alignment
    sites = gt_sites[("chr1", "-" if rec["flag"] & 16 else "+")]
    for p in range(rec["pos"], rec["pos"] + LEN, 4):
        sites[p] = "Chm"[p % 3]
tmp = tempfile.mkdtemp()
bam = os.path.join(tmp, "tagged.bam")
blob = b"".join(mr.bam_record(r["name"], r["flag"], 0, r["pos"], r["cigar"], r["seq"], mr.mod_tags(r["mm"], r["ml"])) for r in distinct)
t0 = time.perf_counter()
with rio.BamWriter(bam, mr.bam_header(REFS), level=1) as w:
    for _ in range(max(RECORDS // 512, 1)):
        w.write(blob)
n = max(RECORDS // 512, 1) * 512
say(f"{n} records of {LEN} bases, {os.path.getsize(bam) / 1e6:.0f} MB BAM written in {time.perf_counter() - t0:.1f} s")

eng = get_engine(None)
rv.parse_mod_bam(bam, gt_sites, None, ALPHABET, None, batch=512) if n <= 4096 else None  # (small inputs: warm everything once)
t0 = time.perf_counter()
for rb, _ in rio.iter_bam_raw_batches(bam, batch=512):
    pass
t_read = time.perf_counter() - t0
t0 = time.perf_counter()
for rb, _ in rio.iter_bam_raw_batches(bam, batch=512):
    rv.tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off)
t_tok = time.perf_counter() - t0
eng.profile_enable(True)
eng.profile_reset()
t0 = time.perf_counter()
probs, labels = rv.parse_mod_bam(bam, gt_sites, None, ALPHABET, None, batch=512)
t_all = time.perf_counter() - t0
kern_ms = eng.profile().get("modbam_sites", (None, None))[0]
eng.profile_enable(False)
say(f"BAM reader alone      : {t_read:7.2f} s  {n / t_read:9.0f} records/s")
say(f"reader + tokeniser    : {t_tok:7.2f} s  {n / t_tok:9.0f} records/s")
say(f"parse_mod_bam         : {t_all:7.2f} s  {n / t_all:9.0f} records/s, {labels.size} calls on truth sites")
if kern_ms is not None:
    say(f"site kernels (events) : {kern_ms / 1e3:7.2f} s  {100 * kern_ms / 1e3 / t_all:5.1f} % of parse_mod_bam")

sample = [distinct[i % 512] for i in range(SAMPLE)]
t0 = time.perf_counter()
got = 0
for rec in sample:  # the reference's loop, restated: modified_bases, aligned pairs, a dictionary lookup per pair
    rev = bool(rec["flag"] & 16)
    mods = mr.modified_bases(rec["seq"], rev, rec["mm"], rec["ml"])
    pairs = mr.aligned_pairs(rec["cigar"], rec["pos"])
    q_mod = {}
    for (_, strand, name), vals in mods.items():
        if strand != int(rev) or str(name) not in ALPHABET:
            continue
        for pos, q in vals:
            q_mod.setdefault(pos, {})[name] = (q + 0.5) / 256
    full = {q: np.array([1 - sum(v.values())] + [v.get(m, 0) for m in ALPHABET[1:]]) for q, v in q_mod.items()}
    truth = gt_sites.get(("chr1", "-" if rev else "+"))
    for q_pos, r_pos, _ in pairs:
        lab, pr = truth.get(r_pos), full.get(q_pos)
        if lab is not None and pr is not None:
            got += 1
t_py = time.perf_counter() - t0
say(f"python restatement    : {t_py:7.2f} s  {SAMPLE / t_py:9.0f} records/s over {SAMPLE} records ({got} calls)")
say("RESULT " + json.dumps({"records": n, "bases": LEN, "reader_rps": round(n / t_read), "reader_tokeniser_rps": round(n / t_tok),
                            "parse_mod_bam_rps": round(n / t_all), "python_restatement_rps": round(SAMPLE / t_py),
                            "kernel_share": None if kern_ms is None else round(kern_ms / 1e3 / t_all, 4)}))
