#!/usr/bin/env python3
"""Records/s of pileup.pileup_modbams on a synthesised BAM of tagged records - with a fixed threshold (one pass) and with the
percentile threshold (the histogram pass in front) - beside its yardstick, validate.parse_mod_bam on the same file in the same
process, the reader + tokeniser alone, the peak device memory at two budgets, and the plain-Python restatement of the pileup
(tests/modbam_restate.py: modified_bases, aligned pairs, a dictionary of counts) on a sample of the same records.  The input is
tests/manual/prof_modbams.py's: 512 distinct records of LEN bases with a C+hm? entry on every third C (about 170 calls at 2 kb),
a tenth of them reverse, CIGARs with I / D / S; repeated to RECORDS.  The kernels' share of the wall time is printed from the
engine's event timing; for rocprofv3's view run the script, in a run of its own, under
`rocprofv3 --kernel-trace --stats -- python tests/manual/prof_pileup.py ...`.  Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_pileup.py [RECORDS=200000] [LEN=2000] [SAMPLE=400]"""
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
from remora_amd import pileup as rp  # noqa: E402
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
for rec in distinct:  # the yardstick's truth: every fourth reference position of every alignment
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
small = os.path.join(tmp, "warm.bam")
with rio.BamWriter(small, mr.bam_header(REFS), level=1) as w:
    w.write(blob)
rp.pileup_modbams(small, ALPHABET, pct_filt=10)  # warm everything once
rv.parse_mod_bam(small, gt_sites, None, ALPHABET, None, batch=512)

t0 = time.perf_counter()
for rb, _ in rio.iter_bam_raw_batches(bam, batch=512):
    rv.tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off)
t_tok = time.perf_counter() - t0
t0 = time.perf_counter()
probs, labels = rv.parse_mod_bam(bam, gt_sites, None, ALPHABET, None, batch=512)
t_val = time.perf_counter() - t0
del probs
eng.profile_enable(True)
eng.profile_reset()
t0 = time.perf_counter()
one = rp.pileup_modbams(bam, ALPHABET, filter_threshold=0.6, pct_filt=None)
t_one = time.perf_counter() - t0
prof_one = eng.profile()
eng.profile_reset()
t0 = time.perf_counter()
two = rp.pileup_modbams(bam, ALPHABET, pct_filt=10)
t_two = time.perf_counter() - t0
prof_two = eng.profile()
eng.profile_enable(False)
t0 = time.perf_counter()
tight = rp.pileup_modbams(bam, ALPHABET, filter_threshold=0.6, pct_filt=None, device_gib=0.25)
t_tight = time.perf_counter() - t0
assert np.array_equal(tight.counts, one.counts) and np.array_equal(tight.pos, one.pos)
ms = lambda prof, k: prof.get(k, (0.0, 0))[0]  # noqa: E731
say(f"reader + tokeniser         : {t_tok:7.2f} s  {n / t_tok:9.0f} records/s")
say(f"validate parse_mod_bam     : {t_val:7.2f} s  {n / t_val:9.0f} records/s, {labels.size} calls on truth sites (the yardstick)")
say(f"pileup, fixed threshold    : {t_one:7.2f} s  {n / t_one:9.0f} records/s, {one.n_calls} calls on {one.pos.size} sites, {one.n_flushes} flushes, "
    f"peak {one.peak_device_bytes / 2**20:.0f} MiB; emit {ms(prof_one, 'pileup_emit') / 1e3:.2f} s, flush {ms(prof_one, 'pileup_flush') / 1e3:.2f} s (events)")
say(f"pileup, --pct-filt 10      : {t_two:7.2f} s  {n / t_two:9.0f} records/s, k_T {two.threshold_k}; emit {ms(prof_two, 'pileup_emit') / 1e3:.2f} s, "
    f"flush {ms(prof_two, 'pileup_flush') / 1e3:.2f} s (events)")
say(f"pileup, 0.25 GiB budget    : {t_tight:7.2f} s  {n / t_tight:9.0f} records/s, {tight.n_flushes} flushes, peak {tight.peak_device_bytes / 2**20:.0f} MiB")

sample = [distinct[i % 512] for i in range(SAMPLE)]
t0 = time.perf_counter()
table = {}
for rec in sample:  # the pileup restated: modified_bases, aligned pairs, a dictionary of counts
    rev = bool(rec["flag"] & 16)
    mods = mr.modified_bases(rec["seq"], rev, rec["mm"], rec["ml"])
    q2r = {q: r for q, r, _ in mr.aligned_pairs(rec["cigar"], rec["pos"]) if q is not None and r is not None}
    q_mod = {}
    for (_, strand, name), vals in mods.items():
        if strand != int(rev) or str(name) not in ALPHABET:
            continue
        for pos, q in vals:
            q_mod.setdefault(pos, {})[name] = 2 * q + 1
    for q, v in q_mod.items():
        r = q2r.get(q)
        if r is None:
            continue
        ks = [v.get(m, 0) for m in ALPHABET[1:]]
        cols = [512 - sum(ks)] + ks
        cls = int(np.argmax(cols))
        table.setdefault((0, r, int(rev)), [0] * (len(ALPHABET) + 1))[cls if cols[cls] >= 308 else len(ALPHABET)] += 1
t_py = time.perf_counter() - t0
say(f"python restatement         : {t_py:7.2f} s  {SAMPLE / t_py:9.0f} records/s over {SAMPLE} records ({len(table)} sites)")
say("RESULT " + json.dumps({"records": n, "bases": LEN, "reader_tokeniser_rps": round(n / t_tok), "validate_rps": round(n / t_val),
                            "pileup_fixed_rps": round(n / t_one), "pileup_pct_rps": round(n / t_two), "pileup_quarter_gib_rps": round(n / t_tight),
                            "pileup_over_validate": round(t_one / t_val, 3), "calls": one.n_calls, "sites": int(one.pos.size),
                            "peak_mib_8gib": round(one.peak_device_bytes / 2**20), "peak_mib_quarter_gib": round(tight.peak_device_bytes / 2**20),
                            "flushes_quarter_gib": tight.n_flushes, "emit_s": round(ms(prof_one, "pileup_emit") / 1e3, 3),
                            "flush_s": round(ms(prof_one, "pileup_flush") / 1e3, 3), "python_restatement_rps": round(SAMPLE / t_py)}))
