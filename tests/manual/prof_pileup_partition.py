#!/usr/bin/env python3
"""Records/s of pileup.pileup_modbams with and without a partition tag on the input of tests/manual/prof_pileup.py with an HP tag
added: 512 distinct records of LEN bases with a C+hm? entry on every third C, a tenth of them reverse, CIGARs with I / D / S,
two of every three with an HP:C tag, 1 or 2 (four bytes a record, which a run without a partition tag walks over); repeated to
RECORDS.  Three runs - a fixed threshold (one pass), the percentile threshold (the histogram pass in front), a 0.25 GiB budget
(several flushes) - beside the reader + tokeniser alone, with the emit, flush and stamp kernels' times from the engine's
events.  Without `--partition-tag` the script calls nothing the commit before the partition tag lacks: run from a built
checkout of that commit (`--root DIR`) it gives the parent's figures on the same input.  Test infrastructure; run by hand on
a GPU box.

    python tests/manual/prof_pileup_partition.py [RECORDS=200000] [LEN=2000] [--partition-tag TAG] [--root DIR]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ARGV = list(sys.argv[1:])
OPTS = {}
for name in ("--partition-tag", "--root"):
    if name in ARGV:
        at = ARGV.index(name)
        OPTS[name] = ARGV[at + 1]
        del ARGV[at : at + 2]
HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(OPTS.get("--root", HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))
import modbam_restate as mr  # noqa: E402

from remora_amd import io as rio  # noqa: E402
from remora_amd import pileup as rp  # noqa: E402
from remora_amd import validate as rv  # noqa: E402
from remora_amd.engine import get_engine  # noqa: E402

RECORDS = int(ARGV[0]) if len(ARGV) > 0 else 200000
LEN = int(ARGV[1]) if len(ARGV) > 1 else 2000
PART = dict(partition_tag=OPTS["--partition-tag"]) if "--partition-tag" in OPTS else {}
REFS = [("chr1", 10_000_000)]
ALPHABET = ["C", "h", "m"]


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


rng = np.random.default_rng(1)
blob = b""
for i in range(512):
    seq = "".join(rng.choice(list("ACGT"), LEN))
    rev = i % 10 == 0
    ords = list(range(0, mr.original_sequence(seq, rev).count("C"), 3))
    mm = "C+hm?" + "".join(f",{d}" for d in [0] + [2] * (len(ords) - 1)) + ";"
    cigar = [("S", 20), ("M", LEN // 2 - 30), ("I", 3), ("M", 200), ("D", 5), ("M", LEN - LEN // 2 - 193 - 10), ("S", 10)]
    tags = mr.mod_tags(mm, rng.integers(0, 256, 2 * len(ords)).tolist()) + (b"HPC" + bytes([1 + i % 3]) if i % 3 < 2 else b"")
    blob += mr.bam_record(f"r{i}", 16 if rev else 0, 0, int(rng.integers(1000, 9_000_000)), cigar, seq, tags)
tmp = tempfile.mkdtemp()
bam, small = os.path.join(tmp, "tagged.bam"), os.path.join(tmp, "warm.bam")
with rio.BamWriter(bam, mr.bam_header(REFS), level=1) as w:
    for _ in range(max(RECORDS // 512, 1)):
        w.write(blob)
with rio.BamWriter(small, mr.bam_header(REFS), level=1) as w:
    w.write(blob)
n = max(RECORDS // 512, 1) * 512
say(f"{n} records of {LEN} bases, {os.path.getsize(bam) / 1e6:.0f} MB BAM; library of {ROOT}; partition tag {PART.get('partition_tag')}")

eng = get_engine(None)
rp.pileup_modbams(small, ALPHABET, pct_filt=10, **PART)  # warm everything once
t0 = time.perf_counter()
for rb, _ in rio.iter_bam_raw_batches(bam, batch=512):
    rv.tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off)
t_tok = time.perf_counter() - t0
say(f"reader + tokeniser         : {t_tok:7.2f} s  {n / t_tok:9.0f} records/s")

result = {"partition_tag": PART.get("partition_tag"), "records": n, "bases": LEN, "reader_tokeniser_rps": round(n / t_tok)}
ms = lambda prof, k: prof.get(k, (0.0, 0))[0]  # noqa: E731
eng.profile_enable(True)
for key, text, kw in (("fixed", "fixed threshold   ", dict(filter_threshold=0.6, pct_filt=None)), ("pct", "--pct-filt 10     ", dict(pct_filt=10)),
                      ("quarter_gib", "0.25 GiB budget   ", dict(filter_threshold=0.6, pct_filt=None, device_gib=0.25))):
    eng.profile_reset()
    t0 = time.perf_counter()
    table = rp.pileup_modbams(bam, ALPHABET, **kw, **PART)
    t = time.perf_counter() - t0
    prof = eng.profile()
    say(f"pileup, {text} : {t:7.2f} s  {n / t:9.0f} records/s, {table.n_calls} calls in {table.pos.size} rows, k_T {table.threshold_k}, "
        f"{table.n_flushes} flushes, peak {table.peak_device_bytes / 2**20:.0f} MiB; emit {ms(prof, 'pileup_emit'):.1f} ms, "
        f"flush {ms(prof, 'pileup_flush'):.1f} ms, stamp {ms(prof, 'pileup_stamp'):.1f} ms in {prof.get('pileup_stamp', (0.0, 0))[1]} launches (events)"
        + (f"; partitions {table.partition_labels}" if PART else ""))
    result.update({f"{key}_rps": round(n / t), f"{key}_emit_ms": round(ms(prof, "pileup_emit"), 2), f"{key}_flush_ms": round(ms(prof, "pileup_flush"), 2),
                   f"{key}_stamp_ms": round(ms(prof, "pileup_stamp"), 2), f"{key}_rows": int(table.pos.size)})
eng.profile_enable(False)
say("RESULT " + json.dumps(result))
