#!/usr/bin/env python3
"""Records/s of pileup.pileup_modbams on duplex-style records: the input of tests/manual/prof_pileup_ref.py - 512 distinct
records of LEN bases cut from a synthetic 10 Mb reference, a C+hm? entry on every third C, a tenth of them reverse, CIGARs with
I / D / S, repeated to RECORDS - with a G-hm? entry added on every G of a CpG of the read:
  (c) --ref --cpg (the '-' entries ignored, as before);  (e) --duplex --ref --cpg;  (f) --hemi --cpg
Every timed run is a process of its own (one warm run on 512 records, then the timed one, the genome loaded outside it), the
three modes in turn, REPEATS times each; the kernels' own time is the engine's (pileup_emit, pileup_pair, pileup_flush).  Test
infrastructure; run by hand on a GPU box.

    python tests/manual/prof_pileup_duplex.py [RECORDS=200000] [LEN=2000] [REPEATS=5]"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ALPHABET = ["C", "h", "m"]
REF_LEN = 10_000_000
MODES = {"c": ("--ref --cpg", {}), "e": ("--duplex --ref --cpg", dict(duplex=True)), "f": ("--hemi --cpg", dict(hemi=True))}


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def worker(mode, bam, small, fa):
    """One timed run in this process."""
    from remora_amd import pileup as rp
    from remora_amd.engine import get_engine

    kw = dict(motifs=[("CG", 0)], **MODES[mode][1])
    rp.pileup_modbams(small, ALPHABET, filter_threshold=0.6, pct_filt=None, ref=fa, **kw)  # warm everything once
    names, lens = zip(*rp.bam_reference_dict(bam))
    genome = rp.RefGenome.from_fasta(fa, list(names), list(lens))
    eng = get_engine(None)
    eng.profile_enable(True)
    eng.profile_reset()
    t0 = time.perf_counter()
    t = rp.pileup_modbams(bam, ALPHABET, filter_threshold=0.6, pct_filt=None, ref=genome, **kw)
    dt = time.perf_counter() - t0
    prof = eng.profile()
    ms = lambda k: prof.get(k, (0.0, 0))[0]  # noqa: E731
    print("WORKER " + json.dumps({"mode": mode, "seconds": dt, "calls": t.n_calls, "sites": int(t.pos.size), "peak_bytes": t.peak_device_bytes,
                                  "unpaired": t.n_unpaired, "emit_ms": ms("pileup_emit"), "pair_ms": ms("pileup_pair"),
                                  "flush_ms": ms("pileup_flush")}), flush=True)


def run_worker(mode, bam, small, fa):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, bam, small, fa], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                         text=True, check=True, timeout=600).stdout
    return json.loads(next(ln for ln in out.splitlines() if ln.startswith("WORKER "))[7:])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    records, length, repeats = (int(args[i]) if len(args) > i else d for i, d in enumerate((200000, 2000, 5)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import modbam_restate as mr

    from remora_amd import io as rio

    rng = np.random.default_rng(1)
    letters = np.frombuffer(b"ACGT", np.uint8)
    ref = letters[rng.integers(0, 4, REF_LEN)].tobytes().decode()
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    m1, m3 = length // 2 - 30, length - length // 2 - 193 - 10
    distinct = []
    for i in range(512):
        rev, pos = i % 10 == 0, int(rng.integers(1000, 9_000_000))
        seq = rand(20) + ref[pos : pos + m1] + rand(3) + ref[pos + m1 : pos + m1 + 200] + ref[pos + m1 + 205 : pos + m1 + 205 + m3] + rand(10)
        orig = mr.original_sequence(seq, rev)
        ords = list(range(0, orig.count("C"), 3))
        mm = "C+hm?" + "".join(f",{d}" for d in [0] + [2] * (len(ords) - 1)) + ";"
        # the G of every CpG of the read, as an ordinal among its G
        g_at = [p for p, b in enumerate(orig) if b == "G"]
        g_ords = [k for k, p in enumerate(g_at) if p > 0 and orig[p - 1] == "C"]
        mm += "G-hm?" + "".join(f",{d}" for d in [g_ords[0]] + [b - a - 1 for a, b in zip(g_ords, g_ords[1:])]) + ";"
        cigar = [("S", 20), ("M", m1), ("I", 3), ("M", 200), ("D", 5), ("M", m3), ("S", 10)]
        distinct.append(dict(name=f"r{i}", seq=seq, flag=16 if rev else 0, pos=pos, cigar=cigar, mm=mm,
                             ml=rng.integers(0, 256, 2 * (len(ords) + len(g_ords))).tolist()))
    tmp = tempfile.mkdtemp()
    bam, small, fa = os.path.join(tmp, "duplex.bam"), os.path.join(tmp, "warm.bam"), os.path.join(tmp, "ref.fa")
    blob = b"".join(mr.bam_record(r["name"], r["flag"], 0, r["pos"], r["cigar"], r["seq"], mr.mod_tags(r["mm"], r["ml"])) for r in distinct)
    for path, times in ((bam, max(records // 512, 1)), (small, 1)):
        with rio.BamWriter(path, mr.bam_header([("chr1", REF_LEN)]), level=1) as w:
            for _ in range(times):
                w.write(blob)
    with open(fa, "w") as fh:
        fh.write(">chr1 synthetic\n" + "".join(ref[i : i + 60] + "\n" for i in range(0, REF_LEN, 60)))
    n = max(records // 512, 1) * 512
    say(f"{n} records of {length} bases, {os.path.getsize(bam) / 1e6:.0f} MB BAM; reference of {REF_LEN} bases")

    runs = {tag: [] for tag in MODES}
    for _ in range(repeats):
        for tag in MODES:
            runs[tag].append(run_worker(tag, bam, small, fa))
    result = {"records": n, "bases": length, "repeats": repeats}
    for tag, (what, _) in MODES.items():
        rps = sorted(n / r["seconds"] for r in runs[tag])
        med = lambda key: sorted(r[key] for r in runs[tag])[len(runs[tag]) // 2]  # noqa: E731
        last = runs[tag][-1]
        say(f"({tag}) {what:22s}: records/s min {rps[0]:9.0f} median {rps[len(rps) // 2]:9.0f} max {rps[-1]:9.0f}; {last['calls']} "
            f"{'pairs' if tag == 'f' else 'calls'} on {last['sites']} sites" + (f", {last['unpaired']} calls unpaired" if tag == "f" else "") +
            f", peak {last['peak_bytes'] / 2**20:.0f} MiB")
        say(f"    kernels ms (median): emit {med('emit_ms'):7.1f}  pair {med('pair_ms'):6.1f}  flush {med('flush_ms'):7.1f}  of {1000 * n / rps[len(rps) // 2]:8.0f} ms")
        result[tag] = {"rps": [round(x) for x in rps], "emit_ms": round(med("emit_ms"), 1), "pair_ms": round(med("pair_ms"), 1),
                       "flush_ms": round(med("flush_ms"), 1), "calls": last["calls"], "sites": last["sites"], "unpaired": last["unpaired"],
                       "peak_mib": round(last["peak_bytes"] / 2**20)}
    shutil.rmtree(tmp, ignore_errors=True)
    say("RESULT " + json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(*sys.argv[2:6])
    else:
        main()
