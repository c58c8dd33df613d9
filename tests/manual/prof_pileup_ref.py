#!/usr/bin/env python3
"""Records/s of pileup.pileup_modbams with a reference, on the input of tests/manual/prof_pileup.py - 512 distinct records of
LEN bases with a C+hm? entry on every third C, a tenth of them reverse, CIGARs with I / D / S, repeated to RECORDS - whose
reads are here cut from a synthetic 10 Mb reference:
  (a) a checkout of the parent commit without --ref (only with --parent-root DIR, a built checkout: its package is used);
  (b) this code without --ref;  (c) --ref --cpg;  (d) --ref --cpg --combine-strands
and the time and the device bytes of loading a synthetic FASTA of 100 Mb and of 3.1 Gb (31 contigs of 100 Mb), the latter only
where the temporary directory has room.  Every timed run is a process of its own (one warm run on 512 records, then the timed
one); (a) and (b) alternate, REPEATS times each.  Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_pileup_ref.py [RECORDS=200000] [LEN=2000] [REPEATS=5] [--parent-root DIR] [--no-genomes]"""
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


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def worker(mode, bam, small, fa):
    """One timed run in this process, with whatever package the parent process put first on the path."""
    from remora_amd import pileup as rp
    from remora_amd.engine import get_engine

    kw = {"plain": {}, "cpg": dict(ref=fa, motifs=[("CG", 0)]), "comb": dict(ref=fa, motifs=[("CG", 0)], combine_strands=True)}[mode]
    rp.pileup_modbams(small, ALPHABET, filter_threshold=0.6, pct_filt=None, **kw)  # warm everything once
    t_load = None
    if kw:  # the genome once, outside the timed run, as a caller with several BAMs would hold it
        names, lens = zip(*rp.bam_reference_dict(bam))
        t0 = time.perf_counter()
        kw["ref"] = rp.RefGenome.from_fasta(fa, list(names), list(lens))
        t_load = time.perf_counter() - t0
    eng = get_engine(None)
    eng.profile_enable(True)
    eng.profile_reset()
    t0 = time.perf_counter()
    t = rp.pileup_modbams(bam, ALPHABET, filter_threshold=0.6, pct_filt=None, **kw)
    dt = time.perf_counter() - t0
    prof = eng.profile()  # the kernels' own time, from the engine's events
    print("WORKER " + json.dumps({"mode": mode, "seconds": dt, "calls": t.n_calls, "sites": int(t.pos.size), "peak_bytes": t.peak_device_bytes,
                                  "load_seconds": t_load, "emit_ms": prof.get("pileup_emit", (0.0, 0))[0],
                                  "flush_ms": prof.get("pileup_flush", (0.0, 0))[0]}), flush=True)


def run_worker(root, mode, bam, small, fa):
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, bam, small, fa], env=env, cwd=root, stdout=subprocess.PIPE,
                         text=True, check=True, timeout=600).stdout
    return json.loads(next(ln for ln in out.splitlines() if ln.startswith("WORKER "))[7:])


def genome_load(tmp, n_contigs, block):
    from remora_amd import pileup as rp

    path = os.path.join(tmp, f"synthetic_{n_contigs}.fa")
    with open(path, "wb") as fh:
        for c in range(n_contigs):
            fh.write(b">chr%d\n" % (c + 1))
            fh.write(block)
    names, lens = [f"chr{c + 1}" for c in range(n_contigs)], [100_000_020] * n_contigs
    t0 = time.perf_counter()
    g = rp.RefGenome.from_fasta(path, names, lens)
    dt = time.perf_counter() - t0
    nbytes = g.device_bytes
    assert g.read("chr1", 0, 60).tolist() == [{65: 1, 67: 2, 71: 4, 84: 8}[b] for b in block[:60]]
    g.close()
    fbytes = os.path.getsize(path)
    os.remove(path)
    return dt, nbytes, fbytes


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    parent = sys.argv[sys.argv.index("--parent-root") + 1] if "--parent-root" in sys.argv else None
    if parent is not None:
        args.remove(parent)
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
        n_c = (mr.original_sequence(seq, rev)).count("C")
        ords = list(range(0, n_c, 3))
        mm = "C+hm?" + "".join(f",{d}" for d in [0] + [2] * (len(ords) - 1)) + ";"
        cigar = [("S", 20), ("M", m1), ("I", 3), ("M", 200), ("D", 5), ("M", m3), ("S", 10)]
        distinct.append(dict(name=f"r{i}", seq=seq, flag=16 if rev else 0, pos=pos, cigar=cigar, mm=mm, ml=rng.integers(0, 256, 2 * len(ords)).tolist()))
    tmp = tempfile.mkdtemp()
    bam, small, fa = os.path.join(tmp, "tagged.bam"), os.path.join(tmp, "warm.bam"), os.path.join(tmp, "ref.fa")
    blob = b"".join(mr.bam_record(r["name"], r["flag"], 0, r["pos"], r["cigar"], r["seq"], mr.mod_tags(r["mm"], r["ml"])) for r in distinct)
    for path, times in ((bam, max(records // 512, 1)), (small, 1)):
        with rio.BamWriter(path, mr.bam_header([("chr1", REF_LEN)]), level=1) as w:
            for _ in range(times):
                w.write(blob)
    with open(fa, "w") as fh:
        fh.write(">chr1 synthetic\n" + "".join(ref[i : i + 60] + "\n" for i in range(0, REF_LEN, 60)))
    n = max(records // 512, 1) * 512
    say(f"{n} records of {length} bases, {os.path.getsize(bam) / 1e6:.0f} MB BAM; reference of {REF_LEN} bases")

    runs = {"a": [], "b": [], "c": [], "d": []}
    for _ in range(repeats):  # (a) and (b) interleaved
        if parent is not None:
            runs["a"].append(run_worker(parent, "plain", bam, small, fa))
        runs["b"].append(run_worker(ROOT, "plain", bam, small, fa))
    for _ in range(repeats):
        runs["c"].append(run_worker(ROOT, "cpg", bam, small, fa))
        runs["d"].append(run_worker(ROOT, "comb", bam, small, fa))
    result = {"records": n, "bases": length, "repeats": repeats}
    for tag, what in (("a", "parent, no --ref"), ("b", "this code, no --ref"), ("c", "--ref --cpg"), ("d", "--ref --cpg --combine-strands")):
        if not runs[tag]:
            continue
        rps = sorted(n / r["seconds"] for r in runs[tag])
        emit, flush = sorted(r["emit_ms"] for r in runs[tag]), sorted(r["flush_ms"] for r in runs[tag])
        last = runs[tag][-1]
        say(f"({tag}) {what:30s}: records/s min {rps[0]:9.0f} median {rps[len(rps) // 2]:9.0f} max {rps[-1]:9.0f}; {last['calls']} calls on "
            f"{last['sites']} sites, peak {last['peak_bytes'] / 2**20:.0f} MiB" + (f", genome load {last['load_seconds']:.3f} s" if last["load_seconds"] else ""))
        say(f"    emit kernels ms min {emit[0]:7.1f} median {emit[len(emit) // 2]:7.1f} max {emit[-1]:7.1f}; flush ms median {flush[len(flush) // 2]:7.1f}")
        result[tag] = {"rps": [round(x) for x in rps], "emit_ms": [round(x, 1) for x in emit], "flush_ms": [round(x, 1) for x in flush], "calls": last["calls"], "sites": last["sites"], "peak_mib": round(last["peak_bytes"] / 2**20)}
    if "--no-genomes" not in sys.argv:
        body = letters[rng.integers(0, 4, 100_000_020)].reshape(-1, 60)
        block = np.concatenate([body, np.full((body.shape[0], 1), 10, np.uint8)], axis=1).tobytes()
        for n_contigs in (1, 31):
            need = n_contigs * (len(block) + 8)
            free = shutil.disk_usage(tmp).free
            if free < need + (1 << 30):
                say(f"genome of {n_contigs} x 100 Mb: skipped, {free / 1e9:.1f} GB free in {tmp}, {need / 1e9:.1f} GB needed")
                continue
            dt, nbytes, fbytes = genome_load(tmp, n_contigs, block)
            say(f"genome of {n_contigs} x 100 Mb: {fbytes / 1e9:.2f} GB FASTA loaded in {dt:.2f} s ({fbytes / 1e9 / dt:.2f} GB/s), {nbytes / 1e9:.3f} GB on the device")
            result[f"genome_{n_contigs}"] = {"fasta_gb": round(fbytes / 1e9, 3), "seconds": round(dt, 2), "device_gb": round(nbytes / 1e9, 3)}
    shutil.rmtree(tmp, ignore_errors=True)
    say("RESULT " + json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(*sys.argv[2:6])
    else:
        main()
