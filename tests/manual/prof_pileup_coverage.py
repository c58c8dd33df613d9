#!/usr/bin/env python3
"""Records/s of pileup.pileup_modbams with and without `coverage` (--coverage-columns) on the input of prof_pileup.py (512
distinct records of LEN bases with a C+hm? entry on every third C, a tenth of them reverse, CIGARs with I / D / S, repeated to
RECORDS), with a fixed threshold and with the percentile threshold; the peak device memory with and without the flag; the
coverage kernel's time per launch (one batch of 512 records) from the engine's event timing; and, with --parent ROOT (a built
checkout of the parent commit), the run without the flag against that checkout in alternating child processes, REPS each:
medians and min - max.  Every timed run is a child process of its own, so that the two trees never share a process.  For
rocprofv3's view of the kernel run one child, in a run of its own, under
`rocprofv3 --kernel-trace --stats -- python tests/manual/prof_pileup_coverage.py --child ROOT BAM fixed 1` on a BAM written by
`python tests/manual/prof_pileup_coverage.py --write BAM [RECORDS] [LEN]`.
Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_pileup_coverage.py [RECORDS=200000] [LEN=2000] [REPS=5] [--parent ROOT]"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ALPHABET = ["C", "h", "m"]


def child(root, bam, mode, coverage):
    """One timed run in this process, on the package of `root`: a warm-up on the first 512 records, then the whole file."""
    sys.path.insert(0, root)
    from remora_amd import pileup as rp
    from remora_amd.engine import get_engine

    kw = dict(filter_threshold=0.6, pct_filt=None) if mode == "fixed" else dict(pct_filt=10)
    if coverage:
        kw["coverage"] = True
    eng = get_engine(None)
    rp.pileup_modbams(bam + ".warm.bam", ALPHABET, **kw)
    eng.profile_enable(True)
    eng.profile_reset()
    t0 = time.perf_counter()
    table = rp.pileup_modbams(bam, ALPHABET, **kw)
    dt = time.perf_counter() - t0
    prof = eng.profile()
    eng.profile_enable(False)
    cov = getattr(table, "coverage", None)
    print("CHILD " + json.dumps({"seconds": dt, "sites": int(table.pos.size), "calls": int(table.n_calls), "peak": int(table.peak_device_bytes),
                                 "cover": None if cov is None else [int(x) for x in cov.sum(axis=0)],
                                 "prof": {k: [round(v[0], 3), int(v[1])] for k, v in prof.items() if k.startswith("pileup_")}}), flush=True)


def run_child(root, bam, mode, coverage):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, bam, mode, "1" if coverage else "0"], capture_output=True,
                         text=True, timeout=900, cwd=root)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({root}, {mode}, coverage={coverage}):\n{out.stderr[-2000:]}")
    return json.loads(next(line for line in out.stdout.splitlines() if line.startswith("CHILD "))[6:])


def write_input(bam, records, length):
    """prof_pileup.py's records into `bam`, and the first 512 of them into `bam`.warm.bam -> the records written."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import modbam_restate as mr
    import numpy as np

    from remora_amd import io as rio

    rng = np.random.default_rng(1)
    blob = b""
    for i in range(512):  # prof_pileup.py's records
        seq = "".join(rng.choice(list("ACGT"), length))
        rev = i % 10 == 0
        n_c = (mr.original_sequence(seq, rev)).count("C")
        ords = list(range(0, n_c, 3))
        mm = "C+hm?" + "".join(f",{d}" for d in [0] + [2] * (len(ords) - 1)) + ";"
        cigar = [("S", 20), ("M", length // 2 - 30), ("I", 3), ("M", 200), ("D", 5), ("M", length - length // 2 - 193 - 10), ("S", 10)]
        pos = int(rng.integers(1000, 9_000_000))
        blob += mr.bam_record(f"r{i}", 16 if rev else 0, 0, pos, cigar, seq, mr.mod_tags(mm, rng.integers(0, 256, 2 * len(ords)).tolist()))
    header = mr.bam_header([("chr1", 10_000_000)])
    with rio.BamWriter(bam, header, level=1) as w:
        for _ in range(max(records // 512, 1)):
            w.write(blob)
    with rio.BamWriter(bam + ".warm.bam", header, level=1) as w:
        w.write(blob)
    return max(records // 512, 1) * 512


def main(argv):
    parent = None
    if "--parent" in argv:
        parent = os.path.abspath(argv[argv.index("--parent") + 1])
        argv = [a for i, a in enumerate(argv) if a != "--parent" and (i == 0 or argv[i - 1] != "--parent")]
    records = int(argv[0]) if len(argv) > 0 else 200000
    length = int(argv[1]) if len(argv) > 1 else 2000
    reps = int(argv[2]) if len(argv) > 2 else 5
    say = lambda *a: print(" ".join(str(x) for x in a), flush=True)  # noqa: E731
    bam = os.path.join(tempfile.mkdtemp(), "tagged.bam")
    n = write_input(bam, records, length)
    say(f"{n} records of {length} bases, {os.path.getsize(bam) / 1e6:.0f} MB BAM")

    result = {"records": n, "bases": length, "reps": reps}
    spread = lambda xs: f"median {statistics.median(xs):9.0f}  min {min(xs):9.0f}  max {max(xs):9.0f} records/s"  # noqa: E731
    for mode in ("fixed", "pct"):
        off, on, par = [], [], []
        last_on = last_off = None
        for _ in range(reps):  # alternating: parent, this tree without the flag, this tree with it
            if parent is not None:
                par.append(n / run_child(parent, bam, mode, False)["seconds"])
            last_off = run_child(ROOT, bam, mode, False)
            off.append(n / last_off["seconds"])
            last_on = run_child(ROOT, bam, mode, True)
            on.append(n / last_on["seconds"])
        if par:
            say(f"{mode:5s} parent, no flag    : {spread(par)}")
        say(f"{mode:5s} this tree, no flag : {spread(off)}")
        say(f"{mode:5s} --coverage-columns : {spread(on)}")
        ms, launches = last_on["prof"].get("pileup_cover", [0.0, 0])
        say(f"{mode:5s} coverage kernel    : {ms:.1f} ms in {launches} launches = {1e3 * ms / max(launches, 1):.1f} us per batch of 512 records (events); "
            f"emit {last_on['prof'].get('pileup_emit', [0, 0])[0]:.1f} ms against {last_off['prof'].get('pileup_emit', [0, 0])[0]:.1f} ms without")
        say(f"{mode:5s} peak device memory : {last_off['peak'] / 2**20:.1f} MiB without, {last_on['peak'] / 2**20:.1f} MiB with the flag "
            f"({last_on['sites']} sites); N_delete / N_diff / N_nocall totals {last_on['cover']}")
        result[mode] = {"parent_rps": [round(x) for x in par], "off_rps": [round(x) for x in off], "on_rps": [round(x) for x in on],
                        "cover_ms": ms, "cover_launches": launches, "peak_off": last_off["peak"], "peak_on": last_on["peak"],
                        "sites": last_on["sites"], "cover_totals": last_on["cover"],
                        "off_inside_parent_range": bool(par) and min(par) <= statistics.median(off) <= max(par)}
    say("RESULT " + json.dumps(result))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5] == "1")
    elif len(sys.argv) > 2 and sys.argv[1] == "--write":  # the input alone, for a profiler run of one child
        write_input(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 200000, int(sys.argv[4]) if len(sys.argv) > 4 else 2000)
    else:
        main(sys.argv[1:])
