#!/usr/bin/env python3
"""What aggregating k-mer levels in ranges costs against the one pass.

1. The aggregation alone: synthetic observations drawn straight into metrics.SiteLevels (no files) - N_BASES bases of
   reads of READ_LEN bases on both strands of one contig, COVER reads deep on each strand, NaN in 2 % of the values -
   aggregated in one pass (rmr_site_kmer_levels) and in about 2, 8 and 32 ranges (plan_level_ranges; add() clips every batch to the range on the
   device, end_range() runs rmr_site_medians, levels() rmr_kmer_levels_from_sites).  Median seconds of ROUNDS runs after a warm-up,
   each ended by the copy of the table to the host; the peak device memory in use during a run is the largest
   total - free that a thread polling torch.cuda.mem_get_info every few milliseconds sees, less what was in use before the
   observations were drawn.  The tables of all configurations are compared byte for byte.
2. The command line: `analyze estimate_kmer_levels` on the 14 reads of tests/golden/data, CLI_ROUNDS runs in fresh processes,
   of this tree and - when PARENT_TREE names a built checkout of the commit before the ranges - of that tree, alternating:
   what the counting pass adds, beside the run-to-run spread of either.
Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_kmer_levels_ranges.py [N_BASES=200000000] [ROUNDS=5] [CLI_ROUNDS=5] [PARENT_TREE]"""
import json
import os
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N_BASES, ROUNDS, CLI_ROUNDS = (int(float(sys.argv[i])) if len(sys.argv) > i else d for i, d in ((1, 200_000_000), (2, 5), (3, 5)))
PARENT = sys.argv[4] if len(sys.argv) > 4 else None
READ_LEN, COVER, KB_KA, MIN_COV, N_BATCHES = 20_000, 30, (2, 2), 10, 16


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


class PeakMemory:
    """Largest total - free of the device while the block runs, polled from a thread."""

    def __init__(self, torch, dev):
        self.torch, self.dev, self.peak, self._stop = torch, dev, 0, threading.Event()

    def _poll(self):
        while not self._stop.is_set():
            free, total = self.torch.cuda.mem_get_info(self.dev)
            self.peak = max(self.peak, total - free)
            time.sleep(0.003)

    def __enter__(self):
        self._th = threading.Thread(target=self._poll, daemon=True)
        self._th.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._th.join()


def aggregation():
    import torch

    from remora_amd.engine import get_engine
    from remora_amd.metrics import LEVEL_BYTES_PER_BASE, SiteLevels, plan_level_ranges, site_key0

    eng = get_engine(0)
    dev = eng.torch_device
    free, total = torch.cuda.mem_get_info(dev)
    before = total - free
    n_reads = N_BASES // READ_LEN
    ctg_len = max(N_BASES // (2 * COVER), 2 * READ_LEN)  # the reads fall on either strand: COVER deep on each
    rng = np.random.default_rng(1)
    start = rng.integers(0, ctg_len - READ_LEN, size=n_reads)
    rev = rng.random(n_reads) < 0.5
    lens = np.full(n_reads, READ_LEN, np.int64)
    key0 = site_key0(0, np.zeros(n_reads, np.int64), rev, start, lens)
    gen = torch.Generator(device=dev).manual_seed(2)
    ref = torch.randint(0, 4, (ctg_len,), dtype=torch.int8, device=dev, generator=gen)
    batches = []
    for part in np.array_split(np.arange(n_reads), N_BATCHES):
        n = int(lens[part].sum())
        vals = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
        vals[torch.rand(n, device=dev, generator=gen) < 0.02] = float("nan")
        # the bases of a read, read-oriented: the reference forward, or its complement backwards
        pos = torch.arange(READ_LEN, device=dev)[None, :]
        s, r = torch.from_numpy(start[part]).to(dev)[:, None], torch.from_numpy(rev[part]).to(dev)[:, None]
        at = torch.where(r, s + READ_LEN - 1 - pos, s + pos)
        seq = torch.where(r, 3 - ref[at], ref[at]).to(torch.int8).reshape(-1)
        batches.append((vals, seq, key0[part], lens[part]))
        del pos, s, r, at
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(dev)
    say(f"{n_reads} reads of {READ_LEN} bases = {int(lens.sum())} observations on {ctg_len} positions x 2 strands, k-mer context {KB_KA}, "
        f"min_cov {MIN_COV}; observations take {(total - free - before) / 2**30:.2f} GiB")

    def one_pass():
        acc = SiteLevels(eng, KB_KA, MIN_COV)
        for b in batches:
            acc.add(*b)
        return acc.levels(want_sites=True), 1

    def in_ranges(budget):
        def run():
            cuts = plan_level_ranges(key0, lens, budget, *KB_KA)
            acc = SiteLevels(eng, KB_KA, MIN_COV, max_resident_bases=budget)
            for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
                acc.begin_range(a, b)
                for batch in batches:
                    acc.add(*batch)
                acc.end_range()
            return acc.levels(want_sites=True), cuts.size - 1
        return run

    rows, tables = [], []
    total_bases = int(lens.sum())
    configs = [("one pass", one_pass)] + [(f"budget 1/{r}", in_ranges(total_bases // r + 64 * COVER)) for r in (2, 8, 32)]
    for name, run in configs:
        run()  # warm-up
        secs, peak, n_ranges, out = [], 0, None, None
        for _ in range(ROUNDS):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            with PeakMemory(torch, dev) as pm:
                t0 = time.perf_counter()
                out, n_ranges = run()
                secs.append(time.perf_counter() - t0)
            peak = max(peak, pm.peak)
        tables.append(out)
        row = {"config": name, "ranges": int(n_ranges), "median_s": float(np.median(secs)), "min_s": min(secs), "max_s": max(secs),
               "peak_gib_over_observations": (peak - (total - free)) / 2**30, "sites": int(out[1].sum())}
        rows.append(row)
        say(json.dumps(row))
    for t in tables[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(t, tables[0])), "tables differ"
    say(f"all {len(tables)} tables equal byte for byte; {LEVEL_BYTES_PER_BASE} B per resident base planned")
    return rows


def command_line():
    data = os.path.join(ROOT, "tests", "golden", "data")
    pod5, bam, table = (os.path.join(data, f) for f in ("can_reads.pod5", "can_mappings.bam", "levels_4mer.txt"))
    tmp = tempfile.mkdtemp()
    trees = [("this tree", ROOT)] + ([("parent", PARENT)] if PARENT else [])
    secs = {name: [] for name, _ in trees}
    outs = {}
    for rnd in range(CLI_ROUNDS + 1):  # the first round warms the file cache and is dropped
        for name, tree in trees:
            out = os.path.join(tmp, f"{name.replace(' ', '_')}.txt")
            t0 = time.perf_counter()
            subprocess.run([sys.executable, "-m", "remora_amd", "analyze", "estimate_kmer_levels", "--pod5-and-bam", pod5, bam,
                            "--refine-kmer-level-table", table, "--kmer-context-bases", "1", "2", "--min-coverage", "3", "--levels-filename", out],
                           cwd=tree, check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            if rnd:
                secs[name].append(time.perf_counter() - t0)
            outs[name] = open(out, "rb").read()
    for name, s in secs.items():
        say(json.dumps({"cli": name, "median_s": float(np.median(s)), "min_s": min(s), "max_s": max(s), "runs": len(s)}))
    if PARENT:
        assert outs["this tree"] == outs["parent"], "level files differ"
        say("level files of the two trees equal byte for byte")


if __name__ == "__main__":
    if N_BASES > 0:
        aggregation()
    if CLI_ROUNDS > 0:
        command_line()
