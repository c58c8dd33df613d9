#!/usr/bin/env python3
"""bench.py — chunks/sec of the fused per-read modified-base-call hot path on MI355X.

A step = one pass of the hot path (chunk arrays -> class logits + per-label counts) over the rank's batch of
synthetic chunks, inputs already resident in HBM.  One process per GPU; chunks shard across ranks with no data-path
collective; the only exchange is one all-reduce of the per-label counts (RCCL over xGMI) at the end of the timed
region.

    python bench.py                          # 1 GPU: the headline config alone (set up, warm up, timed steps, result line)
    python bench.py --full                   # + the side legs, the CPU baseline, the other BASELINE configs, the precision
                                             #   check and the C-ABI collective check (the --no-* options trim it)
    python bench.py --gpus N [...]           # launches N ranks itself (torch.distributed.run) when not under torchrun
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W            # the driver's form: RANK/LOCAL_RANK/WORLD_SIZE from the env

Workloads (BASELINE.json `configs`): convlstm_c100 = configs[2] (the config the metric is quoted on; default, fp32),
conv_c100 = configs[1], convlstm_c100_bf16_10m = configs[3] (10 M chunks strong-sharded over the ranks, bf16),
convlstm_c200_bf16 = configs[4] (3-class, 200-sample chunks, bf16).  `--dtype` overrides a workload's arithmetic.

Prints ONE JSON line on rank 0 (contract in the task statement; the `roofline` object from the timed steps' own kernel
events; `cpu_baseline` and the CPU-checked `parity` figures with --full).  A world size that differs from --gpus is an
error, never a silently smaller run.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    "convlstm_c100": dict(arch="conv_lstm", cfg="C100", dtype="fp32", chunks=1_000_000, scaling="weak", baseline_config=2,
                          desc="synthetic 100-sig-pt CG chunks, ConvLSTM_w_ref size 64 k-mer (4,4) 2-class (BASELINE configs[2])"),
    "conv_c100": dict(arch="conv_only", cfg="C100", dtype="fp32", chunks=1_000_000, scaling="weak", baseline_config=1,
                      desc="synthetic 100-sig-pt CG chunks, Conv_w_ref size 64 (BASELINE configs[1])"),
    "convlstm_c100_bf16_10m": dict(arch="conv_lstm", cfg="C100", dtype="bf16", chunks=10_000_000, scaling="strong", baseline_config=3,
                                   desc="synthetic 10M 100-sig-pt CG chunks read-sharded over the ranks, ConvLSTM_w_ref bf16 "
                                        "(BASELINE configs[3])"),
    # a network of 128 channels (`--size 128`, src/remora/parsers.py:858-862): the streamed-weight kernels (k_stream.hip)
    "convlstm_c100_s128": dict(arch="conv_lstm", cfg="C100", dtype="fp32", chunks=500_000, scaling="weak", baseline_config=None, size=128,
                               desc="synthetic 100-sig-pt CG chunks, ConvLSTM_w_ref size 128 k-mer (4,4) 2-class (the shape of "
                                    "BASELINE configs[2] at twice the channels)"),
    # the shape of configs[4] with torch's DEFAULT weight scale (synth_state(amplify=False): what a reference-initialised network
    # looks like, e.g. the golden models) in fp32: the fp32 parity of this shape is gated here at north_star's fixed 1e-4 against
    # the oracle's fp32 forward AND float64.  (The other synthetic networks are amplified on purpose - conv x 2.45, LSTM x 2.5, fc x
    # 12 - so that the 16-bit gates see every layer; at C200 the amplified one carries 1.35e-4 of the REFERENCE's own fp32 rounding.)
    "convlstm_c200_refinit": dict(arch="conv_lstm", cfg="C200", dtype="fp32", chunks=250_000, scaling="weak", baseline_config=4, init="reference",
                                  desc="synthetic 200-sig-pt all-context chunks, 3-class ConvLSTM_w_ref with torch's default weight "
                                       "scale (the shape of BASELINE configs[4]; fp32 parity gate)"),
    "convlstm_c200_bf16": dict(arch="conv_lstm", cfg="C200", dtype="bf16", chunks=1_000_000, scaling="weak", baseline_config=4,
                               desc="synthetic 200-sig-pt all-context chunks, 3-class 5mC+5hmC ConvLSTM_w_ref bf16 "
                                    "(BASELINE configs[4])"),
}
# what a default 1-GPU run measures beside the headline: (key, workload, dtype override, chunks override)
OTHER_CONFIGS = [
    ("conv_c100", "conv_c100", None, None),
    ("convlstm_c100_bf16", "convlstm_c100", "bf16", None),
    ("convlstm_c100_bf16_10m", "convlstm_c100_bf16_10m", None, None),
    ("convlstm_c200_refinit_fp32", "convlstm_c200_refinit", None, None),  # the fp32 parity gate of the C200 shape (fixed 1e-4)
    ("convlstm_c200_fp32", "convlstm_c200_bf16", "fp32", None),  # amplified network: the comparand of the 16-bit runs of its shape below
    ("convlstm_c200_bf16", "convlstm_c200_bf16", None, None),
    ("convlstm_c100_f16", "convlstm_c100", "f16", None),
    ("convlstm_c200_f16", "convlstm_c200_bf16", "f16", None),
    ("convlstm_c100_bf16x6", "convlstm_c100", "bf16x6", None),
    ("convlstm_c100_bf16x3", "convlstm_c100", "bf16x3", None),
    ("convlstm_c100_f16x3", "convlstm_c100", "f16x3", None),
    ("convlstm_c100_s128_fp32", "convlstm_c100_s128", None, None),
]

PEAK_BF16_MFMA_TFLOPS = 2500.0
PEAK_FP32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, 256 CUs @ 2.4 GHz
PEAK_HBM_GBS = 8000.0
DTYPE_OUT = {"fp32": "f32"}
PRECISION_CHUNKS = 8192  # chunks of the headline data evaluated on the CPU (fp64 + fp32) for the `parity` / `precision` objects
DUMP_LIMIT = 64 << 20  # bytes: what --dump-outputs writes in all
LINE_LIMIT = 4096  # bytes: the ONE stdout line stays below this (the driver keeps a bounded tail); the rest -> bench_details.json
BLOCK = 1_000_000  # the synthetic data set is defined in blocks of 1 M chunks (seed = base + block index)


def geometry(arch, L):
    kw1 = 5 if arch == "conv_lstm" else 11
    P1 = L - kw1 + 1
    P2 = P1 - kw1 + 1
    P3 = (P2 - 9) // 3 + 1
    return kw1, P1, P2, P3


def kernel_flops_per_chunk(arch, L, size=64, K=9, num_out=2):
    """ALGORITHMIC flops (2 per MAC) per chunk of each kernel (no credit for lstm2's dead steps or for
    multiplying one-hot zeros)."""
    kw1, P1, P2, P3 = geometry(arch, L)
    f = {}
    f["conv_sig3"] = 2 * size * 16 * 9 * P3
    f["front_sig"] = 2 * (4 * kw1 * P1 + 16 * 4 * kw1 * P2)
    f["front_seq"] = 16 * K * kw1 * P1  # seq_conv1 as K*kw1 gather-adds x 16 channels
    if arch == "conv_lstm":
        T = P3 - 4
        f["conv_seq2"] = 2 * size * 16 * 13 * P3
        f["conv_merge1"] = 2 * size * 2 * size * 5 * T
        f["lstm_head"] = 2 * (T * 2 * 4 * size * size + 4 * size * size + num_out * size)
        # the fused bf16 front kernel (k_fused.hip) does the work of the five kernels above it
        f["fused_front"] = f["front_sig"] + f["front_seq"] + f["conv_sig3"] + f["conv_seq2"] + f["conv_merge1"]
        # fp32: the producers folded into the staging of their consumer (k_conv_front.hip)
        f["sig3_front"] = f["front_sig"] + f["conv_sig3"]
        f["seq2_front"] = f["front_seq"] + f["conv_seq2"]
    else:
        PQ2 = P1 - 10
        T, T2 = P3 - 4, P3 - 8
        T3 = (T2 - 3) // 2 + 1
        T4 = (T3 - 3) // 2 + 1
        f["conv_seq2"] = 2 * 32 * 16 * 11 * PQ2
        f["conv_seq3"] = 2 * size * 32 * 9 * P3
        f["conv_merge1"] = 2 * size * 2 * size * 5 * T
        f["conv_merge2"] = 2 * size * size * 5 * T2
        f["conv_merge3"] = 2 * size * size * 3 * T3
        f["conv_merge4"] = 2 * size * size * 3 * T4
        f["fc_head"] = 2 * num_out * size * T4
        f["sig3_front"] = f["front_sig"] + f["conv_sig3"]  # the signal branch folded (k_conv_front.hip, matrix-core producer)
    return f


def kernel_alg_bytes_per_chunk(arch, L, dtype, size=64, num_out=2, seq_w=28, map_w=21):
    """ALGORITHMIC HBM bytes per chunk of the matrix kernels: the tensors each one has to read and write once
    (fp32 channel-last activations in the unfused pipelines, bf16 x between the two fused bf16 kernels)."""
    kw1, P1, P2, P3 = geometry(arch, L)
    T = P3 - 4
    b = {"conv_sig3": P2 * 16 * 4 + P3 * size * 4, "conv_merge1": P3 * 2 * size * 4 + T * size * 4}
    if arch == "conv_lstm":
        b["conv_seq2"] = P1 * 16 * 4 + P3 * size * 4
        b["lstm_head"] = T * size * (2 if dtype in ("bf16", "f16") else 4) + 4 * num_out
        b["fused_front"] = L * 4 + seq_w + 2 * map_w + 2 + T * size * 2
        b["sig3_front"] = L * 4 + P3 * size * 4
        b["seq2_front"] = seq_w + 2 * map_w + 2 + P3 * size * 4
    return b


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args_list, n):
    """Not under torchrun and more than one GPU asked for: start the ranks ourselves (one process per GPU)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + args_list
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if "OMP_NUM_THREADS" not in env:
        env["OMP_NUM_THREADS"] = "8"
        env["REMORA_AMD_LAUNCHER_SIZED"] = "OMP_NUM_THREADS"  # dist.bind_rank may refine it; a user's value stays
    return subprocess.call(cmd, env=env)


_BLOCK0 = {}


def synth_range(cfg, start, stop, full_blocks=False, threads=16):
    """Chunks [start, stop) of the synthetic data set of SURVEY §8(d): block b (1 M chunks) is generated from seed
    base + b, so every rank / run sees the same data for the same global chunk index."""
    from concurrent.futures import ThreadPoolExecutor

    from remora_amd import synth

    blocks = list(range(start // BLOCK, (stop - 1) // BLOCK + 1))

    def gen(b):
        lo, hi = max(start, b * BLOCK), min(stop, (b + 1) * BLOCK)
        # whole blocks whenever a range crosses or splits one (so that a global chunk index means the same chunk for
        # every partition of the data set); a short run inside one block generates just its own length
        n_gen = BLOCK if (full_blocks or lo > b * BLOCK) else hi - b * BLOCK
        d = _BLOCK0.get((cfg, b, n_gen))
        if d is None:
            d = synth.synth_chunks_config(cfg, n_gen, shard=b)
            if b == 0:  # block 0 is shared by several configs of a default run: generate it once
                _BLOCK0[(cfg, b, n_gen)] = d
        return {k: (v[lo - b * BLOCK : hi - b * BLOCK] if isinstance(v, np.ndarray) else v) for k, v in d.items()}

    if len(blocks) == 1:
        parts = [gen(blocks[0])]
    else:
        with ThreadPoolExecutor(min(threads, len(blocks))) as ex:
            parts = list(ex.map(gen, blocks))
    out = {}
    for k, v in parts[0].items():
        out[k] = np.concatenate([p[k] for p in parts]) if isinstance(v, np.ndarray) else v
    return out


def precision_check(state, data, kcb, gpu_logits, full=None):
    """Max |logit error| of each GPU path against a float64 CPU evaluation of the same network on the first
    PRECISION_CHUNKS chunks (and the fp32 CPU reference's own error, for scale); argmax agreement over all of them and
    over those whose float64 margin exceeds 2e-2.  `full`: {name: (logits, fp32-path logits)} device tensors over the whole
    step — the reduced-precision paths against the fp32 GPU path on every chunk (the fp32 path itself sits ~4e-6 from
    float64, so it stands in for the exact answer where the CPU cannot cover 1 M chunks in the run)."""
    import torch

    from oracle import oracle as O
    from oracle import torch_ref

    k = min(PRECISION_CHUNKS, data["sequence_lengths"].shape[0])
    enc = O.compute_encoded_kmer_batch(kcb[0], kcb[1], data["sequence"][:k], data["sequence_to_signal_mapping"][:k],
                                       data["sequence_lengths"][:k])
    sig = torch.from_numpy(data["signal"][:k])
    from remora_amd.util import effective_cpu_count

    torch.set_num_threads(min(32, effective_cpu_count()))
    with torch.no_grad():
        ref64 = torch_ref.from_state(state).double()(sig.double(), torch.from_numpy(enc).double()).numpy()
        ref32 = torch_ref.from_state(state)(sig, torch.from_numpy(enc)).numpy()
    srt = np.sort(ref64, axis=1)
    margin = srt[:, -1] - srt[:, -2]
    clear = margin > 2e-2
    out = {"chunks": k, "chunks_with_margin_gt_2e-2": int(clear.sum()), "cpu_fp32_reference_vs_fp64": float(np.abs(ref32 - ref64).max())}
    for name, lg in gpu_logits.items():
        if lg is not None:
            agree = lg[:k].argmax(1) == ref64.argmax(1)
            out[f"{name}_vs_fp64"] = float(np.abs(lg[:k] - ref64).max())
            out[f"{name}_vs_cpu_fp32_reference"] = float(np.abs(lg[:k] - ref32).max())
            out[f"{name}_argmax_agreement_with_fp64"] = float(agree.mean())
            out[f"{name}_argmax_agreement_with_fp64_margin_gt_2e-2"] = float(agree[clear].mean()) if clear.any() else None
    for name, (lg, ref) in (full or {}).items():
        d = (lg - ref).abs()
        top = ref.topk(2, dim=1).values
        clr = (top[:, 0] - top[:, 1]) > 2e-2
        agree = lg.argmax(1) == ref.argmax(1)
        out[f"{name}_vs_fp32_gpu_path_all_chunks"] = {
            "chunks": int(lg.shape[0]), "max_abs": float(d.max()), "mean_abs": float(d.mean()),
            "argmax_agreement": float(agree.float().mean()), "chunks_with_margin_gt_2e-2": int(clr.sum()),
            "argmax_agreement_margin_gt_2e-2": float(agree[clr].float().mean()) if bool(clr.any()) else None}
    return out


def cpu_baseline(state, data, kcb, budget_s=12.0):
    """The reference CPU path timed on this box's host cores: single-thread C restatement of the Cython
    encode + torch.nn restatement of the network, batch 2048, fp32.  `value` = eager with torch.set_num_threads(usable cores)
    (the survey's prescription), median of three repeats; torch.jit.script at the same thread count (what the reference's
    load_model returns, src/remora/model_util.py:115-117) and eager at the fastest thread count of a probe are timed once
    each for the details file."""
    import torch

    from oracle import oracle as O
    from oracle import torch_ref

    from remora_amd.util import effective_cpu_count

    # "all cores" = the cores this process may use: containers show every host core in os.cpu_count() (256 on the MI355X
    # boxes of this pool) while the cgroup grants 16 - a 256-thread intra-op pool on 16 cores runs at 150 chunks/s
    host_cores = effective_cpu_count()
    net = torch_ref.from_state(state)
    net.eval()
    B = 2048
    n_avail = data["sequence_lengths"].shape[0]
    npb = min(B, n_avail)
    probe_enc = O.compute_encoded_kmer_batch(kcb[0], kcb[1], data["sequence"][:npb], data["sequence_to_signal_mapping"][:npb],
                                             data["sequence_lengths"][:npb])
    probe = (torch.from_numpy(data["signal"][:npb]), torch.from_numpy(probe_enc))
    tuned, per_batch_s = {}, {}
    with torch.no_grad():
        for nt in sorted({host_cores, max(host_cores // 2, 1), 2 * host_cores, 32, 16, 8}, reverse=True):
            if nt > (os.cpu_count() or 1):
                continue
            torch.set_num_threads(nt)
            t0 = time.perf_counter()
            net(*probe)
            best = time.perf_counter() - t0
            if best < 1.0:  # cheap enough to repeat: best of 3 more
                for _ in range(3):
                    t0 = time.perf_counter()
                    net(*probe)
                    best = min(best, time.perf_counter() - t0)
            tuned[nt], per_batch_s[nt] = npb / best, best
    best_threads = max(tuned, key=tuned.get)
    jit_err = None
    try:
        jit_net = torch.jit.script(net)
    except Exception as e:  # noqa: BLE001 - reported, not fatal: the eager forms still stand
        jit_net, jit_err = None, str(e)

    def timed(model, threads, budget, warm=2):
        torch.set_num_threads(threads)
        t_enc = t_net = 0.0
        done = it = 0
        with torch.no_grad():
            while True:
                st = (it * B) % max(n_avail - B, 1)
                sl = slice(st, st + B)
                t0 = time.perf_counter()
                enc = O.compute_encoded_kmer_batch(kcb[0], kcb[1], data["sequence"][sl], data["sequence_to_signal_mapping"][sl],
                                                   data["sequence_lengths"][sl])
                t1 = time.perf_counter()
                model(torch.from_numpy(data["signal"][sl]), torch.from_numpy(enc))
                t2 = time.perf_counter()
                if it >= warm:
                    t_enc += t1 - t0
                    t_net += t2 - t1
                    done += B
                it += 1
                if (done and (t_enc + t_net) >= budget) or it >= 400:
                    break
        return {"chunks_per_s": done / (t_enc + t_net), "encode_chunks_per_s": done / t_enc, "model_chunks_per_s": done / t_net,
                "threads": threads, "chunks": done, "warmup_batches": warm}

    # torch's intra-op pool collapses when every core of a large host is asked for on this small network (one batch can take
    # >10 s on 256 cores): such a form is not re-timed — the probe's own batch IS its measurement, and the scripted form at
    # the same thread count is skipped with that reason (two more warm-up passes would cost a minute of the default run)
    slow_all = per_batch_s.get(host_cores, 0.0) > 2.0
    # The line's `value` is ONE fixed form - eager, every usable core (the survey's prescription; with the cgroup's core count
    # for os.cpu_count()) - as the MEDIAN of three repeats: the fastest-of-three-forms of round 3 flipped between eager and
    # scripted from box to box (46.7 k vs 70.4 k chunks/s).  The scripted form and the probe's best thread count are timed once
    # each and stay in the details file.  (A host whose all-cores pool collapses - >2 s per batch - is measured at the probe's
    # best thread count instead, and says so.)
    head_threads = best_threads if slow_all else host_cores
    head = "eager_best_threads" if slow_all else "eager_all_cores"
    repeats = [timed(net, head_threads, budget_s / 5) for _ in range(3)]
    rates = sorted(r["chunks_per_s"] for r in repeats)
    med = [r for r in repeats if r["chunks_per_s"] == rates[1]][0]
    forms = {head: dict(med, repeats_chunks_per_s=[r["chunks_per_s"] for r in repeats], statistic="median of 3")}
    if slow_all:
        forms["eager_all_cores"] = {"chunks_per_s": tuned[host_cores], "threads": host_cores, "chunks": npb, "warmup_batches": 0,
                                    "note": f"one batch took {per_batch_s[host_cores]:.1f} s (network only, the thread probe's measurement)"}
        forms["jit_script_all_cores"] = {"skipped": f"eager at {host_cores} threads takes {per_batch_s[host_cores]:.1f} s per batch of {npb}"}
    else:
        forms["jit_script_all_cores"] = timed(jit_net, host_cores, budget_s / 5) if jit_net is not None else {"error": jit_err}
        forms["eager_best_threads"] = timed(net, best_threads, budget_s / 5) if best_threads != host_cores else {"same_as": "eager_all_cores"}
    return {
        "value": med["chunks_per_s"], "unit": "chunks/s", "cores": med["threads"], "host_cores": host_cores,
        "os_cpu_count": os.cpu_count(), "kind": "port",
        "headline_form": head, "statistic": "median of 3 repeats of one fixed form",
        "repeats_chunks_per_s": [r["chunks_per_s"] for r in repeats],
        "sample": f"3 x {med['chunks']} chunks in batches of {B} (median): C port of compute_encoded_kmer_batch (1 thread) + torch.nn "
                  f"restatement of the network, fp32, eager, {med['threads']} torch threads ({host_cores} usable cores: "
                  f"cgroup quota; os.cpu_count() {os.cpu_count()})",
        "forms": forms, "thread_probe_chunks_per_s": {str(k): v for k, v in tuned.items()},
        "encode_chunks_per_s": med.get("encode_chunks_per_s"), "model_chunks_per_s": med.get("model_chunks_per_s"),
    }

# Specified parity gates per dtype (round-4 review item 7; SURVEY §7 "hard parts"): fp32-class paths by the logit error against
# the oracle's fp32 forward, 16-bit paths by the share of confident calls (fp32 margin > 2e-2) they reproduce.
PARITY_GATES = {
    "fp32": {"max_abs_vs_oracle": 1e-4}, "bf16x6": {"max_abs_vs_oracle": 1e-4}, "f16x3": {"max_abs_vs_oracle": 1e-4},
    "bf16x3": {"max_abs_vs_oracle": 5e-4},
    "f16": {"argmax_agreement_margin_gt_2e-2": 0.9999}, "bf16": {"argmax_agreement_margin_gt_2e-2": 0.998},
}
PARITY_SAMPLE = 20_000


def config_parity(job, fp32_logits=None, comparand_only=False):
    """`parity` of one configuration: its logits on the first PARITY_SAMPLE chunks of rank 0's data against the ORACLE's
    forward in float64 (CPU: C restatement of the encode + torch.nn restatement of the network - not this library), and, where the fp32
    GPU path of the same workload ran in this process (`fp32_logits`, device), over EVERY chunk of the step against it; the
    gate of the dtype (PARITY_GATES) and whether it is met."""
    import torch

    from oracle import oracle as O
    from oracle import torch_ref
    from remora_amd.util import effective_cpu_count

    k = min(PARITY_SAMPLE, job.n)
    d = job.data
    enc = O.compute_encoded_kmer_batch(job.kcb[0], job.kcb[1], d["sequence"][:k], d["sequence_to_signal_mapping"][:k], d["sequence_lengths"][:k])
    torch.set_num_threads(min(32, effective_cpu_count()))
    with torch.no_grad():  # float64: the comparand's own rounding (1e-4 at C200 in fp32) stays out of the fp32-class gates
        ref = torch_ref.from_state(job.state).double()(torch.from_numpy(d["signal"][:k]).double(), torch.from_numpy(enc).double()).numpy()
        ref32 = torch_ref.from_state(job.state)(torch.from_numpy(d["signal"][:k]), torch.from_numpy(enc)).numpy()
    ref32_err = float(np.abs(ref32.astype(np.float64) - ref).max())  # what the reference's own fp32 arithmetic loses on this sample
    got = job.logits[:k].cpu().numpy().astype(np.float64)
    srt = np.sort(ref, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 2e-2
    agree = got.argmax(1) == ref.argmax(1)
    out = {"comparand": "oracle network evaluated in float64 (CPU restatement)", "sample_chunks": int(k), "max_abs_vs_oracle": float(np.abs(got - ref).max()),
           "mean_abs_vs_oracle": float(np.abs(got - ref).mean()), "sample_chunks_with_margin_gt_2e-2": int(clear.sum()),
           "sample_argmax_agreement_margin_gt_2e-2": float(agree[clear].mean()) if clear.any() else None}
    if fp32_logits is not None and fp32_logits.shape == job.logits.shape and job.dtype != "fp32":
        top = fp32_logits.topk(2, dim=1).values
        clr = (top[:, 0] - top[:, 1]) > 2e-2
        ag = job.logits.argmax(1) == fp32_logits.argmax(1)
        dd = (job.logits - fp32_logits).abs()
        out.update({"all_chunks": int(job.logits.shape[0]), "all_chunks_comparand": "fp32 GPU path of the same workload",
                    "max_abs_vs_fp32_path": float(dd.max()), "chunks_with_margin_gt_2e-2": int(clr.sum()),
                    "argmax_agreement_margin_gt_2e-2": float(ag[clr].float().mean()) if bool(clr.any()) else None,
                    "argmax_agreement_all": float(ag.float().mean())})
    out["oracle_fp32_forward_vs_float64"] = ref32_err
    out["max_abs_vs_oracle_fp32_forward"] = float(np.abs(got - ref32.astype(np.float64)).max())
    gate = dict(PARITY_GATES.get(job.dtype, {}))
    if "max_abs_vs_oracle" in gate and job.dtype == "fp32":
        gate["max_abs_vs_oracle_fp32_forward"] = gate["max_abs_vs_oracle"]  # fp32: both comparands, the same fixed number
    if comparand_only:
        # the amplified C200 network in fp32: run as the all-chunks comparand of the 16-bit configurations of its shape; the
        # reference's OWN fp32 forward sits `oracle_fp32_forward_vs_float64` from float64 on it (1.35e-4), so 1e-4 against float64
        # is not a property an fp32 implementation can have there - the fp32 gate of this shape is convlstm_c200_refinit_fp32
        gate = {}
        out["gate_note"] = "no gate: amplified network, comparand of the 16-bit gates (fp32 parity of this shape: convlstm_c200_refinit_fp32)"
    out["gate"] = gate
    met = True
    for key, lim in gate.items():
        val = out.get(key, out.get("sample_" + key))
        met = met and val is not None and (val <= lim if key.startswith("max_abs") else val >= lim)
    out["gate_met"] = bool(met)
    return out


class Job:
    """One workload on this rank: model, resident inputs, and the timed loop."""

    def __init__(self, workload, dtype, chunks, rank, world, local, subbatch=0, shard_base=0):
        import torch

        from remora_amd import dist as rdist
        from remora_amd import synth
        from remora_amd.engine import get_engine
        from remora_amd.model_util import model_from_state

        w = WORKLOADS[workload]
        self.w, self.workload, self.dtype = w, workload, dtype or w["dtype"]
        self.arch, self.cfg, self.size = w["arch"], w["cfg"], int(w.get("size", 64))
        self.cc, self.kcb, _, self.num_out, _ = synth.CONFIGS[self.cfg]
        self.L = sum(self.cc)
        self.rank, self.world, self.local = rank, world, local
        total = chunks or w["chunks"]
        if w["scaling"] == "strong":  # a fixed data set, contiguous ranges per rank (dist.shard_range)
            self.start, self.stop = rdist.shard_range(total, rank, world)
            self.total_chunks_per_step = total
        else:  # weak: every rank its own `total` chunks; rank r takes the blocks after rank r-1's
            per = total
            nblk = (per + BLOCK - 1) // BLOCK
            self.start = (shard_base + rank) * nblk * BLOCK
            self.stop = self.start + per
            self.total_chunks_per_step = per * world
        self.n = self.stop - self.start
        self.eng = get_engine(local)
        if subbatch:
            self.eng.set_subbatch(subbatch)
        self.md = dict(chunk_context=self.cc, kmer_context_bases=self.kcb)
        state = synth.synth_state(self.arch, self.size, sum(self.kcb) + 1, self.num_out, seed=0, amplify=w.get("init") != "reference")
        # centre the class logits (random weights otherwise call one class for every chunk): shift fc.bias by the per-class
        # median of the logits of a FIXED probe set (block 0 of the data set, first 8192 chunks) — every rank computes the
        # same shift from the same data with the same kernels, no broadcast needed
        probe = synth.synth_chunks_config(self.cfg, 8192, shard=0)
        pm = model_from_state(state, self.md, device=local, dtype="fp32")
        pl = pm.infer_chunks(probe["signal"], probe["sequence"], probe["sequence_to_signal_mapping"], probe["sequence_lengths"], self.kcb)
        state["fc.bias"] = (state["fc.bias"].astype(np.float64) - np.median(pl, axis=0).astype(np.float64)).astype(np.float32)
        del pm
        self.state = state
        self.model = model_from_state(state, self.md, device=local, dtype=self.dtype)
        self.data = synth_range(self.cfg, self.start, self.stop, full_blocks=w["scaling"] == "strong")
        self.dev = [torch.from_numpy(self.data[k]).cuda(local) for k in
                    ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")]
        self.counts = torch.zeros(self.num_out, dtype=torch.int64, device=f"cuda:{local}")
        self.logits = None

    def step(self):
        self.logits = self.model.infer_chunks(*self.dev, self.kcb, label_counts=self.counts)

    def host_buffers_leg(self, device_logits=None, reps=2, max_chunks=1 << 20):
        """The same job handed over as HOST buffers (numpy, pageable) through the C-ABI boundary: host copy into pinned slots,
        H2D, kernels, logits + label counts D2H - the PCIe-inclusive rate (never `value`: the task's contract times resident
        inputs).  At 472 B (C100) / 932 B (C200) per chunk a PCIe Gen5 x16 link (63 GB/s spec) carries at most ~130 M / ~65 M
        chunks/s: the 16-bit configs' resident rates are kernel rates, this leg is what a host-fed caller gets."""
        n = min(self.n, max_chunks)
        host = [self.data[k][:n] for k in ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")]
        hc = np.zeros(self.num_out, np.int64)
        self.model.infer_chunks(*host, self.kcb)  # warm-up (staging arenas, pinned slots)
        t0 = time.perf_counter()
        for _ in range(reps):
            lg_h = self.model.infer_chunks(*host, self.kcb, label_counts=hc)
        t1 = time.perf_counter()
        bpc = int(sum(a[0:1].nbytes for a in host) + 4 * self.num_out)
        rate = reps * n / (t1 - t0)
        leg = {"chunks_per_s": rate, "ms_per_step": (t1 - t0) / reps * 1e3, "chunks": n, "bytes_per_chunk_over_pcie": bpc,
               "pcie_GBps": rate * bpc / 1e9, "pcie_gen5_x16_spec_GBps": 63.0,
               "note": "numpy (pageable) chunk arrays in, logits + label counts out on the host; includes the host copy into "
                       "pinned slots, H2D, kernels, D2H"}
        if device_logits is not None:
            leg["max_abs_diff_vs_device_path"] = float(np.abs(lg_h[:4096] - device_logits[:4096].cpu().numpy()).max())
        return leg

    def run(self, steps, warmup):
        """W untimed steps, then exactly K timed steps between barrier + synchronize on both sides; the count all-reduce is
        inside the timed region; elapsed = max over ranks."""
        import torch

        from remora_amd import dist as rdist

        for _ in range(warmup):
            self.step()
        torch.cuda.synchronize()
        self.counts.zero_()
        self.eng.profile_reset()
        self.eng.profile_enable(True)
        rdist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        local_counts = self.counts.clone()
        torch.cuda.synchronize()
        tc0 = time.perf_counter()
        rdist.allreduce_counts(self.counts)  # the one collective of the job
        torch.cuda.synchronize()
        self.allreduce_ms = (time.perf_counter() - tc0) * 1e3
        rdist.barrier()
        t1 = time.perf_counter()
        self.eng.profile_enable(False)
        elapsed = rdist.allreduce_max_float(t1 - t0)
        per_rank = rdist.allgather_counts(local_counts)
        return elapsed, self.eng.profile(), per_rank

    def report(self, steps, warmup, elapsed, prof, traffic_table=None):
        flops = kernel_flops_per_chunk(self.arch, self.L, self.size, sum(self.kcb) + 1, self.num_out)
        alg_b = kernel_alg_bytes_per_chunk(self.arch, self.L, self.dtype, self.size, self.num_out, self.dev[1].shape[1], self.dev[2].shape[1])
        n, total = self.n, self.total_chunks_per_step * steps
        kern = {}
        for name, (ms, launches) in prof.items():
            fl = flops.get(name)
            kern[name] = {"ms_total": ms, "launches": launches, "avg_ms": ms / launches,
                          "tflops": (fl * n * steps / (ms * 1e-3) / 1e12) if fl else None}
        # The fp32 5-tap stride-1 layers at 64 channels run as a Winograd F(4, 5) convolution (k_wino.hip): 8 products per group of
        # four outputs where the direct form has 20.  `tflops` stays the ALGORITHMIC (direct-form) rate - for these kernels it
        # may pass the MFMA peak -, `executed_tflops` is what the matrix cores execute; a roofline fraction is only ever taken of the latter.
        executed = dict(flops)
        if self.dtype == "fp32" and self.size == 64 and os.environ.get("RMR_WINOGRAD", "1") != "0":
            _, _, _, P3 = geometry(self.arch, self.L)
            for name, pout in (("conv_merge1", P3 - 4),) + ((("conv_merge2", P3 - 8),) if self.arch != "conv_lstm" else ()):
                if name in flops and pout >= 4:
                    executed[name] = flops[name] * (8 * ((pout + 3) // 4)) / (5 * pout)
                    if name in kern and kern[name]["tflops"]:
                        kern[name]["executed_tflops"] = kern[name]["tflops"] * executed[name] / flops[name]
                        kern[name]["form"] = "Winograd F(4,5): 8 MFMA products per 4 outputs and input channel (direct form: 20) + 46 VALU transform operations"
            if "sig3_front" in flops:  # sig_conv3 inside the folded kernel: stride 3 as three 3-tap phases in F(4,3) form
                executed["sig3_front"] = flops["front_sig"] + flops["conv_sig3"] * (6 * ((P3 + 3) // 4)) / (3 * P3)
                if "sig3_front" in kern and kern["sig3_front"]["tflops"]:
                    kern["sig3_front"]["executed_tflops"] = kern["sig3_front"]["tflops"] * executed["sig3_front"] / flops["sig3_front"]
                    kern["sig3_front"]["form"] = "sig_conv3 as polyphase Winograd F(4,3): 6 MFMA products per 4 outputs, phase and input channel (direct form: 12)"
            if "seq2_front" in flops:  # seq_conv2 inside the folded kernel: phases of 5, 4, 4 taps, all in F(4,5) form (8 products for 20 / 16 / 16)
                executed["seq2_front"] = flops["front_seq"] + flops["conv_seq2"] * (8 * 3 * ((P3 + 3) // 4)) / (13 * P3)
                if "seq2_front" in kern and kern["seq2_front"]["tflops"]:
                    kern["seq2_front"]["executed_tflops"] = kern["seq2_front"]["tflops"] * executed["seq2_front"] / flops["seq2_front"]
                    kern["seq2_front"]["form"] = "seq_conv2 as polyphase Winograd F(4,5): 24 MFMA products per 4 outputs and input channel (direct form: 52)"
            if self.arch != "conv_lstm" and "conv_seq3" in flops:  # Conv_w_ref's seq_conv3: stride 3 as three 3-tap phases in F(4,3) form
                executed["conv_seq3"] = flops["conv_seq3"] * (6 * ((P3 + 3) // 4)) / (3 * P3)
                if "conv_seq3" in kern and kern["conv_seq3"]["tflops"]:
                    kern["conv_seq3"]["executed_tflops"] = kern["conv_seq3"]["tflops"] * executed["conv_seq3"] / flops["conv_seq3"]
                    kern["conv_seq3"]["form"] = "polyphase Winograd F(4,3): 6 MFMA products per 4 outputs, phase and input channel (direct form: 12)"
        cand = [k for k in kern if flops.get(k) and not k.startswith("front_")]
        dom = max(cand, key=lambda k: kern[k]["ms_total"])
        cpl = n * steps / kern[dom]["launches"]
        achieved = executed[dom] * cpl / (kern[dom]["avg_ms"] * 1e-3) / 1e12
        # fp32 MFMA: 157.3 TF.  bf16 MFMA with split operands executes NPROD bf16 products per algorithmic MAC, so the
        # matrix-pipe ceiling for algorithmic flops is 2.5 PF / NPROD
        nprod = {"fp32": None, "bf16": 1, "f16": 1, "bf16x3": 3, "f16x3": 3, "bf16x6": 6}[self.dtype]
        peak = PEAK_FP32_MFMA_TFLOPS if nprod is None else PEAK_BF16_MFMA_TFLOPS / nprod
        traffic, tsrc = None, None
        ent = ((traffic_table or {}).get(f"{self.workload}:{self.dtype}") or (traffic_table or {}).get(self.dtype) or {}).get(dom)
        if ent and (self.cfg == "C100" or f"{self.workload}:{self.dtype}" in (traffic_table or {})):
            traffic = ent["bytes_per_chunk"] * cpl
            import hashlib

            dom_file = {"fused_front": "k_fused.hip", "conv_merge1": "k_conv.hip", "lstm_head": "k_lstm_x16.hip" if self.dtype in ("bf16", "f16") else "k_lstm.hip"}.get(dom)
            shas = ((traffic_table or {}).get(f"{self.workload}:{self.dtype}") or (traffic_table or {}).get(self.dtype) or {}).get("_kernel_file_sha") or {}
            try:
                now = hashlib.sha256(open(os.path.join(ROOT, "remora_amd", "csrc", dom_file), "rb").read()).hexdigest()[:16] if dom_file else None
            except OSError:
                now = None
            tsrc = {"file": "profiles/traffic.json", "profile": ent.get("source"), "commit": ent.get("commit"),
                    "kernel_file": dom_file, "kernel_file_unchanged_since_profile": (shas.get(dom_file) == now) if (dom_file and now and shas) else None,
                    "profile_chunks_per_launch": ent.get("chunks_per_launch"),
                    "note": "rocprofv3 FETCH_SIZE/WRITE_SIZE passes of this workload (MI355X_MICROARCH.md corrections), bytes per "
                            "chunk scaled to this run's chunks per launch; not re-measured in this run"}
        roofline = {
            "kernel": dom, "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
            "peak_note": ("v_mfma_f32_16x16x4_f32 dense peak" if nprod is None else
                          f"16-bit dense peak 2500 / {nprod} part product(s) per algorithmic MAC"),
            "frac": achieved / peak, "traffic": float(traffic) if traffic else None, "traffic_measured": False, "traffic_source": tsrc,
            "algorithmic_bytes": float(alg_b[dom] * cpl) if dom in alg_b else None,
            "flop_per_chunk": executed[dom], "chunks_per_launch": cpl, "avg_launch_ms": kern[dom]["avg_ms"],
        }
        if executed[dom] != flops[dom]:
            roofline["algorithmic_flop_per_chunk"] = flops[dom]
            roofline["note"] = "Winograd kernel: achieved / flop_per_chunk are the MFMA flops it executes; the direct form's are algorithmic_flop_per_chunk"
        gpu_ms = sum(k["ms_total"] for k in kern.values())
        # necessary flops of the whole network (the fused kernel's entry already contains its five layers)
        net_flops = sum(v for k, v in flops.items() if k not in ("fused_front", "sig3_front", "seq2_front"))
        return {
            "value": total / elapsed, "unit": "chunks/s", "ms_per_step": elapsed / steps * 1e3, "dtype": DTYPE_OUT.get(self.dtype, self.dtype),
            "scaling": self.w["scaling"],
            "config": {"workload": f"{self.w['desc']}, {self.dtype}", "name": self.workload, "baseline_config": self.w["baseline_config"],
                       "chunks_per_step_all_gpus": self.total_chunks_per_step, "chunks_this_rank": n, "chunk_len": self.L,
                       "kmer_context_bases": list(self.kcb), "num_out": self.num_out,
                       "sharding": f"chunks sharded over {self.world} GPU(s) ({self.w['scaling']}), 1 count all-reduce"},
            "roofline": roofline,
            "whole_pipeline": {"algorithmic_tflops": net_flops * n * steps / (gpu_ms * 1e-3) / 1e12, "flop_per_chunk": net_flops,
                               "executed_tflops": sum(v for k, v in executed.items() if k not in ("fused_front", "sig3_front", "seq2_front")) * n * steps / (gpu_ms * 1e-3) / 1e12,
                               "kernel_ms_sum": gpu_ms, "wall_ms": elapsed * 1e3},
            "kernels": kern, "label_counts": [int(x) for x in self.counts.tolist()],
        }


def side_legs(job, args, model_logits):
    """The measurements around the headline (1 GPU, rank 0, outside the timed region)."""
    import torch

    out = {}
    local, kcb, n, L, md = job.local, job.kcb, job.n, job.L, job.md
    eng, model, dev, data = job.eng, job.model, job.dev, job.data
    # ---- the same job handed over as HOST buffers (numpy, pageable): PCIe-inclusive rate of the C-ABI boundary ----
    if not args.no_reads:
        out["host_buffers_pcie_inclusive"] = job.host_buffers_leg(model_logits)
    # ---- E1 standalone (materialised one-hot): HBM-write roofline ----
    if not args.no_encode:
        from remora_amd.encoded_kmers import compute_encoded_kmer_batch

        blk = min(n, 250_000)
        eng.profile_reset()
        eng.profile_enable(True)
        for rep in range(3):
            enc = compute_encoded_kmer_batch(kcb[0], kcb[1], dev[1][:blk], dev[2][:blk], dev[3][:blk])
        torch.cuda.synchronize()
        eng.profile_enable(False)
        ms, launches = eng.profile()["encode_kmers"]
        K = sum(kcb) + 1
        bytes_per_chunk = dev[1].shape[1] + 2 * dev[2].shape[1] + 2 + 4 * 4 * K * L
        gbs = bytes_per_chunk * blk * launches / (ms * 1e-3) / 1e9
        assert float(enc[:4096].sum()) == 4096 * K * L
        out["encode_roofline"] = {"kernel": "encode_kmers", "bound": "hbm", "achieved": gbs, "peak": PEAK_HBM_GBS, "unit": "GB/s",
                                  "frac": gbs / PEAK_HBM_GBS, "bytes_per_chunk": bytes_per_chunk, "chunks_per_launch": blk,
                                  "avg_launch_ms": ms / launches, "chunks_per_s": blk * launches / (ms * 1e-3)}
        del enc
    # ---- reads/sec measured end to end from whole reads ----
    reads_leg = None
    if not args.no_reads and job.arch == "conv_lstm" and job.cfg == "C100":
        from remora_amd import synth
        from remora_amd.data_chunks import RemoraRead
        from remora_amd.inference import call_read_mods, call_reads_mods, iter_call_reads_mods

        mdr = dict(md, motifs=[("CG", 0)], mod_bases=["m"], mod_long_names=["5mC"], can_base="C", base_start_justify=False, offset=0,
                   sig_map_refiner=None)
        nreads = 2048
        rs = []
        for i in range(nreads):
            r = synth.synth_read(5000, idx=i)
            rs.append(RemoraRead(dacs=r["dacs"], shift=r["shift"], scale=r["scale"], seq_to_sig_map=r["seq_to_sig_map"],
                                 int_seq=r["int_seq"], read_id=f"syn{i}"))
        def timed_calls(mdl, calls=9):
            """Seconds of `calls` single call_reads_mods calls after four warm-ups: the pipeline's threads hold two pinned
            staging buffers each, which reach the size of the largest sub-batch only after the tapered sub-batches of a few
            calls have passed through every one of them (calls 1-4 of a process: 17-20 ms against 11-12 ms with the bf16 model)."""
            for _ in range(4):
                got = call_reads_mods(rs, mdl, mdr)
            ts = []
            for _ in range(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call_reads_mods(rs, mdl, mdr)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            return sorted(ts), got

        calls_s, res = timed_calls(model)
        nchunks = sum(r[2].size for r in res)
        ta, tb = 0.0, 3 * calls_s[len(calls_s) // 2]  # (the three-call window of earlier rounds, from the median call)
        for r in rs[:8]:  # (the first calls size the engine's staging buffer and arena)
            call_read_mods(r, model, mdr)
        single = []
        for _ in range(3):
            t1a = time.perf_counter()
            for r in rs[:128]:
                call_read_mods(r, model, mdr)
            single.append((time.perf_counter() - t1a) / 128)
        single.sort()
        stream_batches = [rs[i : i + 512] for i in range(0, nreads, 512)] * 2
        for _ in iter_call_reads_mods(stream_batches[:2], model, mdr):
            pass
        torch.cuda.synchronize()
        tsa = time.perf_counter()
        for _ in iter_call_reads_mods(stream_batches, model, mdr):
            pass
        torch.cuda.synchronize()
        tsb = time.perf_counter()
        def timed_stream(mdl, rounds=3):
            """reads/s of iter_call_reads_mods over `rounds` x 4 batches of 512 reads (the DMA of batch k + 1 under the kernels of
            batch k; results on the host per batch), after a warm-up pass; best and median of three repeats."""
            sb = [rs[i : i + 512] for i in range(0, nreads, 512)] * rounds
            for _ in iter_call_reads_mods(sb[:4], mdl, mdr):
                pass
            rates = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0s = time.perf_counter()
                for _ in iter_call_reads_mods(sb, mdl, mdr):
                    pass
                torch.cuda.synchronize()
                rates.append(512 * len(sb) / (time.perf_counter() - t0s))
            rates.sort()
            return rates[1], rates[-1]

        bf16_rate = bf16_best = None
        streamed_16 = {}
        if job.dtype == "fp32":  # the same reads through the plain-bf16 model of the same weights (3e-2 logit tolerance)
            from remora_amd.model_util import model_from_state

            mb = model_from_state(job.state, md, device=local, dtype="bf16")
            bf16_calls, _ = timed_calls(mb)
            bf16_rate = nreads / bf16_calls[len(bf16_calls) // 2]
            bf16_best = nreads / bf16_calls[0]
            streamed_16["bf16"] = timed_stream(mb)
            del mb
            mh = model_from_state(job.state, md, device=local, dtype="f16")
            streamed_16["f16"] = timed_stream(mh)
            del mh
        reads_leg = {"reads": nreads, "bases_per_read": 5000, "chunks_per_read": nchunks / nreads, "model_dtype": job.dtype,
                     "batched_reads_per_s": 3 * nreads / (tb - ta), "batched_chunks_per_s": 3 * nchunks / (tb - ta),
                     "batched_reads_per_s_best_call": nreads / calls_s[0], "batched_statistic": "median of 9 calls after 4 warm-ups",
                     "batched_reads_per_s_bf16_model": bf16_rate, "batched_reads_per_s_bf16_model_best_call": bf16_best,
                     "streamed_reads_per_s": 512 * len(stream_batches) / (tsb - tsa),
                     "streamed_reads_per_s_bf16_model": streamed_16.get("bf16", (None, None))[0],
                     "streamed_reads_per_s_bf16_model_best": streamed_16.get("bf16", (None, None))[1],
                     "streamed_reads_per_s_f16_model": streamed_16.get("f16", (None, None))[0],
                     "streamed_statistic": "iter_call_reads_mods over 12 batches of 512 reads, median (best) of 3 repeats after a warm-up pass",
                     "single_read_api_reads_per_s": 1.0 / single[1], "single_read_api_us_per_read": single[1] * 1e6,
                     "single_read_statistic": "median of 3 passes over 128 reads after 8 warm-up calls (call_read_mods -> rmr_call_read)",
                     "note": f"call_reads_mods: one upload of the reads, GPU motif scan + geometry/fill + fused inference, logits back "
                             f"on the host, per batch of {nreads} reads"}
        out["reads_pipeline"] = reads_leg
    if not args.no_refine:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_dataset
        import bench_refine
        import bench_vbz

        refine_leg = bench_refine.measure(n_reads=8192, n_bases=5000, steps=2, warmup=1, cpu_reads=4, device=local)
        if reads_leg is not None:
            from remora_amd.refine_signal_map import SigMapRefiner

            table, center, base = bench_refine.synth_reads(64, 5000, seed=5)
            refiner = SigMapRefiner(_levels_array=table, center_idx=center, do_rough_rescale=True, scale_iters=0)
            mdf = dict(mdr, sig_map_refiner=refiner)
            nref = 2048

            def fresh():
                return [RemoraRead(dacs=base[i % 64][0], shift=400.0, scale=60.0, seq_to_sig_map=base[i % 64][1].copy(),
                                   int_seq=base[i % 64][2], read_id=f"lv{i}") for i in range(nref)]

            call_reads_mods(fresh(), model, mdf)  # warm-up (also creates the device refiner)
            batches = [fresh() for _ in range(3)]  # refinement rewrites the reads: a fresh copy per timed call
            torch.cuda.synchronize()
            ta = time.perf_counter()
            for rs2 in batches:
                call_reads_mods(rs2, model, mdf)
            torch.cuda.synchronize()
            tb = time.perf_counter()
            refine_leg["reads_pipeline_with_refiner"] = {
                "reads": nref, "calls": 3, "batched_reads_per_s": 3 * nref / (tb - ta),
                "note": "call_reads_mods with a loaded SigMapRefiner (do_rough_rescale, scale_iters=0, dwell_penalty)"}
        out["refine_signal_map"] = refine_leg
        out["vbz_decode"] = bench_vbz.measure(n_rows=4096, row_samples=102400, steps=3, warmup=1, cpu_rows=8, device=local)
        out["dataset_etl"] = bench_dataset.measure(n_chunks=1 << 20, n_reads=2048, n_bases=5000, device=local)
    return out


def result_line(out):
    """The ONE stdout line: the contract's keys + compact `roofline`, `cpu_baseline`, `parity` — below LINE_LIMIT bytes.
    Everything else a run measures (kernel table, other configs, CPU-baseline forms, side legs) is in bench_details.json."""
    rf, cfg = out["roofline"], out["config"]
    line = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                "vs_baseline", "dtype", "data")}
    line["config"] = {k: cfg[k] for k in ("workload", "name", "baseline_config", "chunks_per_step_all_gpus")}
    line["roofline"] = {k: rf.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_measured",
                                               "algorithmic_bytes", "chunks_per_launch", "avg_launch_ms")}
    cb = out.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "host_cores", "kind", "headline_form", "sample")}
    pr = out.get("precision") or {}
    path = "fp32_path" if out["dtype"] == "f32" else f"{out['dtype']}_path"
    line["parity"] = {"fp32_max_abs": pr.get("fp32_path_vs_cpu_fp32_reference"), "label_counts_exact": out.get("label_counts_match_logits_argmax"),
                      "max_abs_vs_fp64": pr.get(f"{path}_vs_fp64"), "chunks_checked": pr.get("chunks")}
    if out.get("reads_per_sec") is not None:
        line["reads_per_sec"] = out["reads_per_sec"]
    wp = out.get("whole_pipeline")
    if wp:
        # the fraction of the MFMA peak the pipeline EXECUTES (Winograd layers counted at their 0.4 of the direct form's products);
        # the algorithmic (direct-form) rate beside it may pass 1
        line["whole_pipeline_frac_of_peak"] = wp.get("executed_tflops", wp["algorithmic_tflops"]) / rf["peak"]
        if wp.get("executed_tflops") and abs(wp["executed_tflops"] - wp["algorithmic_tflops"]) > 1e-9:
            line["whole_pipeline_algorithmic_frac"] = wp["algorithmic_tflops"] / rf["peak"]
    line["details"] = out.get("details_file")
    txt = json.dumps(line)
    if len(txt) >= LINE_LIMIT:  # never the case with the fields above; a guard, not a code path
        for k in ("details", "whole_pipeline_algorithmic_frac", "whole_pipeline_frac_of_peak", "reads_per_sec"):
            line.pop(k, None)
        line["cpu_baseline"].pop("sample", None)
    return line


def write_details(out, path):
    """Everything the run measured, as one JSON file beside bench.py (and in gpurun_out/ when that exists)."""
    path = path or os.path.join(ROOT, "bench_details.json")
    out["details_file"] = os.path.relpath(path, ROOT) if path.startswith(ROOT) else path
    try:
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1)
        side = os.path.join(ROOT, "gpurun_out")
        if os.path.isdir(side) and not path.startswith(side):
            with open(os.path.join(side, "bench_details.json"), "w") as fh:
                json.dump(out, fh, indent=1)
    except OSError as e:
        out["details_file"] = None
        print(f"bench_details.json not written: {e}", file=sys.stderr)


_T0 = time.time()


def dump_outputs(path, job, rank):
    """--dump-outputs DIR: what the timed path handed its caller after the last timed step, as DIR/<name>.npy -
    logits.npy (float32 [chunks, classes]: the last step's logits, every rank's chunks in rank order) and label_counts.npy
    (float64 [classes]: the per-label counts accumulated over the timed steps, all-reduced over the ranks).  Logits over
    DUMP_LIMIT are cut to a fixed, seeded sample of rows; logits_rows.npy (float64) then holds their row indices.  A collective
    (every rank calls it); rank 0 writes.  Returns {name: shape} on rank 0."""
    from remora_amd import dist as rdist

    logits = rdist.gather_arrays(job.logits.float().cpu().numpy())
    if rank != 0:
        return None
    arrays = {"label_counts": job.counts.cpu().numpy().astype(np.float64)}
    if logits.nbytes + arrays["label_counts"].nbytes > DUMP_LIMIT:
        keep = (DUMP_LIMIT - (1 << 20)) // (logits[0].nbytes + 8)
        rows = np.sort(np.random.default_rng(0).choice(logits.shape[0], keep, replace=False))
        arrays["logits_rows"] = rows.astype(np.float64)
        logits = logits[rows]
    arrays["logits"] = np.ascontiguousarray(logits, np.float32)
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, f"{name}.npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def note(msg):
    """progress breadcrumb on stderr (stdout carries exactly one line: the result)"""
    print(f"[bench {time.time() - _T0:6.1f}s] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="convlstm_c100", choices=sorted(WORKLOADS) + ["all"],
                    help="'all' = the default headline plus every other BASELINE config (implies --full)")
    ap.add_argument("--chunks", type=int, default=0, help="chunks per GPU per step (weak) / in total (strong); 0 = the workload's")
    ap.add_argument("--subbatch", type=int, default=0)
    ap.add_argument("--dtype", default=None, choices=["fp32", "bf16x6", "bf16x3", "f16x3", "bf16", "f16"],
                    help="GEMM arithmetic (default: the workload's): fp32 MFMA or bf16 MFMA with 1 / 2 / 3-part operands")
    ap.add_argument("--full", action="store_true",
                    help="1 GPU: after the headline, the side legs, the CPU baseline, the other BASELINE configs / dtypes and the "
                         "precision check; every world size: the C-ABI collective check.  Without it a run does only what its "
                         "result line needs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and the CPU parity / precision checks")
    ap.add_argument("--no-encode", action="store_true", help="--full: skip the standalone encode-kernel roofline leg")
    ap.add_argument("--no-reads", action="store_true", help="--full: skip the measured reads/sec and host-buffer legs")
    ap.add_argument("--no-alt", "--no-others", dest="no_others", action="store_true", help="--full: skip the other BASELINE configs / dtypes")
    ap.add_argument("--no-refine", action="store_true", help="--full: skip the refinement / VBZ / dataset-ETL legs")
    ap.add_argument("--cpu-budget", type=float, default=12.0)
    ap.add_argument("--details", default=None, help="where the full report goes (default: bench_details.json beside bench.py)")
    ap.add_argument("--dist-timeout", type=float, default=180.0, help="seconds a collective may take before the run is declared failed")
    ap.add_argument("--no-cabi-collective", action="store_true",
                    help="multi-rank runs with --full: skip the cross-check of the library's own RCCL communicator after the result line")
    ap.add_argument("--dist-backend", default=None, help="torch.distributed backend (default nccl = RCCL)")
    ap.add_argument("--logits-hash", action="store_true",
                    help="testing: gather every rank's logits of the last step on rank 0 (after the timed region) and record the "
                         "sha256 of their concatenation in rank order in the details file")
    ap.add_argument("--force-device", type=int, default=None, help="testing: put every rank on this GPU")
    ap.add_argument("--shard-base", type=int, default=0, help="testing: rank r of a weak run takes the data of rank shard_base + r")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path returned in its last step as DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.workload == "all":
        args.full = True
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(sys.argv[1:], args.gpus))

    # stdout carries exactly ONE line, the result of rank 0: everything else that writes to fd 1 (RCCL prints a version
    # banner there when a communicator is created, child tools, stray prints) goes to stderr
    result_fd = os.dup(1)
    os.dup2(2, 1)
    sys.stdout = os.fdopen(os.dup(2), "w")

    import torch

    from remora_amd import dist as rdist

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        os.environ.setdefault("NCCL_DEBUG", "WARN")  # RCCL's own warnings/errors on stderr: the first multi-rank run must be diagnosable
    # a rank of a multi-GPU run goes onto the socket of its GPU before the process group, its threads or any pinned buffer
    # exist (dist.bind_rank: NUMA node of the device from sysfs; a single process keeps every core it was given)
    binding = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        dev0 = args.force_device if args.force_device is not None else int(os.environ.get("LOCAL_RANK", "0"))
        # (testing, --force-device: every rank on one GPU - the plan's entry of each rank is that GPU's)
        forced_addrs = [rdist.gpu_pci_address(dev0)] * int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))) if args.force_device is not None else None
        binding = rdist.bind_rank(dev0, gpu_addrs=forced_addrs)
    ti0 = time.perf_counter()
    init_failure = None
    try:
        rank, world, local = rdist.init_process_group(args.dist_backend, set_device=args.force_device is None, timeout_s=args.dist_timeout)
        # communicators are created lazily: the first collective pays for it.  With RCCL as the backend a gloo side channel
        # exists beside it (dist.py): a first all-reduce that fails or times out on ANY rank moves every rank's collectives
        # (16 bytes of label counts, the clocks) onto gloo - the data path never crosses ranks, so the curve keeps its point
        rccl_init_ms = rdist.first_collective_ms()
    except Exception as e:  # noqa: BLE001
        init_failure = f"{type(e).__name__}: {str(e).splitlines()[0][:300] if str(e) else ''}"
        print(f"warning: rank {os.environ.get('RANK', '0')}: torch.distributed initialisation ({args.dist_backend or 'nccl'}) failed "
              f"after {time.perf_counter() - ti0:.1f} s: {init_failure}", file=sys.stderr, flush=True)
    if init_failure is not None:
        # the process group itself could not be built (every rank sees the same library and the same node, so every rank
        # is here): one retry with gloo as the only backend
        if (args.dist_backend or "nccl") == "gloo":
            sys.exit(3)
        try:
            import torch.distributed as tdist

            if tdist.is_initialized():
                tdist.destroy_process_group()
            rank, world, local = rdist.init_process_group("gloo", set_device=False, timeout_s=args.dist_timeout)
            rccl_init_ms = rdist.first_collective_ms()
            rdist.note_fallback(init_failure)
        except Exception as e:  # noqa: BLE001 - no transport at all is a failed run, said clearly
            print(f"error: rank {os.environ.get('RANK', '0')}: the gloo retry failed as well: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
            sys.exit(3)
    if world != args.gpus:
        print(f"error: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} rank(s); refusing to report a run of a "
              f"different size", file=sys.stderr)
        sys.exit(2)
    if args.force_device is not None:
        local = args.force_device
    torch.cuda.set_device(local)
    primary = "convlstm_c100" if args.workload == "all" else args.workload
    job = Job(primary, args.dtype, args.chunks, rank, world, local, args.subbatch, args.shard_base)
    if rank == 0:
        note(f"{primary} {job.dtype}: model + {job.n} chunks resident")
    try:
        elapsed, prof, per_rank = job.run(args.steps, args.warmup)
    except Exception as e:  # noqa: BLE001
        print(f"error: rank {rank}: timed region failed: {type(e).__name__}: {e}", file=sys.stderr, flush=True)
        raise
    logits_sha = None
    if args.logits_hash:
        import hashlib

        allg = rdist.gather_arrays(job.logits.cpu().numpy())
        logits_sha = hashlib.sha256(np.ascontiguousarray(allg).tobytes()).hexdigest()
    dumped = dump_outputs(args.dump_outputs, job, rank) if args.dump_outputs else None
    coll = None
    if world > 1:
        backend = rdist.transport()
        print(f"[bench rank {rank}/{world} cuda:{local}] backend {backend}: rccl_init_ms {rccl_init_ms:.1f} (process group + first "
              f"collective), allreduce_ms {job.allreduce_ms:.3f} (int64[{job.num_out}] label counts, in the timed region)",
              file=sys.stderr, flush=True)
        ms = rdist.allgather_floats([rccl_init_ms, job.allreduce_ms])
        b = binding or {}
        print(f"[bench rank {rank}/{world} cuda:{local}] pci {b.get('pci')} numa node {b.get('numa_node')} bound {b.get('bound')} "
              f"cores {len(b.get('cpus') or [])} helper threads {b.get('threads')}", file=sys.stderr, flush=True)
        placement = rdist.gather_objects({"rank": rank, "device": local, "pci": b.get("pci"), "numa_node": b.get("numa_node"),
                                          "bound": b.get("bound"), "cores": len(b.get("cpus") or []), "threads": b.get("threads"),
                                          "error": b.get("error")})
        coll = {"backend": backend, "rccl_init_ms_per_rank": [float(r[0]) for r in ms], "allreduce_ms_per_rank": [float(r[1]) for r in ms],
                "placement_per_rank": placement}
    if rank == 0:
        note(f"timed region done: {job.total_chunks_per_step * args.steps / elapsed / 1e6:.2f} M chunks/s")
    try:
        traffic_table = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    except (OSError, ValueError):
        traffic_table = {}
    # the C-ABI collective (rmr_allreduce_counts: RCCL called from the library, no torch) cross-checked against the
    # torch.distributed result on the same counts — outside the timed region.  One process: before the result line (it is
    # part of it).  Several ranks: AFTER rank 0 has printed the result line, reported on stderr — whatever a second
    # communicator does on a node this code has never seen, it cannot cost the measurement.  A check, not the headline: --full.
    cabi = rdist.cabi_allreduce_check(job.eng, per_rank, rank, world) if world == 1 and args.full else None

    def cabi_after(details_path=None):
        """Never costs the run its exit code: the measurement was taken with torch.distributed's communicator and is already
        printed; this auxiliary communicator's failure is reported on stderr and in the details file, rc stays 0."""
        if world == 1 or args.no_cabi_collective or not args.full:
            return
        tq = time.perf_counter()
        try:
            res = rdist.cabi_allreduce_check(job_eng, per_rank, rank, world, timeout_s=min(args.dist_timeout, 60.0))
        except BaseException as e:  # noqa: BLE001
            res = {"status": "error", "error": f"{type(e).__name__}: {e}"}
        res["ms"] = (time.perf_counter() - tq) * 1e3
        print(f"[bench rank {rank}/{world}] C-ABI collective (rmr_comm_init + rmr_allreduce_counts, RCCL inside the library): "
              f"{json.dumps(res)}", file=sys.stderr, flush=True)
        if details_path:
            try:
                full = json.load(open(details_path))
                full["allreduce_counts_c_abi"] = res
                with open(details_path, "w") as fh:
                    json.dump(full, fh, indent=1)
            except (OSError, ValueError):
                pass
        if res.get("status") not in ("ok", "skipped"):
            print(f"warning: rank {rank}: the library's own RCCL communicator did not reduce the label counts ({res.get('status')}); "
                  f"the result line was measured with torch.distributed's communicator and stands (exit code 0)", file=sys.stderr, flush=True)
            sys.stderr.flush()
            os._exit(0)  # a worker thread may be stuck inside a collective: leave without the interpreter's teardown

    job_eng = job.eng
    if rank != 0:
        cabi_after()
        return
    rep = job.report(args.steps, args.warmup, elapsed, prof, traffic_table)
    total = job.total_chunks_per_step * args.steps
    assert sum(rep["label_counts"]) == total, "label counts do not add up"
    assert per_rank is None or [int(x) for x in np.sum(per_rank, axis=0)] == rep["label_counts"], "per-rank counts != all-reduce"
    # the tally of the count kernel against the argmax of the logits the last step returned (this rank's chunks)
    last = np.bincount(job.logits.argmax(1).cpu().numpy(), minlength=job.num_out).astype(np.int64) * args.steps
    counts_exact = bool(per_rank is not None and np.array_equal(last, np.asarray(per_rank[0], np.int64)))
    out = {
        "metric": "chunks/sec, 5mC CG ConvLSTM_w_ref inference (fused chunk arrays -> logits + label counts)"
        if primary.startswith("convlstm") else "chunks/sec, Conv_w_ref inference (fused chunk arrays -> logits + label counts)",
        "value": rep["value"], "unit": "chunks/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": rep["ms_per_step"], "higher_is_better": True, "scaling": rep["scaling"], "vs_baseline": None,
        "dtype": rep["dtype"], "data": "synthetic", "config": rep["config"],
        "roofline": rep["roofline"], "whole_pipeline": rep["whole_pipeline"], "kernels": rep["kernels"],
        "label_counts": rep["label_counts"], "label_counts_match_logits_argmax": counts_exact,
        "label_counts_per_rank": [[int(x) for x in r] for r in per_rank] if per_rank is not None else None,
        "allreduce_counts_c_abi": ((cabi if world == 1 else "run after the result line; result on stderr (see bench.py)")
                                   if args.full else "not run (--full runs it)"),
        "collective": coll, "logits_sha256": logits_sha, "outputs_dumped": dumped,
    }
    if world == 1 and args.full:
        legs = side_legs(job, args, job.logits)
        out.update(legs)
        note("side legs done")
        rl = legs.get("reads_pipeline")
        # reads/sec: MEASURED from whole reads when that leg ran; the chunks/312 figure BASELINE.md §3.4 prescribes is kept beside it
        out["reads_per_sec_derived"] = rep["value"] / 312.0
        out["reads_per_sec"] = rl["batched_reads_per_s"] if rl else None
        out["reads_per_sec_bf16_model"] = rl.get("batched_reads_per_s_bf16_model") if rl else None
        out["reads_per_sec_note"] = ("measured: call_reads_mods on 2048 synthetic 5 kb reads per call (reads_pipeline); "
                                     "reads_per_sec_derived = chunks/s / 312 CG sites per read (BASELINE.md §3.4)")
        if not args.no_cpu_baseline:
            nb = min(job.n, 1 << 17)
            sample = {k: v[:nb] for k, v in job.data.items() if isinstance(v, np.ndarray)}
            out["cpu_baseline"] = cpu_baseline(job.state, sample, job.kcb, args.cpu_budget)
            out["gpu_over_cpu"] = rep["value"] / out["cpu_baseline"]["value"]
            note("cpu baseline done")
        # ---- the other BASELINE configs / dtypes, each with its own value + roofline (same protocol, fewer legs) ----
        others = {}
        npc = min(job.n, PRECISION_CHUNKS)
        head_logits = {f"{job.dtype}_path": job.logits[:npc].cpu().numpy()}
        primary_state, primary_sample, primary_kcb = job.state, {k: v[:npc] for k, v in job.data.items() if isinstance(v, np.ndarray)}, job.kcb
        primary_key = (primary, job.dtype)
        kept = {(primary, job.dtype): job.logits}  # whole-step logits by (workload, dtype): reduced precision vs fp32 on every chunk
        del job
        torch.cuda.empty_cache()
        if not args.no_others:
            for key, wl, dt, ch in OTHER_CONFIGS:
                if (wl, dt or WORKLOADS[wl]["dtype"]) == primary_key:
                    continue
                try:
                    j = Job(wl, dt, ch, 0, 1, local, args.subbatch)
                    el, pf, _ = j.run(min(args.steps, 5), min(args.warmup, 2))
                    r = j.report(min(args.steps, 5), min(args.warmup, 2), el, pf, traffic_table)
                    assert sum(r["label_counts"]) == j.total_chunks_per_step * min(args.steps, 5)
                    if wl == primary and j.cfg == "C100" and j.arch == "conv_lstm":
                        head_logits[f"{j.dtype}_path"] = j.logits[:npc].cpu().numpy()
                    if j.n <= BLOCK:
                        kept[(wl, j.dtype)] = j.logits
                    others[key] = {k: r[k] for k in ("value", "unit", "ms_per_step", "dtype", "scaling", "config", "roofline", "kernels")}
                    others[key]["steps"] = min(args.steps, 5)
                    if not args.no_cpu_baseline:  # the oracle is the checker here, never the thing measured
                        others[key]["parity"] = config_parity(j, kept.get((wl, "fp32")) if j.n <= BLOCK else None,
                                                              comparand_only=key == "convlstm_c200_fp32")
                    if not args.no_reads:  # what a host-fed caller gets from this configuration (PCIe-inclusive; never `value`)
                        others[key]["host_buffers_pcie_inclusive"] = j.host_buffers_leg(j.logits)
                    note(f"other config {key}: {r['value'] / 1e6:.2f} M chunks/s, {r['roofline']['kernel']} {r['roofline']['frac']:.2f} of peak")
                    del j
                    torch.cuda.empty_cache()
                except Exception as e:  # noqa: BLE001 - one config failing must not take the headline line down
                    others[key] = {"error": f"{type(e).__name__}: {e}"}
            out["other_configs"] = others
        if not args.no_cpu_baseline:
            full = {f"{wl}:{dt}": (lg, kept[(wl, "fp32")]) for (wl, dt), lg in kept.items()
                    if dt != "fp32" and (wl, "fp32") in kept and kept[(wl, "fp32")].shape == lg.shape}
            out["precision"] = precision_check(primary_state, primary_sample, primary_kcb, head_logits, full)
    write_details(out, args.details)
    os.write(result_fd, (json.dumps(result_line(out)) + "\n").encode())
    cabi_after(args.details or os.path.join(ROOT, "bench_details.json"))
    if cabi and cabi.get("status") != "ok":  # one process: in the details file (`allreduce_counts_c_abi`) and here; rc stays 0
        print(f"warning: C-ABI collective check: {cabi}", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
