#!/usr/bin/env python3
"""Time of one `Trainer.step` (forward with train-mode BatchNorm, loss, backward, AdamW) on device-resident data: the median
of STEPS steps after WARMUP warm-up steps, by HIP events, at batch 2048, chunk length 100, sizes 64 and 128.  Reported per
configuration: time per step, chunks/s, each kernel group's share from the engine profiler (rmr_profile_*, a run of its
own), the executed fp32 MFMA rate (the MFMA instructions the launches issue, counted from the shapes, 2048 FLOP each) as a
fraction of the 157.3 TF peak, and the workspace per chunk.  Comparand, same process, same batch: the training step of
remora_amd.nets.ConvLSTM under torch on the same GPU with torch.optim.AdamW (on the CPU where that step cannot run).
One JSON line per configuration.  Test infrastructure; run by hand on a GPU box.

    python tests/manual/prof_train.py [BATCH=2048] [STEPS=20] [WARMUP=5]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from remora_amd import nets  # noqa: E402
from remora_amd.train_model import Trainer  # noqa: E402

BATCH, STEPS, WARMUP = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 2048), (2, 20), (3, 5)))
L, K, NUM_OUT = 100, 9, 2
PEAK_TF = 157.3


def mfma_flop(size, n):
    """FLOP of the v_mfma_f32_16x16x4_f32 instructions one step issues (2048 each), from the launch geometry of k_train.hip:
    a product of R rows, K deep, NC wide runs ceil(R / 64) ceil(NC / 64) blocks of 4 waves x ceil(K / 16) x 16 instructions;
    a weight gradient ceil(K / 64) ceil(NC / 64) blocks per slice of 4 waves x rows / 4 x 4 instructions."""
    cdiv = lambda a, b: -(-a // b)
    gemm = lambda R, Kd, NC: cdiv(R, 64) * cdiv(NC, 64) * 4 * cdiv(Kd, 16) * 16
    wgrad = lambda R, Kd, NC: cdiv(Kd, 64) * cdiv(NC, 64) * 4 * cdiv(R, 4) * 4
    L1, L2 = L - 4, L - 8
    L3 = (L2 - 9) // 3 + 1
    T = L3 - 4
    S, EC = size, 4 * K
    # (IC, OC, KW, stride, Lin, Lout, has a data gradient, forward on the matrix cores)
    convs = [(1, 4, 5, 1, L, L1, False, False), (4, 16, 5, 1, L1, L2, True, True), (16, S, 9, 3, L2, L3, True, True),
             (EC, 16, 5, 1, L, L1, False, True), (16, S, 13, 3, L1, L3, True, True), (2 * S, S, 5, 1, L3, T, True, True)]
    ins = 0
    for IC, OC, KW, st, Lin, Lout, dgrad, fwd in convs:
        if fwd:
            ins += gemm(n * Lout, KW * IC, OC)
        ins += wgrad(n * Lout, KW * IC, OC)
        if dgrad:
            ins += gemm(n * cdiv(Lin, st), cdiv(KW, st) * OC, st * IC)
    ins += gemm(n * T, S, 4 * S) + (T - 1) * gemm(n, S, 4 * S) + gemm(n, S, 4 * S)             # lstm1 input half, its steps, lstm2
    ins += gemm(n, 4 * S, S) * (1 + (T - 1)) + gemm(n * T, 4 * S, S)                            # dz1, dh steps, dx
    ins += wgrad(n * T, S, 4 * S) + wgrad(n * (T - 1), S, 4 * S) + wgrad(n, S, 4 * S) + wgrad(n, S, NUM_OUT)
    return ins * 2048


def inputs(dev):
    g = torch.Generator().manual_seed(1)
    sigs = torch.randn(BATCH, 1, L, generator=g)
    code = torch.randint(0, 4, (BATCH, K, L), generator=g)
    enc = torch.nn.functional.one_hot(code, 4).permute(0, 1, 3, 2).reshape(BATCH, 4 * K, L).float()
    labels = torch.randint(0, NUM_OUT, (BATCH,), generator=g)
    return sigs.to(dev).contiguous(), enc.to(dev).contiguous(), labels.to(dev)


def median_step_ms(step, sync_events=True):
    for _ in range(WARMUP):
        step()
    times = []
    for _ in range(STEPS):
        if sync_events:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            step()
            t1.record()
            t1.synchronize()
            times.append(t0.elapsed_time(t1))
        else:
            w = time.perf_counter()
            step()
            times.append((time.perf_counter() - w) * 1e3)
    return float(np.median(times)), float(np.min(times))


def torch_step_ms(size, dev):
    sigs, enc, labels = inputs(dev)
    net = nets.build(size, K, NUM_OUT, seed=3).to(dev).train()
    opt = torch.optim.AdamW(net.parameters(), weight_decay=1e-4)

    def step():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(net(sigs, enc), labels)
        loss.backward()
        opt.step()
        return float(loss)  # the HIP step hands its loss to the host as well

    return median_step_ms(step, sync_events=dev.type == "cuda")


for size in (64, 128):
    tr = Trainer(size, K, NUM_OUT, L, max_batch=BATCH, seed=3, weight_decay=1e-4)
    dev = tr.engine.torch_device
    sigs, enc, labels = inputs(dev)
    med, best = median_step_ms(lambda: tr.step(sigs, enc, labels))
    tr.engine.profile_enable(True)
    tr.engine.profile_reset()
    for _ in range(3):
        tr.step(sigs, enc, labels)
    prof = tr.engine.profile()
    tr.engine.profile_enable(False)
    total = sum(ms for ms, _ in prof.values())
    res = {"config": f"batch {BATCH}, C{L}, size {size}", "hip_step_ms_median": round(med, 3), "hip_step_ms_min": round(best, 3),
           "hip_chunks_per_s": round(BATCH / med * 1e3), "workspace_bytes_per_chunk": round(tr.workspace_bytes_per_chunk),
           "mfma_tflops_executed": round(mfma_flop(size, BATCH) / med / 1e9, 2),
           "mfma_fraction_of_peak": round(mfma_flop(size, BATCH) / med / 1e9 / PEAK_TF, 4),
           "kernel_share": {k: round(ms / total, 3) for k, (ms, _) in sorted(prof.items(), key=lambda kv: -kv[1][0])},
           "kernel_launches_per_step": {k: n // 3 for k, (_, n) in prof.items()},
           "profiled_kernel_ms_per_step": round(total / 3, 3)}
    try:
        t_med, t_min = torch_step_ms(size, dev)
        res.update(torch_device="gpu", torch_step_ms_median=round(t_med, 3), torch_step_ms_min=round(t_min, 3),
                   torch_chunks_per_s=round(BATCH / t_med * 1e3))
    except Exception as e:  # noqa: BLE001 - reported, and the CPU figure given instead
        t_med, t_min = torch_step_ms(size, torch.device("cpu"))
        res.update(torch_device=f"cpu (the GPU step failed: {type(e).__name__}: {str(e)[:200]})", torch_step_ms_median=round(t_med, 3),
                   torch_step_ms_min=round(t_min, 3), torch_chunks_per_s=round(BATCH / t_med * 1e3))
    res["hip_over_torch_time"] = round(med / res["torch_step_ms_median"], 3)
    print(json.dumps(res), flush=True)
    del tr
