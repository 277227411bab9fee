#!/usr/bin/env python
"""ms per dm_trainer_step at n = 2,048 on an MI355X, next to the arithmetic bound and to a torch-CPU fp32 step of the same network.

    python tools/train_rate.py [--n 2048] [--steps 30] [--warmup 5] [--cpu-steps 2] [--out profiles/train/README.md]

GPU time: HIP events on the trainer's stream around every step (dm_trainer_profile), after warm-up steps of the same shape; a step includes its
uploads, the input check, forward, backward, the loss download and Adam.  Bound: forward, dX and dW each take the 8.924 MFLOP per window of the
inference graph: 3 x 8.924 MFLOP x n, over the 157.3 TFLOP/s fp32 MFMA peak.  CPU column: torch autograd, float32, at most 16
threads (tests/train_oracle.py's network and Adam).  A run that finds no GPU fails; nothing is estimated.
"""
import argparse
import datetime
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MFLOP_PER_WINDOW = 8.924
FP32_MFMA_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from deepmod_amd import _lib, model, synth, train
    if _lib.load().dm_device_count() < 1:
        raise SystemExit("train_rate: no gfx950 device visible")
    flat = model.flatten_weights(train.initial_weights(0))
    x = synth.synthetic_windows(a.n, seed=1)
    y = np.eye(2, dtype=np.float32)[np.random.default_rng(2).integers(0, 2, a.n)]
    tr = train.Trainer(flat, device=0, max_batch=a.n)
    for _ in range(a.warmup):
        tr.step(x, y)
    tr.profile(True)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        tr.step(x, y)
    wall_ms = (time.perf_counter() - t0) * 1e3 / a.steps
    ms, steps = tr.profile(False)
    tr.close()
    gpu_ms = ms / steps
    gflop = 3 * MFLOP_PER_WINDOW * a.n / 1e3
    bound_ms = gflop / FP32_MFMA_TFLOPS

    import torch
    import train_oracle as oracle
    torch.set_num_threads(min(16, torch.get_num_threads()))
    batches = [(x, y)] * (a.cpu_steps + 1)
    t0 = time.perf_counter()
    oracle.train_trajectory(flat, batches[:1], torch.float32)
    t1 = time.perf_counter()
    oracle.train_trajectory(flat, batches[1:], torch.float32)
    cpu_ms = (time.perf_counter() - t1) * 1e3 / a.cpu_steps

    lines = ["# `dm_trainer_step` rate (tools/train_rate.py)", "",
             "| n | GPU ms per step (HIP events, %d steps after %d warm-up) | host wall ms per step | bound ms (%.1f GFLOP at %.1f TFLOP/s fp32 MFMA) | step / bound | torch-CPU fp32 ms per step (%d threads) |"
             % (steps, a.warmup, gflop, FP32_MFMA_TFLOPS, torch.get_num_threads()),
             "|---|---|---|---|---|---|",
             "| %d | %.3f | %.3f | %.3f | %.1f | %.0f |" % (a.n, gpu_ms, wall_ms, bound_ms, gpu_ms / bound_ms, cpu_ms), "",
             "The bound is arithmetic only.  A step is about 100 small launches with two host round trips; the GEMM kernels take their operands from L2 by strided scalar loads without LDS staging and `dw_kernel` runs one wave per block, so the distance to the bound is the kernels' structure, not launch overhead alone.", "",
             "Measured %s, one run of `python tools/train_rate.py` (%s); the spread between runs was not measured." %
             (datetime.date.today().isoformat(), _lib.load().dm_version().decode()), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
