#!/usr/bin/env python
"""Steps per second of dm_cluster_trainer_step (csrc/cluster_train.hip.inc) at n = 4,096 on 10^6 resident rows, and the same step (forward with
dropout, mean squared error, backward, Adam) in torch-CPU float32 on 16 threads.  Recorded in profiles/cluster_train/README.md, not gated.

  python tools/cluster_train_rate.py [--rows 1000000] [--n 4096] [--steps 2000] [--repeats 5] [--cpu-steps 50]

The GPU figure is a host clock around `steps` calls that ends in reading their losses back (which waits for the last step): launches, the id
upload and Python between the calls included - what a training run sees.  Each repeat is timed after 100 uncounted steps; median (min .. max).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmod_amd import _lib, cluster, cluster_train  # noqa: E402


def gpu_rate(x, y, n, steps, repeats, keep_prob):
    tr = cluster_train.ClusterTrainer(cluster_train.initial_weights(0), 0, max_batch=n)
    tr.set_data(x, y)
    rng = np.random.default_rng(1)
    ids = [rng.integers(0, len(y), n).astype(np.int64) for _ in range(64)]
    times = []
    for rep in range(repeats + 1):
        count = 100 if rep == 0 else steps
        t0 = tr.get_state()[3]
        c0 = time.perf_counter()
        for s in range(count):
            tr.step(ids[s % 64], keep_prob, 0)
        tr.losses(t0 + count - 1, 1)
        if rep:
            times.append((time.perf_counter() - c0) / count)
    tr.close()
    return times


def cpu_rate(x, y, n, steps, keep_prob):
    import torch
    torch.set_num_threads(16)
    flat = cluster.flatten_cluster_weights(cluster_train.initial_weights(0))
    w = torch.tensor(flat, requires_grad=True)
    opt = torch.optim.Adam([w], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    xt, yt = torch.tensor(x), torch.tensor(y)
    g = torch.Generator().manual_seed(0)
    times = []
    for s in range(steps + 5):
        c0 = time.perf_counter()
        ids = torch.randint(0, len(y), (n,), generator=g)
        xb, yb = xt[ids], yt[ids]
        l1 = torch.relu(xb @ w[:1400].reshape(14, 100) + w[1400:1500])
        d1 = l1 / keep_prob * torch.floor(keep_prob + torch.rand(n, 100, generator=g))
        l2 = torch.relu(d1 @ w[1500:3500].reshape(100, 20) + w[3500:3520])
        d2 = l2 / keep_prob * torch.floor(keep_prob + torch.rand(n, 20, generator=g))
        out = torch.sigmoid(d2 @ w[3520:3540].reshape(20, 1) + w[3540])[:, 0]
        loss = ((out - yb) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        if s >= 5:
            times.append(time.perf_counter() - c0)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-steps", type=int, default=50)
    ap.add_argument("--keep_prob", type=float, default=0.7)
    args = ap.parse_args()
    lib = _lib.load()
    if lib.dm_device_count() < 1:
        raise SystemExit("Error: no gfx950 GPU visible (a rate is measured on the GPU or not at all)")
    rng = np.random.default_rng(0)
    x = rng.random((args.rows, 14), dtype=np.float32)
    x[:, 2] = rng.integers(0, 30, args.rows)
    y = np.round(rng.random(args.rows), 3).astype(np.float32)
    gpu = np.array(gpu_rate(x, y, args.n, args.steps, args.repeats, args.keep_prob))
    cpu = np.array(cpu_rate(x, y, args.n, args.cpu_steps, args.keep_prob))
    res = {"rows": args.rows, "n": args.n, "steps": args.steps, "repeats": args.repeats,
           "gpu_us_per_step": [round(float(v) * 1e6, 2) for v in (np.median(gpu), gpu.min(), gpu.max())],
           "gpu_steps_per_s": round(1.0 / float(np.median(gpu)), 1), "gpu_rows_per_s": round(args.n / float(np.median(gpu))),
           "cpu_ms_per_step": [round(float(v) * 1e3, 3) for v in (np.median(cpu), cpu.min(), cpu.max())],
           "cpu_steps_per_s": round(1.0 / float(np.median(cpu)), 1), "cpu_rows_per_s": round(args.n / float(np.median(cpu))),
           "library": lib.dm_version().decode()}
    print(json.dumps(res))
    print("| n | resident rows | GPU us per step: median (min .. max) of %d x %d steps | GPU steps/s | GPU rows/s | torch-CPU fp32 ms per step (16 threads): "
          "median (min .. max) of %d | CPU steps/s | CPU rows/s |" % (args.repeats, args.steps, args.cpu_steps))
    print("|---|---|---|---|---|---|---|---|")
    print("| %d | %d | %.1f (%.1f .. %.1f) | %.0f | %.3g | %.2f (%.2f .. %.2f) | %.0f | %.3g |" %
          ((args.n, args.rows) + tuple(res["gpu_us_per_step"]) + (res["gpu_steps_per_s"], res["gpu_rows_per_s"]) + tuple(res["cpu_ms_per_step"]) +
           (res["cpu_steps_per_s"], res["cpu_rows_per_s"])))


if __name__ == "__main__":
    main()
