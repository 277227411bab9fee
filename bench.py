#!/usr/bin/env python
"""bench.py — BASELINE.json metric on BASELINE.json config 2.

    python bench.py --gpus N --steps K --warmup W [--full]

A "step" is one pass of the hot path over one batch of 65,536 synthetic 7-feature x wd21 windows
that are already resident in HBM: dm_predict_windows (BiLSTM classify) + dm_summary_add (per-position
coverage / mod-count accumulate).  N > 1 (launched by torch.distributed.run, one rank per GPU; torch is only the
launcher): windows shard across ranks with no data-path collective (weak scaling: every rank runs its own K
batches); the only collective is ONE integer RCCL reduce-scatter of the per-position counters at the end (every rank is
left with the all-rank sums of its slice of the contig - the merge the streaming detect uses), inside the timed region,
through the product's C ABI (dm_comm_create once, dm_summary_reduce_scatter) - barriers and the max-over-ranks of the
elapsed time go through the same communicator.  Rank 0 prints ONE JSON line.

A plain run does only what `value` needs: set-up, warm-up, the K timed steps, --dump-outputs, the line (with the roofline of the
timed launches and the socket power sampled while they ran).  Every side measurement that takes a run of its own is behind --full:
the 1.5 s steady-state leg, the other MFMA modes, the trained-like model, host-buffer rates, both end-to-end legs (`extras`), the
CPU baselines with the parity against the oracle, and at N > 1 the host-fed rate of all ranks.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

# RCCL between the ranks of a node needs the ROCr runtime's dmabuf IPC mode on this stack (deepmod_amd/_lib.py): set before torch
# (which initialises the runtime under torch.distributed.run) is imported
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH = 65536
N_BATCHES = 16                # 16 x 65,536 = 1,048,576 windows ("10^6 windows batched 64k")
FLOP_PER_WINDOW = 8.924e6     # 11 live steps x 2 dirs x 3 layers + head
# /opt/skills/guides/MI355X_MICROARCH.md dense MFMA peaks: v_mfma_f32_16x16x4_f32 157.3 TF, 16-bit (f16/bf16) 2.5 PF
PRECISIONS = {
    "f16x3": {"peak": 2500.0, "kernel": "lstm16q::bilstm_f16q_kernel<0>", "dtype": "f16x3",
              "label": "split-f16 MFMA (hi+lo f16 operands, 3 products per fp32 product, fp32 accumulate), step-major: "
                       "the state of all three layers stays on the chip; 16x16x32 MFMAs (round 4), the left-over K slots' three products in one MFMA (round 5)",
              "peak_note": "v_mfma_f32_16x16x32_f16 dense 16-bit peak 2.5 PF; the kernel issues 25,600 MFMAs of 16x16x32 per 32 windows and direction "
                           "(K = 6 k32-steps x 3 products + ONE mixed MFMA that carries the three products of the left-over slots side by side, layer 0: "
                           "3 x 3 + 2; N = 100 exactly; the zero-state k32-steps of step 0 skipped; round 4: 28,350) = 26.2 MFLOP per "
                           "window = 2.94 matrix FLOP per algorithmic FLOP, so frac <= 0.34 by construction; back-to-back MFMAs on real operand bits "
                           "sustain 1.4-1.75 PF on this part at its 1,400 W limit (profiles/r02/README.md); the 32x32x16 form of rounds 2-3 "
                           "(3.09 issued per algorithmic; tools/experiments/f16s since round 6) measured 8-9 % slower in the same process (profiles/r05/shape_ab.txt)",
              "issued_per_algorithmic": 25600 * 16384 * 2 / 32.0 / FLOP_PER_WINDOW},
    "f16i8": {"peak": 2500.0, "kernel": "lstm16q::bilstm_f16q_kernel<1>", "dtype": "f16+i8",
              "label": "OPT-IN, REDUCED PRECISION: split-f16 MFMA with both cross terms of every product as one int8 MFMA (v_mfma_i32_16x16x64_i8 "
                       "since round 5, int32 accumulate, folded per super-tile); on 10^6 windows at weight scale 4 the worst window is ~1e-4 from the oracle "
                       "(the default kernel: 9e-6) - not a substitute for the default where the tolerance is binding",
              "peak_note": "priced against the dense 16-bit peak 2.5 PF like the default: per 32 windows and direction the kernel issues 17,800 "
                           "MFMAs of 16 cycles instead of 25,600 (the mixed k32-step keeps its three f16 products in one MFMA) = "
                           "2.04 matrix units per algorithmic unit; the 32x32x16 form of round 3 (tools/experiments/f16s) was ~5 % slower",
              "issued_per_algorithmic": 17800 * 16384 * 2 / 32.0 / FLOP_PER_WINDOW},
    "f32": {"peak": 157.3, "kernel": "lstm32::bilstm_f32_kernel", "dtype": "f32", "label": "fp32 MFMA",
            "peak_note": "v_mfma_f32_16x16x4_f32 dense fp32, 157.3 TF"},
}
CONTIG_LEN = 4_641_652        # E. coli K-12 sized contig for the synthetic summary
SETUP_LAUNCHES = 32           # untimed classifier launches during setup (GPU power-state warm-up), reported in the JSON
DUMP_POSITIONS = 1 << 20      # --dump-outputs: counters at this many contig positions, a fixed sample drawn with DUMP_SEED
DUMP_SEED = 7


def usable_cores():
    """(cores this process may actually use, why): affinity mask capped by the cgroup CPU quota - a container that
    reports 256 logical CPUs but is throttled to 16 CPU-seconds per second would otherwise oversubscribe OpenMP."""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    why = "sched_getaffinity: %d of %d logical CPUs" % (n, os.cpu_count() or n)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            q = max(1, int(float(quota) / float(period)))
            if q < n:
                n = q
                why += "; cgroup cpu.max %s/%s -> %d CPUs" % (quota, period, q)
    except Exception:
        pass
    return n, why


def _timed(fn, n_windows, budget_s):
    """Run fn() (classifies n_windows) repeatedly for ~budget_s -> (windows/s, windows, seconds)."""
    fn()                                                   # warm up threads / caches
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = int(max(1, min(256, budget_s / one)))
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = time.perf_counter() - t0
    return reps * n_windows / dt, reps * n_windows, dt


def cpu_baseline(weights, x_sample_src):
    """The CPU path next to the GPU figure: oracle/deepmod_oracle.c - a plain-C fp32 restatement of the
    TF graph (NOT TensorFlow/Eigen: TF is not installable here), OpenMP over windows - on the host cores of this box,
    bounded to ~25 s: all usable cores at the GPU batch size (`value`), the same cores fed the reference's own
    rnn_pred_batch_size = 512 windows per call (myDetect.py:30, :808-812), and one thread."""
    from oracle import oracle_np
    cores, why = usable_cores()
    oracle_np.build_c_oracle()
    run = lambda x, t: (lambda: oracle_np.predict_windows_c(weights, x, nthreads=t))
    sample = x_sample_src[:16384]
    ref_prob, ref_cls = oracle_np.predict_windows_c(weights, sample, nthreads=cores)     # kept: bench's parity field compares the GPU path with it
    big, n_big, dt_big = _timed(run(sample, cores), len(sample), 12.0)
    chunks = [sample[i:i + 512] for i in range(0, 4096, 512)]
    b512, n512, dt512 = _timed(lambda: [oracle_np.predict_windows_c(weights, c, nthreads=cores) for c in chunks], 4096, 6.0)
    one, n_one, dt_one = _timed(run(sample[:1024], 1), 1024, 6.0)
    gemm = cpu_gemm_baseline(weights, sample, cores)
    return (ref_prob, ref_cls), {"value": big, "unit": "base-positions/s", "cores": cores, "cores_why": why, "logical_cpus": os.cpu_count(), "kind": "port",
            "sample": "%d windows (passes over the first 16,384 windows of batch 0) in %.1f s, oracle/deepmod_oracle.c = fp32 C "
                      "restatement of the TF graph with libm expf/tanhf (scalar-ish loop nest, ~0.4 TFLOP/s; NOT TensorFlow/Eigen), "
                      "%d OpenMP threads" % (n_big, dt_big, cores),
            "batch512": {"value": b512, "cores": cores, "sample": "%d windows as calls of 512 (rnn_pred_batch_size, myDetect.py:30) in %.1f s" % (n512, dt512)},
            "single_thread": {"value": one, "cores": 1, "sample": "%d windows in %.1f s" % (n_one, dt_one)},
            "gemm": gemm}


def cpu_gemm_baseline(weights, sample, cores):
    """A fairer stand-in for what TensorFlow-CPU does with this graph: the same 67 MatMuls as LIBRARY sgemm calls with
    vectorised sigmoid / tanh on all usable cores - oracle/oracle_torch.py (torch-CPU addmm + intra-op threads; numpy / OpenBLAS,
    oracle/oracle_np.predict_windows_np, if torch is not importable).  Batch 512 (rnn_pred_batch_size, myDetect.py:30) and 16,384.
    Still NOT TensorFlow.  (The graph is elementwise-heavy - 33,000 transcendentals per window against K <= 200 GEMMs - so the library
    form is not the 3-6x a dense-GEMM graph would gain over the C loop nest.)"""
    out = {"kind": "port", "cores": cores}
    try:
        from oracle import oracle_torch
        g = oracle_torch.TorchGraph(weights, cores)
        fn = g.predict
        out["what"] = ("oracle/oracle_torch.py: the graph as torch-CPU library calls (addmm = library sgemm per (step, layer, direction), vectorised "
                       "sigmoid / tanh, %d intra-op threads): the GEMM-library restatement of the path, approximately what TF-CPU / Eigen would do; "
                       "NOT TensorFlow" % cores)
    except Exception as exc:
        from oracle import oracle_np
        fn = lambda x: oracle_np.predict_windows_np(weights, x)[0]
        out["what"] = "oracle/oracle_np.predict_windows_np (numpy / OpenBLAS sgemm; torch not importable: %r); NOT TensorFlow" % (exc,)
    for name, batch, budget in (("batch512", 512, 4.0), ("batch16384", 16384, 6.0)):
        x = sample[:batch]
        try:
            v, n, dt = _timed(lambda: fn(x), batch, budget)
            out[name] = {"value": v, "unit": "base-positions/s", "sample": "%d windows as calls of %d in %.1f s" % (n, batch, dt)}
        except Exception as exc:      # a leg that cannot run must not cost the line
            out[name] = {"error": repr(exc)}
    out["value"] = (out.get("batch16384") or {}).get("value")
    return out


# every file a classifier kernel is compiled from (its translation unit, what that includes, the interface header) - VERDICT r05 weak 9a: the
# default kernel also compiles the shared helpers and the unit's launch / packing code, an edit there must mark a committed profile stale too
KERNEL_SOURCES = {"f16x3": ["kern_f16q0.hip", "lstm_f16q.hip.inc", "lstm_common.hip.inc", "kernels.h"],
                  "f16i8": ["kern_f16q1.hip", "kern_f16q0.hip", "lstm_f16q.hip.inc", "lstm_common.hip.inc", "kernels.h"],
                  "f32": ["kern_f32.hip", "lstm_f32.hip.inc", "kernels.h"]}


def kernel_source_sha(precision):
    """Hash of everything the classifier kernel of `precision` is built from - its sources (KERNEL_SOURCES) and the compiler flags of
    __graft_entry__.HIPCC_FLAGS: a PMC summary is only valid for the kernel it was collected on."""
    import hashlib
    import __graft_entry__ as ge
    h = hashlib.sha256()
    for f in KERNEL_SOURCES[precision]:
        h.update(f.encode() + b"\0")
        h.update(open(os.path.join(ROOT, "deepmod_amd", "csrc", f), "rb").read())
    h.update(" ".join(ge.HIPCC_FLAGS).encode())
    return h.hexdigest()[:16]


def measured_traffic(precision):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes of this same command
    (profiles/<round>/<precision>/pmc_summary.json of the newest round that has one: FETCH_SIZE and WRITE_SIZE in KB,
    separate --pmc passes; gfx950 correction: FETCH_SIZE x 2 - calibrated in round 5 on known byte counts, tools/ubench/fetch_calib.hip:
    the counter reports exactly half the bytes both for 16-byte coalesced loads and for this kernel's own pattern, 4-byte loads of 28-byte
    feature rows; WRITE_SIZE is exact - profiles/r05/fetch_calib.txt).  The kernel's HBM traffic is ~1.7x the algorithmic bytes because
    the two directions of a window are separate work items that each fetch their 308-byte half in 128-byte lines; HBM runs at < 0.1 TB/s.
    `stale` is true when the kernel sources changed since that profile was taken."""
    rounds = sorted(d for d in os.listdir(os.path.join(ROOT, "profiles")) if d.startswith("r") and d[1:].isdigit())
    for rnd in reversed(rounds):
        path = os.path.join(ROOT, "profiles", rnd, precision, "pmc_summary.json")
        if not os.path.exists(path):
            continue
        try:
            pmc = json.load(open(path))
            fetch = pmc["FETCH_SIZE"]["mean_per_launch"] * 1024.0
            write = pmc["WRITE_SIZE"]["mean_per_launch"] * 1024.0
        except Exception:
            continue
        return {"bytes": 2.0 * fetch + write, "fetch_size_bytes_raw": fetch, "write_size_bytes": write,
                "kernel_ms_rocprof_steady": pmc.get("kernel_ms_rocprof_steady"), "kernel_trace": pmc.get("kernel_trace"),
                "source": os.path.relpath(path, ROOT), "windows_per_launch": pmc.get("windows_per_launch", BATCH),
                "profiled_kernel_src_sha": pmc.get("kernel_src_sha"), "kernel_src_sha": kernel_source_sha(precision),
                "stale": pmc.get("kernel_src_sha") != kernel_source_sha(precision)}
    return None


def power_evidence(precision):
    """Committed evidence for what bounds the default kernel (profiles/<round>/README.md section 1): socket power and clock
    sampled while the kernel runs (tools/power_trace.sh) and the matrix rate a microbenchmark with the same instruction mix
    reaches (tools/ubench/mfma32_fill.hip).  Informational: `roofline.peak` stays the guide's dense MFMA peak."""
    rounds = sorted(d for d in os.listdir(os.path.join(ROOT, "profiles")) if d.startswith("r") and d[1:].isdigit())
    for rnd in reversed(rounds):
        path = os.path.join(ROOT, "profiles", rnd, "power_%s.txt" % precision)
        if not os.path.exists(path):
            continue
        txt = open(path).read()
        import re
        pw = re.search(r"busy median ([0-9.]+)", txt)
        ck = re.search(r"sclk MHz while busy: median (\d+)", txt)
        out = {"source": os.path.relpath(path, ROOT), "socket_power_w_busy_median": float(pw.group(1)) if pw else None,
               "socket_power_cap_w": 1400.0, "sclk_mhz_busy_median": int(ck.group(1)) if ck else None, "sclk_mhz_max": 2400}
        if precision.startswith("f16x3"):
            out["note"] = ("the split-f16 kernels run at or near the package power limit with the shader clock held at ~2.0-2.2 GHz; "
                           "back-to-back f16 MFMAs on real operand bits sustain 1,400-1,650 TFLOP/s on this part (clock 1.36-1.49 GHz) "
                           "and 1,200 with a VALU / LDS filler mix like this kernel's (profiles/r02/ubench_mfma32_fill.txt)")
        return out
    return None


def dump_outputs(out_dir, prob_dev, cls_dev, counters):
    """--dump-outputs: what the timed path hands its caller after the last timed step, as float32 .npy files in out_dir - that step's
    prob [BATCH, 2] and cls [BATCH], and the touch / cov / mod counters accumulated by every step so far at DUMP_POSITIONS positions drawn
    without replacement with DUMP_SEED (sorted; all positions if there are fewer).  Counters stay exact in float32 below 2^24 steps."""
    os.makedirs(out_dir, exist_ok=True)
    n = counters[0].size
    idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, min(n, DUMP_POSITIONS), replace=False))
    arrays = {"prob": prob_dev.to_host(), "cls": cls_dev.to_host()}
    arrays.update({name: c[idx] for name, c in zip(("touch", "cov", "mod"), counters)})
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32))
    return {"dir": out_dir, "shapes": {k: list(a.shape) for k, a in arrays.items()}, "bytes": 4 * sum(a.size for a in arrays.values()),
            "note": "float32; prob / cls of the last timed step, counters after it at %d positions sampled with seed %d" % (idx.size, DUMP_SEED)}


def steady_power_leg(m, model, _lib, plog, x_dev0, prob_dev, cls_dev, seconds=1.5):
    """Socket power and shader clock of THIS box while the default kernel runs back to back for ~1.5 s (after the timed region: the
    64-step timed leg is ~0.1 s, about the firmware's own averaging time).  -> (summary of the samples from 0.3 s on, avg launch ms)"""
    m.set_option(_lib.DM_OPT_ASYNC, 1)
    m.sync()
    m.profile_reset()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(32):
            m.predict_windows(x_dev0, prob=prob_dev, cls=cls_dev)
        m.sync()
    t1 = time.perf_counter()
    ms, launches, _kw = m.profile_get()
    m.set_option(_lib.DM_OPT_ASYNC, 0)
    out = plog.summary(t0, t1, skip_s=0.3)
    out["avg_launch_ms"] = ms / max(launches, 1)
    out["launches"] = launches
    watts = (out.get("socket_power_w") or {}).get("median")
    if watts and launches:          # the path runs at the board's power limit: time per window = joules per window / what the box allows
        out["microjoules_per_window"] = 1e3 * watts * out["avg_launch_ms"] / int(x_dev0.shape[0])
    return out


def parity_field(m, x_sample, ref):
    """max |dp|, class flips away from near ties and AUC of the GPU path's p1 against the oracle's class on the windows the
    cpu_baseline leg classified with the oracle (BASELINE.json: the metric is base-positions/s + per-base AUC vs ref)."""
    ref_prob, ref_cls = ref
    prob, cls = m.predict_windows(x_sample)
    near = np.abs(ref_prob[:, 1] - 0.5) < 1e-4
    clear = ~near
    pos, neg = prob[clear & (ref_cls == 1), 1], prob[clear & (ref_cls == 0), 1]
    auc = None
    if len(pos) and len(neg):         # Mann-Whitney U with midranks
        allv = np.concatenate([pos, neg]).astype(np.float64)
        order = np.argsort(allv, kind="mergesort")
        ranks = np.empty(len(allv))
        ranks[order] = np.arange(1, len(allv) + 1)
        sv = allv[order]
        lo = np.searchsorted(sv, sv, "left")
        hi = np.searchsorted(sv, sv, "right")
        ranks[order] = 0.5 * (lo + hi + 1)
        auc = float((ranks[:len(pos)].sum() - len(pos) * (len(pos) + 1) / 2.0) / (len(pos) * len(neg)))
    return {"windows": int(len(x_sample)), "max_abs_dp": float(np.abs(prob - ref_prob).max()), "tolerance": 1e-4,
            "class_flips": int(((cls.astype(np.int64) != ref_cls) & clear).sum()), "near_ties": int(near.sum()),
            "auc_vs_oracle": auc, "class1_fraction_oracle": float(ref_cls.mean()),
            "note": "GPU path vs oracle/deepmod_oracle.c on the first 16,384 windows of batch 0 (untimed); AUC of p1 against the oracle's class away from near ties"}


def extras(m, _lib, model, precision, x_dev0, x_host0, prob_dev, cls_dev, reps=4):
    """Untimed-for-`value` side measurements on rank 0 at N = 1: the other MFMA modes on the same batch and the PCIe-inclusive rate
    when the boundary is handed pageable host buffers.  The other modes are timed LIKE THE MAIN LEG: asynchronous
    launches on the in-order queue, SETUP_LAUNCHES untimed launches of THAT mode first (the power / clock state of a mode is its own),
    then >= 64 timed launches, kernel time from HIP events."""
    out = {}
    m.set_option(_lib.DM_OPT_ASYNC, 1)
    for key, other in (("other_precision", "f32" if precision.startswith("f16") else "f16x3"),
                       ("opt_in_precision", "f16i8" if precision != "f16i8" else "f16x3")):
        m.set_precision(other)
        n_timed = 64 if other != "f32" else 32
        for _ in range(SETUP_LAUNCHES if other != "f32" else 8):
            m.predict_windows(x_dev0, prob=prob_dev, cls=cls_dev)
        m.sync()
        m.profile_reset()
        t0 = time.perf_counter()
        for _ in range(n_timed):
            m.predict_windows(x_dev0, prob=prob_dev, cls=cls_dev)
        m.sync()
        wall = time.perf_counter() - t0
        ms, launches, kw = m.profile_get()
        rate = kw / (ms * 1e-3)
        Q = PRECISIONS[other]
        out[key] = {"precision": other, "kernel": Q["kernel"], "avg_launch_ms": ms / max(launches, 1), "launches": launches,
                    "windows_per_s_kernel": rate, "windows_per_s_wall": n_timed * BATCH / wall, "achieved_tflops": rate * FLOP_PER_WINDOW / 1e12,
                    "peak_tflops": Q["peak"], "frac": rate * FLOP_PER_WINDOW / 1e12 / Q["peak"], "label": Q["label"],
                    "timing": "%d untimed + %d timed asynchronous launches of this mode back to back" % (SETUP_LAUNCHES if other != "f32" else 8, n_timed)}
    m.set_precision(precision)
    # the two MFMA shapes behind DM_PREC_F16X3 on THIS box, alternating in this process: per switch SETUP_LAUNCHES
    # untimed launches, then 64 timed ones (HIP events), four alternations; the driver's box decides which shape is the default
    if precision == "f16x3" and m.get_info(_lib.DM_INFO_HAS_F16S):      # (experiment builds only since round 6: DM_WITH_F16S=1, tools/experiments/f16s)
        try:
            ab = {16: [], 32: []}
            for rep in range(4):
                for shape in (16, 32):
                    m.set_option(_lib.DM_OPT_F16X3_SHAPE, shape)
                    for _ in range(SETUP_LAUNCHES):
                        m.predict_windows(x_dev0, prob=prob_dev, cls=cls_dev)
                    m.sync()
                    m.profile_reset()
                    for _ in range(64):
                        m.predict_windows(x_dev0, prob=prob_dev, cls=cls_dev)
                    m.sync()
                    ms, launches, _kw = m.profile_get()
                    ab[shape].append(ms / max(launches, 1))
            med = lambda v: sorted(v)[len(v) // 2]
            out["shape_ab"] = {"avg_launch_ms_16x16x32": ab[16], "avg_launch_ms_32x32x16": ab[32],
                               "median_ms_16x16x32": med(ab[16]), "median_ms_32x32x16": med(ab[32]),
                               "ratio_16_over_32": med(ab[16]) / med(ab[32]), "default_shape": 16,
                               "kernels": {"16": "lstm16q::bilstm_f16q_kernel<0>", "32": "lstm16s::bilstm_f16s_kernel<0>"},
                               "timing": "same process, same batch, alternating 16 / 32 x 4; per switch %d untimed + 64 timed asynchronous launches, HIP events" % SETUP_LAUNCHES}
        finally:
            m.set_option(_lib.DM_OPT_F16X3_SHAPE, 16)
    m.set_option(_lib.DM_OPT_ASYNC, 0)
    # a model with TRAINED weight statistics (tests/golden/trained_like_weights.npz: the reference's own .data shards are absent) loaded
    # the way the command line loads a model: precision "auto" = the load-time calibration gate decides whether the int8 cross-term mode
    # may stand in for the three-product kernel (dm_model_calibrate_i8).  Same batch, same timing as the main leg.
    try:
        z = np.load(os.path.join(ROOT, "tests", "golden", "trained_like_weights.npz"))
        wt = {k.replace("|", "/"): np.ascontiguousarray(z[k], dtype=np.float32) for k in z.files}
        t0 = time.perf_counter()
        mt = model.BiLSTMModel(wt, device=m.device, precision="auto")
        t_load = time.perf_counter() - t0
        mt.set_option(_lib.DM_OPT_PROFILE, 1)
        mt.set_option(_lib.DM_OPT_ASYNC, 1)
        for _ in range(SETUP_LAUNCHES):
            mt.predict_windows(x_dev0, prob=prob_dev, cls=cls_dev)
        mt.sync()
        mt.profile_reset()
        t0 = time.perf_counter()
        for _ in range(64):
            mt.predict_windows(x_dev0, prob=prob_dev, cls=cls_dev)
        mt.sync()
        wall = time.perf_counter() - t0
        ms, launches, kw = mt.profile_get()
        chosen = {_lib.DM_PREC_F16X3: "f16x3", _lib.DM_PREC_F16I8: "f16i8", _lib.DM_PREC_F32: "f32"}[mt.get_info(_lib.DM_INFO_PRECISION)]
        rate = kw / (ms * 1e-3)
        out["trained_like_model"] = {"weights": "tests/golden/trained_like_weights.npz (tests/golden/make_trained_like.py: the exact architecture trained on a planted "
                                                "per-5-mer signal; kernel |w| median 0.05, max 1.7)",
                                     "precision_requested": "auto", "calibration": mt.calibration, "precision_selected": chosen,
                                     "model_load_s_including_calibration": t_load, "avg_launch_ms": ms / max(launches, 1), "launches": launches,
                                     "windows_per_s_kernel": rate, "windows_per_s_wall": 64 * BATCH / wall,
                                     "frac": rate * FLOP_PER_WINDOW / 1e12 / PRECISIONS[chosen]["peak"], "weights_obj": wt, "model_obj": mt}
    except Exception as exc:
        out["trained_like_model"] = {"error": repr(exc)}
    m.predict_windows(x_host0)            # host in, host out: H2D + kernel + D2H, synchronous
    t0 = time.perf_counter()
    for _ in range(reps):
        m.predict_windows(x_host0)
    dt = time.perf_counter() - t0
    out["host_buffers"] = {"value": reps * len(x_host0) / dt, "unit": "base-positions/s",
                           "note": "dm_predict_windows on pageable host x[65536,21,7] fp32, prob+cls returned to host "
                                   "(PCIe-inclusive, 588 B in + 9 B out per window); never used as `value`"}
    return out


# ---- extras.e2e: BASELINE configs[2] at full size through the CLI ----
E2E_GENOME_LEN, E2E_COVERAGE, E2E_READS_PER_FILE, E2E_CHROM = 4_641_652, 30.0, 100, "NC_000913.3"
# sha256 of the two BED files the command writes for this input with the default kernel (deterministic: integer counters, a
# deterministic classifier - lstm16q::bilstm_f16q_kernel; the 32x32x16 kernel of rounds 2-3, DM_F16X3_SHAPE=32, gives a3c49283... / d065fd60...:
# a different summation order moves a few near-tie windows; profiles/r04/bench_f16x3.json; round 5's merged mixed k32-step and the event-length cut of
# profiles/HISTORY.md 4.1' changed both from c95a6b53... / 4775978f..., its 19-instruction cell from 595d1000... / 007c2a59..., for the same reason).  A different digest = different BED bytes.
E2E_EXPECTED_BED_SHA256 = {"+": "b2b556e53d74dc62f840cb3ab9e05347139a6bea24d7a076ed5bd17271eb9d07",
                            "-": "a5a74fb041653f7e9961f76e9e6225f8e53c0579a56f0f838c66aba09e305f30"}


def _e2e_gen(args):
    from deepmod_amd import synth_reads
    out_dir, first, n = args
    return synth_reads.write_synthetic_packed_run(out_dir, E2E_GENOME_LEN, E2E_COVERAGE, E2E_READS_PER_FILE, seed=1, chrom=E2E_CHROM,
                                                  first_file=first, n_files=n)


def e2e_leg(precision):
    """configs[2] (E. coli 4.64 Mb at 30x: 23,300 synthetic reads, 1.39e8 base-positions) from packed feature containers on disk to
    the two BED files through `bin/DeepMod.py detect` with TWO feeder processes and the command's defaults: the wall time of the whole
    command (interpreter start to exit), what it classified, and the digest of what it wrote.  Input generation is untimed."""
    import hashlib, multiprocessing, re, shutil, subprocess, tempfile
    from deepmod_amd import synth
    cores, _ = usable_cores()
    base = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 12e9 else None
    tmp = tempfile.mkdtemp(prefix="dm_bench_e2e_", dir=base)
    try:
        wrk = os.path.join(tmp, "reads")
        total_files = int(np.ceil(E2E_COVERAGE * E2E_GENOME_LEN / 6000.0 / E2E_READS_PER_FILE))
        nproc = max(1, min(32, cores))
        chunk = int(np.ceil(total_files / nproc))
        t0 = time.perf_counter()
        with multiprocessing.get_context("spawn").Pool(nproc) as pool:
            files = sum(pool.map(_e2e_gen, [(wrk, i, chunk) for i in range(0, total_files, chunk)]), [])
        t_gen = time.perf_counter() - t0
        prefix = os.path.join(tmp, "model", "mod_train_synth")
        os.makedirs(os.path.dirname(prefix))
        synth.write_synthetic_checkpoint(prefix, seed=26, scale=4.0)
        out = os.path.join(tmp, "out")
        cmd = [sys.executable, os.path.join(ROOT, "bin", "DeepMod.py"), "detect", "--wrkBase", wrk, "--modfile", prefix, "--outFolder", out,
               "--Base", "C", "--gpus", "1", "--threads", "2", "--FileID", "stream"]
        t0 = time.perf_counter()
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        wall = time.perf_counter() - t0
        if res.returncode != 0:
            return {"error": "bin/DeepMod.py detect exited %d: %s" % (res.returncode, (res.stdout[-500:] + res.stderr[-1500:]))}
        m1 = re.search(r"Streaming detect: (\d+) reads, (\d+) base-positions", res.stdout)
        m2 = re.search(r"windows run through the classifier: (\d+) of", res.stdout)
        reads, n_pos = (int(m1.group(1)), int(m1.group(2))) if m1 else (None, None)
        n_win = int(m2.group(1)) if m2 else None
        sha, lines = {}, {}
        for strand in "+-":
            path = "%s/stream/mod_pos.%s%s.C.bed" % (out, E2E_CHROM, strand)
            h = hashlib.sha256()
            nl = 0
            with open(path, "rb") as fh:
                for blk in iter(lambda: fh.read(1 << 24), b""):
                    h.update(blk)
                    nl += blk.count(b"\n")
            sha[strand], lines[strand] = h.hexdigest(), nl
        expected = E2E_EXPECTED_BED_SHA256 if precision == "f16x3" else {"+": None, "-": None}
        return {"config": "configs[2]: E. coli 4.64 Mb at 30x, packed feature containers -> bin/DeepMod.py detect --threads 2 (two feeder processes, "
                          "streaming mode, default options) -> 2 BED files, 1 GPU", "input_files": len(files), "input_generation_s_untimed": t_gen,
                "wall_s": wall, "reads": reads, "base_positions": n_pos, "windows_classified": n_win,
                "base_positions_per_s": n_pos / wall if n_pos else None, "windows_per_s": n_win / wall if n_win else None,
                "units_note": "base_positions counts every aligned base of the run; the streaming command classifies only the windows centred "
                              "on the base of interest (no other class can reach the BED, myDetect.py:1091) - windows_per_s is the rate in the "
                              "unit of `value`, over the WHOLE command (process start-up, model load, BED writing included)",
                "bed_lines": lines, "bed_sha256": sha, "bed_sha256_expected": expected,
                "bed_matches_expected": (all(sha[k] == expected[k] for k in "+-") if all(expected.values()) else None),
                "stdout_tail": res.stdout.strip().splitlines()[-5:-1]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


E2E_RAW_READS, E2E_RAW_REPEAT, E2E_RAW_GENOME = 4000, 20, 500000


def _e2e_raw_gen(args):
    from deepmod_amd import synth_reads
    out, part, n = args
    return synth_reads.write_synthetic_raw_run(out, n_reads=n, reads_per_file=10, genome_len=E2E_RAW_GENOME, seed=3, chrom="chrS", part=part, min_len=2000, max_len=8000)[0]


def e2e_raw_leg(precision):
    """The path real data takes, from RAW signal containers (int16 DAC samples + the basecaller's event tables + alignment records) to the two BED files
    through `bin/DeepMod.py detect` with FOUR feeder processes and the command's defaults: signal normalisation and per-event statistics on the GPU (resident
    there since round 6), CIGAR walk and window association in the feeders, feature rows assembled on the device, classifier, summary.  4,000 synthetic reads
    are generated (untimed) and the work folder holds them 20 x by symbolic links - 80,000 reads, ~4e8 base-positions - so that the command runs for seconds,
    not for its start-up.  Reported: the whole command, its detect step, the steady state between the first batch and the drained device."""
    import multiprocessing, re, shutil, subprocess, tempfile
    from deepmod_amd import synth
    cores, _ = usable_cores()
    tmp = tempfile.mkdtemp(prefix="dm_bench_raw_")          # (on disk, read back through the page cache - like tools/raw_profile.py and like a real run's containers)
    try:
        src = os.path.join(tmp, "src")
        nproc = max(1, min(32, cores))
        per = -(-E2E_RAW_READS // nproc)
        t0 = time.perf_counter()
        with multiprocessing.get_context("spawn").Pool(nproc) as pool:
            files = sum(pool.map(_e2e_raw_gen, [(src, pt, per) for pt in range(nproc)]), [])
        t_gen = time.perf_counter() - t0
        wrk = os.path.join(tmp, "in")
        os.makedirs(wrk)
        os.symlink(os.path.join(src, "genome.fa"), os.path.join(wrk, "genome.fa"))
        for k in range(E2E_RAW_REPEAT):
            for f in files:
                stem = f[:-len(".dmraw.npz")]
                os.symlink(f, os.path.join(wrk, "c%02d_%s" % (k, os.path.basename(f))))
                os.symlink(stem + ".sam", os.path.join(wrk, "c%02d_%s.sam" % (k, os.path.basename(stem))))
        prefix = os.path.join(tmp, "model", "mod_train_synth")
        os.makedirs(os.path.dirname(prefix))
        synth.write_synthetic_checkpoint(prefix, seed=26, scale=4.0)
        cmd = [sys.executable, os.path.join(ROOT, "bin", "DeepMod.py"), "detect", "--wrkBase", wrk, "--Ref", os.path.join(wrk, "genome.fa"), "--modfile", prefix,
               "--outFolder", os.path.join(tmp, "out"), "--Base", "C", "--gpus", "1", "--threads", "4", "--FileID", "raw", "--alignStr", "minimap2"]
        t0 = time.perf_counter()
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if res.returncode != 0:
            return {"error": "bin/DeepMod.py detect exited %d: %s" % (res.returncode, (res.stdout[-500:] + res.stderr[-1500:]))}
        so = res.stdout
        m1 = re.search(r"Streaming detect: (\d+) reads, (\d+) base-positions .* in ([0-9.]+) s", so)
        m2 = re.search(r"windows run through the classifier: (\d+) of", so)
        m3 = re.search(r"first batch from a feeder ([0-9.]+), last batch ([0-9.]+), device drained ([0-9.]+)", so)
        m4 = re.search(r"detect wall ([0-9.]+) s, waiting for feeders ([0-9.]+) s", so)
        m5 = re.search(r"event statistics resident on the device for (\d+) of (\d+) rows", so)
        m6 = re.search(r"waiting for the device ([0-9.]+) s", so)
        reads, n_pos, t_detect = (int(m1.group(1)), int(m1.group(2)), float(m1.group(3))) if m1 else (None, None, None)
        steady = n_pos / max(float(m3.group(3)) - float(m3.group(1)), 1e-9) if (m1 and m3) else None
        return {"config": "synthetic raw containers (%d reads x %d by symbolic links, %d-base genome) -> bin/DeepMod.py detect --threads 4 (four feeder processes, "
                          "streaming mode, default options: event statistics resident on the device) -> 2 BED files, 1 GPU" % (E2E_RAW_READS, E2E_RAW_REPEAT, E2E_RAW_GENOME),
                "input_files": len(files) * E2E_RAW_REPEAT, "input_generation_s_untimed": t_gen, "wall_s": wall, "reads": reads, "base_positions": n_pos,
                "windows_classified": int(m2.group(1)) if m2 else None, "detect_step_s": t_detect,
                "base_positions_per_s_whole_command": n_pos / wall if n_pos else None, "base_positions_per_s_detect_step": n_pos / t_detect if n_pos else None,
                "base_positions_per_s_steady_state": steady, "detect_wall_s": float(m4.group(1)) if m4 else None,
                "waiting_for_feeders_s": float(m4.group(2)) if m4 else None, "waiting_for_device_s": float(m6.group(1)) if m6 else None,
                "rows_with_statistics_resident_on_the_device": [int(m5.group(1)), int(m5.group(2))] if m5 else None,
                "units_note": "base_positions counts every aligned base of the run (the streaming command classifies the ~quarter of them whose window is centred on the base of "
                              "interest); steady state = base_positions / (device drained - first batch), i.e. without process start-up, model load and BED writing",
                "stdout_tail": so.strip().splitlines()[-6:-1]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


class _stdout_to_stderr:
    """While RCCL is being set up, file descriptor 1 points at stderr: the library prints its version banner through C stdio on the first communicator of a
    process (NCCL_DEBUG=VERSION is set on these boxes), and the contract of this script is ONE JSON line on stdout."""

    def __enter__(self):
        import ctypes
        self._libc = ctypes.CDLL(None)
        sys.stdout.flush()
        self._libc.fflush(None)
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        self._libc.fflush(None)
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


class _FileControl:
    """Barrier / max over the ranks through the rendezvous files: the control plane of a run whose RCCL set-up failed."""

    def __init__(self, rdv):
        self.rdv, self.round = rdv, 0

    def max(self, value: float) -> float:
        self.round += 1
        return max(self.rdv.all_gather_json("control_%d" % self.round, value))

    def barrier(self):
        self.max(0.0)


def _agree(rdv, name, communicator, error):
    """All ranks keep the communicator, or none does: (communicator, None) or (None, every rank's error)."""
    errors = [e for e in rdv.all_gather_json(name, error) if e]
    if not errors:
        return communicator, None
    if communicator is not None:
        try:
            communicator.close()
        except Exception:
            pass
    return None, "; ".join(errors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--full", action="store_true",
                    help="after the line's own measurement, every side measurement as well (several minutes): the steady-state power leg, extras, "
                         "cpu_baseline and parity; at N > 1 the host-fed rate of all ranks")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline and parity")
    ap.add_argument("--precision", choices=sorted(PRECISIONS) + ["auto"], default="f16x3",
                    help="MFMA mode of the classifier kernel (f16x3 and f32 meet the 1e-4 probability tolerance; f16i8 is the reduced-precision mode; "
                         "auto = what the command line does: f16x3 unless the model's own calibration run lets f16i8 in)")
    ap.add_argument("--weights", choices=["synthetic", "trained-like"], default="synthetic",
                    help="synthetic: U(-a, a) kernels at scale 4 (seed 26; the workload of every round); trained-like: tests/golden/trained_like_weights.npz")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the untimed side measurements (other precision, host-buffer rate, e2e)")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip extras.e2e (configs[2] through bin/DeepMod.py detect: ~6 GB of synthetic input in /dev/shm or /tmp)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed to DIR/<name>.npy (float32, ~13 MB): "
                                                          "prob, cls and a fixed sample of the touch / cov / mod counters")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))

    torch = None
    dist_mode = world > 1 or os.environ.get("DM_BENCH_FORCE_DIST") == "1"   # 1-rank dry run of the N > 1 path
    if dist_mode:
        import torch  # loaded first so that ONE HIP / RCCL runtime serves the process (the library dlopens librccl by soname); used for cuda.synchronize only

    from deepmod_amd import _lib, comm as dmcomm, model, summary, synth

    lib = _lib.load()
    if lib.dm_device_count() < 1:
        raise SystemExit("bench.py: no gfx950 device visible; there is no CPU fallback")
    device = local_rank if dist_mode else 0
    if os.environ.get("DM_BENCH_ONE_DEVICE") == "1":      # test hook: every rank on device 0 (two real processes on a one-GPU box; RCCL refuses
        device = 0                                        # duplicate devices, so this exercises the rendezvous and the no-RCCL control plane)

    communicator = rdv = control = comm_error = None
    if dist_mode:
        # torch.distributed.run is only the launcher: ranks find each other through a file rendezvous keyed by the
        # launcher's pid (the common parent of all ranks) and the master port, and talk RCCL through the product's C ABI
        rdv = dmcomm.FileRendezvous(os.path.join("/tmp", "deepmod_bench_rdv_%d_%s" % (os.getppid(), os.environ.get("MASTER_PORT", "0"))),
                                    rank, world, timeout=300.0, fresh_after=time.time() - 600.0)
        # RCCL could never be exercised on more than one rank while this was written (no multi-GPU box was reachable): a failure to
        # set it up must not cost the run its throughput line - the data path has no collective.  The ranks agree on the outcome;
        # without RCCL the final merge is skipped, barriers / the max go through the rendezvous files, and the JSON line says so
        try:
            if os.environ.get("DM_BENCH_BREAK_RCCL") == "1":      # test hook: the degraded mode below, without a broken RCCL
                raise RuntimeError("DM_BENCH_BREAK_RCCL=1")
            with _stdout_to_stderr():
                uid = dmcomm.rccl_unique_id() if rank == 0 else None
        except Exception as exc:
            uid, comm_error = b"", "dm_rccl_unique_id: %r" % (exc,)
        uid = rdv.broadcast("rccl_id", uid)
        if uid:
            try:
                with _stdout_to_stderr():
                    communicator = dmcomm.Communicator(device, uid, rank, world)
            except Exception as exc:
                comm_error = "dm_comm_create on rank %d: %r" % (rank, exc)
        elif comm_error is None:
            comm_error = "rank 0 could not create the RCCL id"
        communicator, comm_error = _agree(rdv, "comm_up", communicator, comm_error)
        control = communicator if communicator is not None else _FileControl(rdv)

    if args.weights == "trained-like":
        z = np.load(os.path.join(ROOT, "tests", "golden", "trained_like_weights.npz"))
        weights = {k.replace("|", "/"): np.ascontiguousarray(z[k], dtype=np.float32) for k in z.files}
    else:
        weights = synth.synthetic_weights(seed=26, scale=4.0)     # ~50 % of the windows are class 1: both summary branches are taken
    m = model.BiLSTMModel(weights, device=device, precision=args.precision)
    calibration = m.calibration
    if args.precision == "auto":          # the line is labelled with the mode the gate chose
        args.precision = {_lib.DM_PREC_F16X3: "f16x3", _lib.DM_PREC_F16I8: "f16i8", _lib.DM_PREC_F32: "f32"}[m.get_info(_lib.DM_INFO_PRECISION)]
    m.set_option(_lib.DM_OPT_PROFILE, 1)
    P = PRECISIONS[args.precision]

    # synthetic windows, distinct per rank and per batch, resident in HBM before the timed region
    n_batches = min(N_BATCHES, max(1, args.steps))
    rng = np.random.default_rng(1234 + rank)
    x_dev, pos_dev, flag_dev = [], [], []
    x0 = None
    for b in range(n_batches):
        xb = synth.synthetic_windows(BATCH, seed=20260928 + 1000 * rank + b)
        if b == 0:
            x0 = xb
        x_dev.append(model.DeviceArray.from_host(xb, device))
        # one aligned base per window: consecutive reference positions of ~8 kb reads, C in ~25 % of rows
        start = rng.integers(0, CONTIG_LEN - BATCH)
        pos_dev.append(model.DeviceArray.from_host((start + np.arange(BATCH)).astype(np.int64), device))
        base_is_c = rng.random(BATCH) < 0.25
        not_gap = rng.random(BATCH) < 0.97
        flag_dev.append((base_is_c.astype(np.uint8) | (not_gap.astype(np.uint8) << 1)))
    prob_dev = model.DeviceArray((BATCH, 2), np.float32, device)
    cls_dev = model.DeviceArray((BATCH,), np.uint8, device)
    flag_dev = [model.DeviceArray.from_host(f, device) for f in flag_dev]
    summ = summary.PositionSummary(CONTIG_LEN, device=device)
    # one in-order device queue: classify -> accumulate -> classify ...; the host only waits at the end of the timed region
    m.set_option(_lib.DM_OPT_ASYNC, 1)
    summ.follow(m)

    def step(i):
        b = i % n_batches
        m.predict_windows(x_dev[b], prob=prob_dev, cls=cls_dev)
        summ.add_classified(pos_dev[b], flag_dev[b], cls_dev, BATCH)

    def sync_all():
        m.sync()
        summ.sync()
        if torch is not None:
            torch.cuda.synchronize()

    try:  # contract: bracket the timed region with torch.cuda.synchronize() as well (torch does nothing else here)
        import torch as _t
        if _t.cuda.is_available():
            _t.cuda.set_device(device)
            torch = _t
    except Exception:
        torch = None

    # setup, untimed like the data upload above: bring the GPU out of its idle power state (the first ~10 launches of a
    # process run ~15 % slower than the steady state, profiles/r01/README.md) so that a short --steps run measures the
    # same clocks as a long one; then the W warmup steps the caller asked for
    for i in range(SETUP_LAUNCHES):
        m.predict_windows(x_dev[i % n_batches], prob=prob_dev, cls=cls_dev)
    sync_all()
    for i in range(args.warmup):
        step(i)
    if communicator is not None:
        # untimed, part of the warm-up: the first reduce of this size makes RCCL set up its channels and buffers
        try:
            warm = summary.PositionSummary(CONTIG_LEN, device=device)
            warm.follow(m)
            warm.reduce_scatter(communicator)
            warm.sync()
            warm.close()
        except Exception as exc:
            comm_error = "first ncclReduceScatter on rank %d: %r" % (rank, exc)
        communicator, comm_error = _agree(rdv, "comm_warm", communicator, comm_error)
        control = communicator if communicator is not None else _FileControl(rdv)
    sync_all()
    m.profile_reset()
    # socket power / shader clock of THIS box (sysfs hwmon of the device, ~1 kHz, a thread of this process): rank 0 only
    plog = None
    if rank == 0:
        try:
            from deepmod_amd import powerlog
            plog = powerlog.PowerLog(_lib.pci_bus_id(device)).start()
        except Exception:
            plog = None
    if control is not None:
        control.barrier()
    sync_all()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(args.warmup + i)
    if communicator is not None:
        summ.reduce_scatter(communicator)     # the only collective: int32 touch|cov|mod summed over the ranks, one slice per rank (ncclReduceScatter)
    sync_all()
    if control is not None:
        control.barrier()
    t_end = time.perf_counter()
    elapsed_rank = t_end - t0
    elapsed = control.max(elapsed_rank) if control is not None else elapsed_rank
    power_timed = plog.summary(t0, t_end) if plog is not None else None
    dumped = None
    if args.dump_outputs and rank == 0:     # untimed, before the legs below reuse prob_dev / cls_dev; N > 1 with RCCL: this rank's merged slice
        dumped = dump_outputs(args.dump_outputs, prob_dev, cls_dev, summ.fetch_slice() if communicator is not None else summ.fetch())
    per_rank = None
    if control is not None and communicator is None:        # no RCCL: every rank reports the totals of its own counters
        per_rank = rdv.all_gather_json("rate", {"rank": rank, "windows_per_s": BATCH * args.steps / elapsed_rank, "elapsed_s": elapsed_rank,
                                                "device": device, "slice_sums": [int(a.sum()) for a in summ.fetch()]})
    if communicator is not None:
        sl = summ.fetch_slice()               # this rank's slice of the merged counters
        per_rank = rdv.all_gather_json("rate", {"rank": rank, "windows_per_s": BATCH * args.steps / elapsed_rank,
                                                "elapsed_s": elapsed_rank, "device": device, "slice_first": summ._slice[0],
                                                "slice_count": summ._slice[1], "slice_sums": [int(a.sum()) for a in sl]})

    kernel_ms, launches, kwindows = m.profile_get()
    total_windows = BATCH * args.steps * world
    value = total_windows / elapsed
    # N > 1, after the timed region: what `value` cannot show - the ranks feeding their GPUs from HOST memory at the same time (pageable
    # x[65536,21,7] in, prob + cls out, synchronous: 588 B in + 9 B out per window over PCIe, all ranks at once; never `value`).  A curve
    # that bends here and not in `value` is the host side of the node (PCIe / memory bandwidth), not the GPUs.  --full only
    host_fed = None
    if control is not None and args.full:
        err = None                                    # (every rank reaches every barrier / max below whatever its own calls do)
        try:
            m.set_option(_lib.DM_OPT_ASYNC, 0)
            m.predict_windows(x0)
        except Exception as exc:
            err = repr(exc)
        control.barrier()
        t0 = time.perf_counter()
        try:
            for _ in range(3):
                m.predict_windows(x0)
        except Exception as exc:
            err = repr(exc)
        dt = time.perf_counter() - t0
        slowest = control.max(dt)
        host_fed = {"value": world * 3 * BATCH / slowest, "unit": "base-positions/s", "this_rank_windows_per_s": 3 * BATCH / dt, "error_on_this_rank": err,
                    "note": "all ranks at once, dm_predict_windows on pageable host buffers (PCIe-inclusive), 3 calls of 65,536 windows per rank after the timed region; never `value`"}
    if rank == 0:
        avg_launch_s = kernel_ms * 1e-3 / max(launches, 1)
        achieved = (kwindows / max(launches, 1)) * FLOP_PER_WINDOW / avg_launch_s / 1e12
        if per_rank is None:
            check = [int(a.sum()) for a in summ.fetch()]
        else:                                 # the slices of all ranks together are the merged counters (no RCCL: the ranks' own totals)
            check = [sum(r["slice_sums"][k] for r in per_rank) for k in range(3)]
        traffic = measured_traffic(args.precision)
        out = {
            "metric": "base-positions/sec (whole node), E. coli 5mC wd21/f7 BiLSTM",
            "value": value, "unit": "base-positions/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed * 1e3 / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": P["dtype"], "data": "synthetic",
            "config": {"workload": "configs[1]: rnn_conmodC_P100wd21_f7ne1u0_4 geometry (3x100 BiLSTM, wd21, f7), "
                                   "synthetic weights (real .data shards absent), %d windows/step resident in HBM, "
                                   "%d distinct batches (1,048,576 windows)" % (BATCH, n_batches),
                       "batch": BATCH, "windows_total": total_windows, "parallelism": "window-sharded x%d" % world, "forced_dist_dry_run": bool(dist_mode and world == 1), "all_ranks_on_device_0_test_hook": os.environ.get("DM_BENCH_ONE_DEVICE") == "1", "setup_launches": SETUP_LAUNCHES,
                       "precision": P["label"], "weights": args.weights, "calibration_gate": calibration,
                       "full": args.full},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": P["peak"], "unit": "TFLOP/s",
                         "frac": achieved / P["peak"], "traffic": (traffic or {}).get("bytes"),
                         "traffic_detail": traffic, "algorithmic_bytes": 596 * BATCH,
                         "kernel": P["kernel"], "avg_launch_ms": avg_launch_s * 1e3,
                         "kernel_ms_rocprof_steady": (traffic or {}).get("kernel_ms_rocprof_steady"),      # the same launches under rocprofv3, set-up launches dropped (committed profile, another box)
                         "launches": launches, "flop_per_window": FLOP_PER_WINDOW,
                         "peak_note": P["peak_note"],
                         "matrix_pipe_busy_est": achieved * P.get("issued_per_algorithmic", 1.0) / P["peak"],
                         "issued_tflops": achieved * P.get("issued_per_algorithmic", 1.0),
                         "power": {"timed_region": power_timed, "committed_profile_of_another_box": power_evidence(args.precision),
                                   "note": "timed_region / steady: sampled on THIS box by this process (sysfs hwmon power1_input = PPT, freq1_input = sclk); "
                                           "steady = the same kernel back to back for 1.5 s after the timed region (the timed leg is ~0.1 s)"}},
            "summary_check": {"touch": check[0], "cov": check[1], "mod": check[2],
                              "note": "counter totals after the merge (N > 1: the ranks' slices of the reduce-scatter added up)"},
        }
        if dumped is not None:
            out["dump_outputs"] = dumped
        if communicator is not None:
            out["multi_gpu"] = dict(communicator.stats(), collective="ncclReduceScatter(int32 sum) x 3 counter arrays via dm_summary_reduce_scatter "
                                    "on one persistent dm_comm: rank r is left with the merged counters of positions [r, r + 1) * ceil(L / N)",
                                    reduce_bytes_per_rank=12 * CONTIG_LEN, per_rank=per_rank,
                                    measured_on_hardware_with_more_than_one_rank=bool(world > 1 and os.environ.get("DM_BENCH_ONE_DEVICE") != "1" and not os.environ.get("DEEPMOD_RCCL_LIBRARY")),
                                    collective_library="%s (ncclGetVersion %d)" % dmcomm.rccl_info(), rccl_error=None, host_fed_all_ranks=host_fed,
                                    note="`collectives` / `bytes` count one untimed warm-up merge of the same size and the timed one")
        elif control is not None:
            out["multi_gpu"] = {"collective": "NOT RUN: RCCL could not be set up, the final merge of the counters was skipped (barriers and the "
                                              "max over ranks went through the rendezvous files); the data path has no collective, so `value` stands",
                                "rccl_error": comm_error, "per_rank": per_rank, "host_fed_all_ranks": host_fed, "measured_on_hardware_with_more_than_one_rank": bool(world > 1 and os.environ.get("DM_BENCH_ONE_DEVICE") != "1")}
        if args.full and world == 1 and plog is not None and plog.available:
            try:
                st = out["roofline"]["power"]["steady"] = steady_power_leg(m, model, _lib, plog, x_dev[0], prob_dev, cls_dev)
                # the K timed steps are ~30 ms, shorter than the firmware's power averaging: the same launches in the steady state of the box, beside it
                ach = BATCH * FLOP_PER_WINDOW / (st["avg_launch_ms"] * 1e-3) / 1e12
                out["roofline"]["steady"] = {"avg_launch_ms": st["avg_launch_ms"], "launches": st["launches"], "achieved": ach, "frac": ach / P["peak"],
                                             "windows_per_s_kernel": BATCH / (st["avg_launch_ms"] * 1e-3),
                                             "note": "the same kernel on the same batch back to back for 1.5 s after the timed region (HIP events per launch): `frac` "
                                                     "above is the contract's K timed steps, this is the box's steady state - both are measured, neither is `value`"}
            except Exception as exc:
                out["roofline"]["power"]["steady"] = {"error": repr(exc)}
        if plog is not None:
            plog.stop()
        if args.full and world == 1 and not args.no_extras:
            out["extras"] = extras(m, _lib, model, args.precision, x_dev[0], x0, prob_dev, cls_dev)
            if not args.no_e2e and args.precision == "f16x3":
                try:
                    out["extras"]["e2e"] = e2e_leg(args.precision)
                except Exception as exc:
                    out["extras"]["e2e"] = {"error": repr(exc)}
                try:
                    out["extras"]["e2e_raw"] = e2e_raw_leg(args.precision)
                except Exception as exc:
                    out["extras"]["e2e_raw"] = {"error": repr(exc)}
        tl = (out.get("extras") or {}).get("trained_like_model") or {}
        wt, mt = tl.pop("weights_obj", None), tl.pop("model_obj", None)
        if args.full and world == 1 and not args.no_cpu_baseline:
            ref, out["cpu_baseline"] = cpu_baseline(weights, x0)
            m.set_option(_lib.DM_OPT_ASYNC, 0)
            out["parity"] = parity_field(m, x0[:16384], ref)
            if mt is not None:            # the gate-selected mode of the trained-like model against the oracle on the same windows
                from oracle import oracle_np
                mt.set_option(_lib.DM_OPT_ASYNC, 0)
                tl["parity"] = parity_field(mt, x0[:16384], oracle_np.predict_windows_c(wt, x0[:16384]))
        if mt is not None:
            mt.close()
        try:      # RCCL prints its version banner through C stdio: push it out first so that the JSON line is the last line
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)

    if control is not None:
        control.barrier()
    if communicator is not None:
        communicator.close()


if __name__ == "__main__":
    main()
