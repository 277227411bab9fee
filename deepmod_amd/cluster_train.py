"""`DeepMod.py traincluster`: fit the CpG-cluster model (the second stage of the 5mC workflow, cluster.py) on the GPU from a DeepMod BED and
bisulfite truth, over dm_cluster_trainer_* of the C ABI (csrc/cluster_train.hip.inc).

  DeepMod.py traincluster --predFile <prefix> --motifFolder <dir> --truth <bedMethyl[,bedMethyl]> [--chr chr1[,chr2]] [--heldout chrN[,..]]
                          [--cov 5] [--keep_prob 0.7] [--epochs 1] [--batchsize 4096] [--seed 0] --outFolder <dir> --FileID <id>

The reference ships no training script for this model.  What it pins, and what is followed here:
  * the serialized training graph train_deepmod/na12878_cluster_train_mod-keep_prob0.7-nb25-chr1/Cg.cov5.nb25.meta: X [n,14], Y [n], keep_prob;
    layer_1 = relu(X W_1 + b_1); TF1 dropout layer_1 / keep_prob * floor(keep_prob + U[0,1)); layer_2 = relu(. W_2 + b_2), the same dropout;
    output = sigmoid(. W_O + b_O); loss = mean((output - Y)^2); Adam(0.001, 0.9, 0.999, 1e-8); initial values truncated_normal(0, 1) for the three
    kernels and zeros for the biases;
  * DeepMod_tools/hm_cluster_predict.py:18-41, the truth reader the prediction tool still carries (read_truth), :16 batch_size = 4096;
  * the directory name and docs/Description of well-trained models.md: keep_prob 0.7, +-25 bp, trained on chr1.
The 14 features are cluster.cluster_features'.

THE PROJECT'S OWN (the reference does not state them, and TensorFlow's random stream could not be reproduced anyway): the order of the rows (epoch e
visits np.random.default_rng([seed, e]).permutation(N) in consecutive slices of --batchsize, the last shorter slice kept), the number of epochs
(default 1), the dropout random stream (dropout_keep below, keyed by --seed and the step count) and the draw of the initial values
(np.random.default_rng(seed), values beyond 2 standard deviations redrawn).  A run here and a run of the reference's lost script start from different
draws of the same distributions.

After every epoch: the training MSE from the step losses, with --heldout the MSE and Pearson r of those contigs at keep_prob 1 (ClusterModel on the
current weights), and a TF bundle <outFolder>/Cg.cov<cov>.nb25-<epoch> with the six variables, their twelve Adam slots and beta1_power / beta2_power
(train.checkpoint_tensors' convention) under the reference's names, plus the `checkpoint` state file; no .meta.  <outFolder>/<FileID>_cluster_train.json
holds the inputs, the site counts and the per-epoch numbers.  The bundles load through ClusterModel.from_checkpoint: `detect --clusterCpG <prefix>` and
DeepMod_tools/hm_cluster_predict.py take them as they are.  No torch, no CPU path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib, cluster, tfbundle
from .train import BETA1, BETA2, write_json

COV_THRD = 5          # hm_cluster_predict.py:18
KEEP_PROB = 0.7       # the directory name of the shipped model
MASK_UNITS = 120      # 100 units of layer 1, then 20 of layer 2
NW = 3541
SHAPES = {"W_1": (14, 100), "b_1": (100,), "W_2": (100, 20), "b_2": (20,), "W_O": (20, 1), "b_O": (1,)}


# ---------------------------------------------------------------------------------------------
# the dropout mask: the definition the kernel is held to, bit for bit
# ---------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _mix(z):
    """splitmix64's finalizer on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dropout_keep(seed: int, step: int, n: int, keep_prob: float) -> np.ndarray:
    """uint8 [n, 120]: keep of (row in batch, unit) at step `step` of a run with `seed`; units 0..99 are layer 1, 100..119 layer 2.
    key = mix(mix(seed) + step); one hash per pair of units, h = mix(key + 64 row + unit // 2): the even unit takes its bits 63..41, the odd unit bits
    40..18; u = float32(those 23 bits) / 2^23 in [0, 1); keep = floor(float32(keep_prob) + u) in float32 - TF1 dropout's floor(keep_prob + uniform)
    with this project's own counter-based stream."""
    with np.errstate(over="ignore"):
        key = _mix(_mix(np.array([seed & _M64], np.uint64)) + np.uint64(step & _M64))
        idx = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(64) + np.arange(MASK_UNITS // 2, dtype=np.uint64)[None, :]
        h = _mix(key + idx)
    bits = np.stack([h >> np.uint64(41), (h >> np.uint64(18)) & np.uint64(0x7FFFFF)], axis=2).reshape(n, MASK_UNITS)
    u = bits.astype(np.float32) * np.float32(1.0 / 8388608.0)
    return np.floor(np.float32(keep_prob) + u).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def read_truth(path: str, chrom=None, start=None, end=None, cov: int = COV_THRD) -> Dict[Tuple[str, str, int], float]:
    """readBed of hm_cluster_predict.py:20-41, rule for rule: the first line is skipped; lines of more than 20 characters (stripped) are kept and
    split at white space into 11 fields chr, start, end, _, _, strand, _, _, _, coverage, percentage (the ENCODE bisulfite bedMethyl layout);
    coverage < cov is dropped, then the region filter; (chr, strand, start) -> round(int(percentage) / 100.0, 3), a later duplicate overwriting an
    earlier one.  A kept line that does not split into 11 fields is refused with file and line number (the reference raises ValueError there)."""
    out = {}
    with open(path, "r") as fh:
        fh.readline()
        for lineno, line in enumerate(fh, 2):
            line = line.strip()
            if len(line) <= 20:
                continue
            fields = line.split()
            if len(fields) != 11:
                raise ValueError("%s:%d: expected 11 fields of a bedMethyl line, got %d" % (path, lineno, len(fields)))
            try:
                pos, true_cov = int(fields[1]), int(fields[9])
                if true_cov < cov:
                    continue
                perc = round(int(fields[10]) / 100.0, 3)
            except ValueError as exc:
                raise ValueError("%s:%d: %s" % (path, lineno, exc))
            if (chrom not in (None, fields[0])) or not ((start is None or pos >= start) and (end is None or pos <= end)):
                continue
            if true_cov == 0:
                continue
            out[(fields[0], fields[5], pos)] = perc
    return out


def contig_paths(pred_prefix: str, motif_folder: str, chrom: str) -> Tuple[str, str]:
    return "%s.%s.C.bed" % (pred_prefix, chrom), "%s/motif_%s_C.bed" % (motif_folder, chrom)


def contig_rows(pred_prefix: str, motif_folder: str, chrom: str, truth) -> Tuple[np.ndarray, np.ndarray, int]:
    """The feed of one contig exactly as cluster.hm_cluster_predict obtains it (read_motif, read_pred, cluster_features: neighbours count whether
    or not they have truth), reduced to the rows whose (chr, strand, pos) is a truth key -> (X float32 [n,14], Y float32 [n], sites of the contig);
    rows in the file's order ('+' sites ascending, then '-')."""
    pred_path, motif_path = contig_paths(pred_prefix, motif_folder, chrom)
    pred = cluster.read_pred(pred_path, chrom, cluster.read_motif(motif_path))
    x, lines = cluster.cluster_features(pred)
    keys = [(chrom, s, int(p)) for s in "+-" for p in pred[s][0]]
    keep = np.array([k in truth for k in keys], bool)
    y = np.array([truth[k] for k in keys if k in truth], np.float32)
    return np.ascontiguousarray(x[keep], np.float32).reshape(-1, 14), y, len(keys)


def build_dataset(pred_prefix: str, motif_folder: str, truth, chroms: List[str]):
    """-> (X, Y, {'with_truth': n, 'without_truth': n, 'per_contig': {chr: [with, without]}}): contigs in the given order."""
    xs, ys, per = [], [], {}
    for chrom in chroms:
        x, y, sites = contig_rows(pred_prefix, motif_folder, chrom, truth)
        xs.append(x)
        ys.append(y)
        per[chrom] = [int(len(y)), int(sites - len(y))]
    x = np.concatenate(xs) if xs else np.zeros((0, 14), np.float32)
    y = np.concatenate(ys) if ys else np.zeros(0, np.float32)
    return x, y, {"with_truth": int(len(y)), "without_truth": int(sum(v[1] for v in per.values())), "per_contig": per}


# ---------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------
def initial_weights(seed: int = 0) -> Dict[str, np.ndarray]:
    """The graph's initial values from numpy's generator (the project's own draw): truncated_normal(mean 0, stddev 1) - standard normal, redrawn
    beyond 2 standard deviations, as train.initial_weights draws the BiLSTM's head - for W_1, W_2, W_O; zeros for the biases."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in cluster.WEIGHT_ORDER:
        if name.startswith("b"):
            out[name] = np.zeros(SHAPES[name], np.float32)
            continue
        v = rng.standard_normal(SHAPES[name])
        while True:
            bad = np.abs(v) > 2.0
            if not bad.any():
                break
            v[bad] = rng.standard_normal(int(bad.sum()))
        out[name] = v.astype(np.float32)
    return out


def unflatten_cluster_weights(flat: np.ndarray) -> Dict[str, np.ndarray]:
    out, off = {}, 0
    for name in cluster.WEIGHT_ORDER:
        size = int(np.prod(SHAPES[name]))
        out[name] = np.ascontiguousarray(flat[off:off + size].reshape(SHAPES[name]), dtype=np.float32)
        off += size
    if off != flat.size:
        raise ValueError("expected %d floats, got %d" % (off, flat.size))
    return out


def checkpoint_tensors(w: np.ndarray, m: np.ndarray, v: np.ndarray, t: int) -> Dict[str, np.ndarray]:
    """What tf.train.Saver() stores for this graph, under the names of the reference's .index: the six variables, <name>/Adam (m), <name>/Adam_1 (v)
    and beta1_power / beta2_power as train.checkpoint_tensors writes them after t steps (beta ** (t + 1): TF1 starts them at beta)."""
    out = {}
    for blob, suffix in ((w, ""), (m, "/Adam"), (v, "/Adam_1")):
        for name, arr in unflatten_cluster_weights(blob).items():
            out[name + suffix] = arr
    out["beta1_power"] = np.array(BETA1 ** (t + 1), np.float32)
    out["beta2_power"] = np.array(BETA2 ** (t + 1), np.float32)
    return out


# ---------------------------------------------------------------------------------------------
# the handle
# ---------------------------------------------------------------------------------------------
class ClusterTrainer:
    """One dm_cluster_trainer on one GPU: weights, Adam slots, the resident rows and the loss record stay on the device."""

    def __init__(self, weights, device: int = 0, max_batch: int = cluster.BATCH_SIZE):
        self._lib = _lib.load()
        flat = cluster.flatten_cluster_weights(weights) if isinstance(weights, dict) else np.ascontiguousarray(weights, dtype=np.float32)
        self.device, self.max_batch = device, int(max_batch)
        self._h = self._lib.dm_cluster_trainer_create(device, flat.ctypes.data, flat.size, self.max_batch)
        if not self._h:
            raise _lib.DeepModHipError("dm_cluster_trainer_create: " + _lib.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dm_cluster_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _xy(x, y):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != 14 or y.shape != (x.shape[0],):
            raise ValueError("expected x [n,14] and y [n], got %s and %s" % (x.shape, y.shape))
        return x, y

    def set_data(self, x, y):
        x, y = self._xy(x, y)
        _lib.check(self._lib.dm_cluster_trainer_set_data(self._h, x.ctypes.data, y.ctypes.data, x.shape[0]))

    def grad(self, x, y, keep_prob: float = 1.0, keep=None, seed: int = 0, step: int = 0, want_out: bool = True, want_grad: bool = True):
        """-> (loss, out float32[n] or None, gradient blob float32[3541] or None); keep: uint8 [n,120] or None (the mask generated for (seed, step));
        the state does not change."""
        x, y = self._xy(x, y)
        n = x.shape[0]
        if keep is not None:
            keep = np.ascontiguousarray(keep, dtype=np.uint8)
            if keep.shape != (n, MASK_UNITS):
                raise ValueError("expected keep [%d,%d], got %s" % (n, MASK_UNITS, keep.shape))
        loss = ctypes.c_float(0.0)
        out = np.empty(n, np.float32) if want_out else None
        grad = (np.empty if n else np.zeros)(NW, np.float32) if want_grad else None
        _lib.check(self._lib.dm_cluster_trainer_grad(self._h, x.ctypes.data, y.ctypes.data, n, float(keep_prob), keep.ctypes.data if keep is not None else None,
                                                     int(seed) & _M64, int(step), ctypes.byref(loss), out.ctypes.data if want_out else None,
                                                     grad.ctypes.data if want_grad else None))
        return loss.value, out, grad

    def adam(self, grad):
        grad = np.ascontiguousarray(grad, dtype=np.float32)
        if grad.size != NW:
            raise ValueError("gradient blob of %d floats" % grad.size)
        _lib.check(self._lib.dm_cluster_trainer_adam(self._h, grad.ctypes.data))

    def step(self, ids, keep_prob: float = KEEP_PROB, seed: int = 0):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.ndim != 1:
            raise ValueError("expected ids [n], got %s" % (ids.shape,))
        _lib.check(self._lib.dm_cluster_trainer_step(self._h, ids.ctypes.data, ids.shape[0], float(keep_prob), int(seed) & _M64))

    def losses(self, first_step: int, count: int) -> np.ndarray:
        out = np.empty(count, np.float32)
        _lib.check(self._lib.dm_cluster_trainer_losses(self._h, int(first_step), int(count), out.ctypes.data))
        return out

    def mask(self, seed: int, step: int, n: int, keep_prob: float) -> np.ndarray:
        out = np.empty((n, MASK_UNITS), np.uint8)
        _lib.check(self._lib.dm_cluster_trainer_mask(self._h, int(seed) & _M64, int(step), int(n), float(keep_prob), out.ctypes.data))
        return out

    def get_state(self):
        """-> (weights, m, v float32[3541], t)"""
        w, m, v = (np.empty(NW, np.float32) for _ in range(3))
        t = ctypes.c_int64(0)
        _lib.check(self._lib.dm_cluster_trainer_get_state(self._h, w.ctypes.data, m.ctypes.data, v.ctypes.data, ctypes.byref(t)))
        return w, m, v, t.value

    def set_state(self, w=None, m=None, v=None, t: int = 0):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (w, m, v)]
        for a in arrs:
            if a is not None and a.size != NW:
                raise ValueError("state blob of %d floats" % a.size)
        _lib.check(self._lib.dm_cluster_trainer_set_state(self._h, *[None if a is None else a.ctypes.data for a in arrs], int(t)))


# ---------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------
def check_options(mo) -> None:
    """What `traincluster` refuses before it reads anything, one line each."""
    if not (0.0 < mo['keep_prob'] <= 1.0):
        raise SystemExit("Error: traincluster: --keep_prob %g outside (0, 1]" % mo['keep_prob'])
    if mo['epochs'] < 1 or mo['batchsize'] < 1 or mo['batchsize'] > 65536:
        raise SystemExit("Error: traincluster: --epochs must be at least 1 and --batchsize in [1, 65536]")
    both = [c for c in mo['chr'] if c in mo['heldout']]
    if both:
        raise SystemExit("Error: traincluster: contig %s is named in both --chr and --heldout" % ",".join(both))
    if not mo['predFile'] or not mo['motifFolder'] or not mo['truth']:
        raise SystemExit("Error: traincluster: --predFile, --motifFolder and --truth are needed")
    for path in mo['truth'] + [p for c in mo['chr'] + mo['heldout'] for p in contig_paths(mo['predFile'], mo['motifFolder'], c)]:
        if not os.path.isfile(path):
            raise SystemExit("Error: traincluster: no file %s" % path)


def pearson_r(a: np.ndarray, b: np.ndarray) -> Optional[float]:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if len(a) < 2 or a.std() == 0.0 or b.std() == 0.0:
        return None
    return float(np.corrcoef(a, b)[0, 1])


def score(weights_flat: np.ndarray, x: np.ndarray, y: np.ndarray, device: int = 0):
    """MSE and Pearson r of the model at keep_prob 1 on rows (x, y): the existing scoring kernel (dm_cluster_predict)."""
    model = cluster.ClusterModel(unflatten_cluster_weights(weights_flat), device)
    try:
        p = model.predict(x).astype(np.float64)
    finally:
        model.close()
    return float(np.mean((p - y.astype(np.float64)) ** 2)), pearson_r(p, y)


def train_cluster(mo, device: int = 0) -> dict:
    """The whole command (module docstring).  -> what <FileID>_cluster_train.json holds."""
    check_options(mo)
    truth = {}
    for path in mo['truth']:
        try:
            truth.update(read_truth(path, cov=mo['cov']))
        except ValueError as exc:
            raise SystemExit("Error: traincluster: --truth: %s" % exc)
    x, y, counts = build_dataset(mo['predFile'], mo['motifFolder'], truth, mo['chr'])
    if len(y) == 0:
        raise SystemExit("Error: traincluster: no site of %s has truth with coverage >= %d in %s" % (",".join(mo['chr']), mo['cov'], ",".join(mo['truth'])))
    held = None
    if mo['heldout']:
        hx, hy, hcounts = build_dataset(mo['predFile'], mo['motifFolder'], truth, mo['heldout'])
        if len(hy) == 0:
            raise SystemExit("Error: traincluster: no site of the --heldout contigs %s has truth" % ",".join(mo['heldout']))
        held = (hx, hy, hcounts)
    if _lib.load().dm_device_count() < 1:
        raise SystemExit('Error: no gfx950 GPU visible (this build has no CPU path)')
    os.makedirs(mo['outFolder'], exist_ok=True)
    seed, bs, n = int(mo['seed']), int(mo['batchsize']), len(y)
    trainer = ClusterTrainer(initial_weights(seed), device, max_batch=bs)
    report = {"inputs": {k: mo[k] for k in ('predFile', 'motifFolder', 'truth', 'chr', 'heldout', 'cov', 'keep_prob', 'epochs', 'batchsize', 'seed')},
              "sites": counts, "heldout_sites": held[2] if held else None, "epochs": [], "best_epoch": None}
    try:
        trainer.set_data(x, y)
        for epoch in range(1, mo['epochs'] + 1):
            order = np.random.default_rng([seed, epoch - 1]).permutation(n)
            t0, sizes = trainer.get_state()[3], []
            for lo in range(0, n, bs):
                ids = order[lo:lo + bs]
                trainer.step(ids, mo['keep_prob'], seed)
                sizes.append(len(ids))
            try:
                losses = trainer.losses(t0, len(sizes))
            except _lib.DeepModHipError as exc:
                raise SystemExit("Error: traincluster: epoch %d: %s" % (epoch, exc))
            w, m, v, t = trainer.get_state()
            prefix = os.path.join(mo['outFolder'], "Cg.cov%d.nb%d-%d" % (mo['cov'], cluster.NBSIZE, epoch))
            tfbundle.write_bundle(prefix, checkpoint_tensors(w, m, v, t))
            entry = {"epoch": epoch, "steps": len(sizes), "t": int(t), "checkpoint": os.path.basename(prefix),
                     "train_mse": float(np.sum(losses.astype(np.float64) * np.array(sizes)) / n), "heldout_mse": None, "heldout_r": None}
            if held:
                entry["heldout_mse"], entry["heldout_r"] = score(w, held[0], held[1], device)
            report["epochs"].append(entry)
            if mo.get('outLevel', 2) <= 2:
                print("traincluster epoch %d: steps=%d train_mse=%.6f%s -> %s" % (epoch, len(sizes), entry["train_mse"],
                      "" if not held else " heldout_mse=%.6f r=%s" % (entry["heldout_mse"], entry["heldout_r"]), prefix), flush=True)
    finally:
        trainer.close()
    if held:
        report["best_epoch"] = min(report["epochs"], key=lambda e: (e["heldout_mse"], e["epoch"]))["epoch"]
    write_json(os.path.join(mo['outFolder'], "%s_cluster_train.json" % mo['FileID']), report)
    return report
