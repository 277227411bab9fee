"""`DeepMod.py train` on the GPU: the training half of the reference (bin/DeepMod_scripts/myMultiBiRNN.py) over dm_trainer_* of the C ABI.

The function names of the reference are kept:
  getTFiles1               :233-251   the *.xy.gz files of a folder (same glob depths, same --test P,<pct> slicing; every glob result is
                                      sorted first - the reference's order is whatever the file system returns)
  getDataFromFile_new      :306-361   np.loadtxt -> position | 2 labels | 7 features -> the windows tx[mind-10 : mind+11] of the labelled rows
  train_save_model         :96-228    4 epochs, the group / sub-batch schedule of :128-190 and its checkpoint schedule
  mMult_RNN_LSTM_train     :425-460   groups from --wrkBase "a,b;c", np.random.seed(3) shuffles, the largest group first
Forward, backpropagation through time and Adam run in HIP kernels (csrc/train.hip.inc); this module reads files, schedules batches and writes
checkpoints.  No torch, no CPU path.

Initialisation is TF1's (glorot-uniform kernels, zero biases, truncated-normal head) drawn from a numpy generator seeded by --seed:
TensorFlow's own random stream cannot be reproduced, so a run here and a run of the reference start from different draws of the same
distributions.  Checkpoints are TF bundles with the variables, the Adam slots and beta1_power / beta2_power under the names and shapes of
the reference's .index files, plus the `checkpoint` state file; no .meta is written (a serialized graph this build's detect does not need).

Beside every checkpoint the schedule writes <prefix>.train.json: its own position (epoch, reader positions, step count t) and what it depends on
(batchsize, unbalanced, test, a digest of the file lists).  --resume reads it and the bundle back and continues: every later checkpoint is byte
for byte the uninterrupted run's.  --startFrom takes only the 14 variables of a bundle and runs the whole schedule.  --validate K keeps at least
K windows of the files --test held out on the device (xyload.XYSet) and scores them at every checkpoint as `predict` would (<prefix>.valid.json).
"""
from __future__ import annotations

import ctypes
import glob
import hashlib
import json
import os
import sys
import time
from typing import Dict, List, Optional

import numpy as np

from . import _lib, tfbundle
from .model import HID, LAYERS, NFEAT, WIN, flatten_weights
from .synth import HEAD_B, HEAD_W, cell_name

batchsize = 2048                     # myMultiBiRNN.py:12; train_save_model takes it as a parameter as well
TRAINING_STEPS = 4                   # epochs (:97)
SUMPSIZE = 25                        # sub-batches loaded per round of the first group (:108)
BETA1, BETA2 = 0.9, 0.999


# ---------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------
def blob_names():
    """(name, shape) of the tensors of the canonical blob, in blob order."""
    out = []
    for d in ("fw", "bw"):
        for layer in range(LAYERS):
            kin = NFEAT if layer == 0 else HID
            out.append((cell_name(d, layer, "kernel"), (kin + HID, 4 * HID)))
            out.append((cell_name(d, layer, "bias"), (4 * HID,)))
    out += [(HEAD_W, (2 * HID, 2)), (HEAD_B, (2,))]
    return out


def unflatten_weights(flat: np.ndarray) -> Dict[str, np.ndarray]:
    out, off = {}, 0
    for name, shape in blob_names():
        size = int(np.prod(shape))
        out[name] = np.ascontiguousarray(flat[off:off + size].reshape(shape), dtype=np.float32)
        off += size
    if off != flat.size:
        raise ValueError("expected %d floats, got %d" % (off, flat.size))
    return out


def initial_weights(seed: int = 0) -> Dict[str, np.ndarray]:
    """TF1's initial values of mCreateSession's variables (:34-35, :42-43): BasicLSTMCell kernels glorot-uniform (the default initializer of
    tf.get_variable), biases zero, head W and b tf.truncated_normal (standard normal, redrawn beyond 2 sigma) - from numpy's generator."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in blob_names():
        if name in (HEAD_W, HEAD_B):
            v = rng.standard_normal(shape)
            while True:
                bad = np.abs(v) > 2.0
                if not bad.any():
                    break
                v[bad] = rng.standard_normal(int(bad.sum()))
            out[name] = v.astype(np.float32)
        elif name.endswith("bias"):
            out[name] = np.zeros(shape, np.float32)
        else:
            a = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[name] = rng.uniform(-a, a, shape).astype(np.float32)
    return out


class Trainer:
    """One dm_trainer on one GPU: weights, Adam slots and the tape stay on the device."""

    def __init__(self, weights, device: int = 0, max_batch: int = 2 * batchsize):
        self._lib = _lib.load()
        flat = flatten_weights(weights) if isinstance(weights, dict) else np.ascontiguousarray(weights, dtype=np.float32)
        self.device, self.max_batch = device, int(max_batch)
        self._h = self._lib.dm_trainer_create(device, flat.ctypes.data, flat.size, NFEAT, HID, WIN, LAYERS, self.max_batch)
        if not self._h:
            raise _lib.DeepModHipError("dm_trainer_create: " + _lib.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dm_trainer_destroy(self._h)
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
        if x.ndim != 3 or x.shape[1:] != (WIN, NFEAT) or y.shape != (x.shape[0], 2):
            raise ValueError("expected x [n,%d,%d] and y [n,2], got %s and %s" % (WIN, NFEAT, x.shape, y.shape))
        return x, y

    def grad(self, x, y, unbalanced: bool = False, want_prob: bool = True, want_grad: bool = True):
        """-> (loss, prob float32[n,2] or None, gradient blob float32[408402] or None); the state does not change.  An empty batch gives loss 0 and
        a zero gradient."""
        x, y = self._xy(x, y)
        n = x.shape[0]
        loss = ctypes.c_float(0.0)
        prob = np.empty((n, 2), np.float32) if want_prob else None
        grad = (np.empty if n else np.zeros)(_lib.DM_WEIGHT_FLOATS, np.float32) if want_grad else None       # n = 0: the library writes nothing
        _lib.check(self._lib.dm_trainer_grad(self._h, x.ctypes.data, y.ctypes.data, n, 1 if unbalanced else 0, ctypes.byref(loss),
                                             prob.ctypes.data if want_prob else None, grad.ctypes.data if want_grad else None))
        return loss.value, prob, grad

    def adam(self, grad):
        grad = np.ascontiguousarray(grad, dtype=np.float32)
        if grad.size != _lib.DM_WEIGHT_FLOATS:
            raise ValueError("gradient blob of %d floats" % grad.size)
        _lib.check(self._lib.dm_trainer_adam(self._h, grad.ctypes.data))

    def step(self, x, y, unbalanced: bool = False) -> float:
        x, y = self._xy(x, y)
        loss = ctypes.c_float(0.0)
        _lib.check(self._lib.dm_trainer_step(self._h, x.ctypes.data, y.ctypes.data, x.shape[0], 1 if unbalanced else 0, ctypes.byref(loss)))
        return loss.value

    @staticmethod
    def _ids_y(ids, y):
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        y = np.ascontiguousarray(y, dtype=np.float32)
        if ids.ndim != 1 or y.shape != (ids.shape[0], 2):
            raise ValueError("expected ids [n] and y [n,2], got %s and %s" % (ids.shape, y.shape))
        return ids, y

    def grad_set(self, xyset, ids, y, unbalanced: bool = False, want_prob: bool = True, want_grad: bool = True):
        """grad() of the windows `ids` of an xyload.XYSet on this device, gathered there: 8 B of id and 8 B of y per window go up."""
        ids, y = self._ids_y(ids, y)
        n = ids.shape[0]
        loss = ctypes.c_float(0.0)
        prob = np.empty((n, 2), np.float32) if want_prob else None
        grad = (np.empty if n else np.zeros)(_lib.DM_WEIGHT_FLOATS, np.float32) if want_grad else None
        _lib.check(self._lib.dm_trainer_grad_set(self._h, xyset._h, ids.ctypes.data, y.ctypes.data, n, 1 if unbalanced else 0, ctypes.byref(loss),
                                                 prob.ctypes.data if want_prob else None, grad.ctypes.data if want_grad else None))
        return loss.value, prob, grad

    def step_set(self, xyset, ids, y, unbalanced: bool = False) -> float:
        """step() of the windows `ids` of an xyload.XYSet on this device: the host-fed step's results bit for bit."""
        ids, y = self._ids_y(ids, y)
        loss = ctypes.c_float(0.0)
        _lib.check(self._lib.dm_trainer_step_set(self._h, xyset._h, ids.ctypes.data, y.ctypes.data, ids.shape[0], 1 if unbalanced else 0, ctypes.byref(loss)))
        return loss.value

    def profile(self, on: bool = True):
        """-> (ms, steps) of the dm_trainer_step calls since the last call (HIP events on the trainer's stream), then switches the bracketing."""
        ms, steps = ctypes.c_double(0.0), ctypes.c_int64(0)
        _lib.check(self._lib.dm_trainer_profile(self._h, 1 if on else 0, ctypes.byref(ms), ctypes.byref(steps)))
        return ms.value, steps.value

    def get_state(self):
        """-> (weights, m, v float32[408402], t)"""
        w, m, v = (np.empty(_lib.DM_WEIGHT_FLOATS, np.float32) for _ in range(3))
        t = ctypes.c_int64(0)
        _lib.check(self._lib.dm_trainer_get_state(self._h, w.ctypes.data, m.ctypes.data, v.ctypes.data, ctypes.byref(t)))
        return w, m, v, t.value

    def set_state(self, w=None, m=None, v=None, t: int = 0):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (w, m, v)]
        for a in arrs:
            if a is not None and a.size != _lib.DM_WEIGHT_FLOATS:
                raise ValueError("state blob of %d floats" % a.size)
        _lib.check(self._lib.dm_trainer_set_state(self._h, *[None if a is None else a.ctypes.data for a in arrs], int(t)))


def checkpoint_tensors(w: np.ndarray, m: np.ndarray, v: np.ndarray, t: int) -> Dict[str, np.ndarray]:
    """What tf.train.Saver() stores for this graph: every variable, its Adam slots <name>/Adam (m) and <name>/Adam_1 (v), and the optimizer's
    beta1_power / beta2_power (beta ** (t + 1): TF1 initialises them to beta and multiplies after every step)."""
    out = {}
    for blob, suffix in ((w, ""), (m, "/Adam"), (v, "/Adam_1")):
        for name, arr in unflatten_weights(blob).items():
            out[name + suffix] = arr
    out["beta1_power"] = np.array(BETA1 ** (t + 1), np.float32)
    out["beta2_power"] = np.array(BETA2 ** (t + 1), np.float32)
    return out


class TrainSaver:
    """saver.save(sess, prefix): a TF bundle (tfbundle.write_bundle) + the `checkpoint` state file; no .meta."""

    last_saved = None                                   # (weights blob, t) of the last save: --validate scores what was written

    def save(self, sess: "TrainSession", prefix: str):
        w, m, v, t = sess.trainer.get_state()
        tfbundle.write_bundle(prefix, checkpoint_tensors(w, m, v, t))
        self.last_saved = (w, t)
        return prefix

    def restore_training(self, sess: "TrainSession", prefix: str, t: int, slots: bool):
        """The trainer's state from the bundle at prefix: the 14 variables, and with slots (--resume) the Adam slots and step count t;
        without (--startFrom) m = v = 0 and t = 0."""
        w, m, v = load_training_state(prefix, t, slots)
        if sess.trainer is None:
            sess.run(sess.graph.init)
        sess.trainer.set_state(w, m, v, t if slots else 0)


def load_training_state(prefix: str, t: int, slots: bool):
    """-> (w, m, v) blobs of the bundle at prefix.  Refused in one line: a bundle that is not there, a tensor that is missing or has another
    shape, and with slots beta1_power / beta2_power that are not those of step count t."""
    what = "--resume" if slots else "--startFrom"
    if not os.path.isfile(prefix + ".index"):
        raise SystemExit("Error: %s: no TF checkpoint at %r" % (what, prefix))
    entries = tfbundle.read_index(prefix + ".index")
    suffixes = ("", "/Adam", "/Adam_1") if slots else ("",)
    for suffix in suffixes:
        for name, shape in blob_names():
            if name + suffix not in entries:
                raise SystemExit("Error: %s: %s holds no tensor %r" % (what, prefix, name + suffix))
            if tuple(entries[name + suffix].shape) != tuple(shape):
                raise SystemExit("Error: %s: tensor %r of %s has shape %s, this model needs %s" %
                                 (what, name + suffix, prefix, tuple(entries[name + suffix].shape), tuple(shape)))
    powers = ("beta1_power", "beta2_power") if slots else ()
    for name in powers:
        if name not in entries:
            raise SystemExit("Error: %s: %s holds no tensor %r" % (what, prefix, name))
    tensors = tfbundle.load_bundle(prefix, [name + suffix for suffix in suffixes for name, _ in blob_names()] + list(powers))
    for name, beta in zip(powers, (BETA1, BETA2)):
        want = np.float32(beta ** (t + 1))
        if np.float32(tensors[name]) != want:
            raise SystemExit("Error: %s: %s of %s is %r, step count t = %d of its .train.json gives %r" %
                             (what, name, prefix, float(tensors[name]), t, float(want)))
    blobs = [flatten_weights({name: tensors[name + suffix] for name, _ in blob_names()}) for suffix in suffixes]
    zero = np.zeros(_lib.DM_WEIGHT_FLOATS, np.float32)
    return (blobs[0], blobs[1], blobs[2]) if slots else (blobs[0], zero, zero.copy())


# ---------------------------------------------------------------------------------------------
# the TF1-shaped seam: sess.run([train_op, loss_op], feed_dict={X: x, Y: y}) on a model.Session
# ---------------------------------------------------------------------------------------------
class _Op:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<deepmod_amd train %s>" % self.name


class TrainGraph:
    """The training tokens model.mCreateSession hands out; X, Y, init, init_l, mfpred and prediction are those of its Graph (`share`)."""

    def __init__(self, num_input, num_hidden, timesteps, moptions, share=None):
        if (num_input, num_hidden, timesteps) != (NFEAT, HID, WIN):
            raise ValueError("this build supports fnum=7 hidden=100 windowsize=21 only (got %s)" % ((num_input, num_hidden, timesteps),))
        self.unbalanced = moptions.get("unbalanced") == 1
        self.seed = int(moptions.get("seed", 0) or 0)
        self.max_batch = int(moptions.get("max_batch") or 2 * batchsize - 1)
        for n in ("init", "init_l", "loss_op", "accuracy", "train_op", "X", "Y", "auc_op", "mpre", "mspf", "mfpred", "prediction"):
            setattr(self, n, _Op(n))
        self.auc_op = (_Op("auc_value"), self.auc_op)       # tf.metrics.* return (value, update_op); the reference fetches [1]
        self.mpre = (_Op("precision_value"), self.mpre)
        self.mspf = (_Op("recall_value"), self.mspf)
        self.saver = TrainSaver()
        if share is not None:                               # model.mCreateSession: one set of placeholders for detect and train
            for n in ("init", "init_l", "X", "Y", "mfpred", "prediction"):
                setattr(self, n, getattr(share, n))

    def is_train_token(self, f) -> bool:
        return any(f is t for t in (self.loss_op, self.accuracy, self.train_op, self.auc_op[1], self.mpre[1], self.mspf[1]))


class SetWindows:
    """X of a feed whose windows are not on the host: the ids of windows of an xyload.XYSet (TrainSession.run gathers them on the device)."""

    def __init__(self, xyset, ids):
        self.set, self.ids = xyset, np.ascontiguousarray(ids, dtype=np.int64)

    def __len__(self):
        return len(self.ids)


class TrainSession:
    """The training side of model.Session (which creates one at the first fetch of a training token): run(init) creates the trainer from the
    seeded initial values, run([train_op, loss_op], feed) is one dm_trainer_step, a fetch without train_op is one dm_trainer_grad (loss,
    accuracy, precision, recall, AUC of that batch: the metrics are reset before every progress line, so they are the batch's own).  A
    batch larger than the tape makes the trainer grow, state kept.  An X that is a SetWindows routes to dm_trainer_step_set / _grad_set; the
    set is not the trainer's, so it outlives a growth."""

    def __init__(self, graph: TrainGraph, device: int = 0):
        self.graph, self.device = graph, device
        self.trainer: Optional[Trainer] = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.trainer is not None:
            self.trainer.close()
            self.trainer = None

    def _fit(self, n):
        """A batch larger than the tape: a new trainer of that size takes over weights, Adam slots and step count."""
        if n <= self.trainer.max_batch:
            return
        state = self.trainer.get_state()
        self.trainer.close()
        self.trainer = Trainer(state[0], self.device, n + n // 8)
        self.trainer.set_state(*state)

    def run(self, fetches, feed_dict=None):
        g = self.graph
        single = not isinstance(fetches, (list, tuple))
        flist = [fetches] if single else list(fetches)
        if all(f is g.init or f is g.init_l for f in flist):
            if any(f is g.init for f in flist) and self.trainer is None:
                self.trainer = Trainer(initial_weights(g.seed), self.device, g.max_batch)
            return None if single else [None] * len(flist)
        if self.trainer is None:
            raise _lib.DeepModHipError("TrainSession.run before run(init)")
        if feed_dict is None or g.X not in feed_dict or g.Y not in feed_dict:
            raise ValueError("feed_dict must provide X and Y")
        x, y = feed_dict[g.X], np.asarray(feed_dict[g.Y])
        from_set = isinstance(x, SetWindows)            # `train --resident 1`: the windows stay on the device, the feed names them by id
        if not from_set:
            x = np.asarray(x)
        self._fit(len(x))
        prob = None
        if any(f is g.train_op for f in flist):
            if any(f is not g.train_op and f is not g.loss_op for f in flist):
                raise ValueError("train_op can be fetched together with loss_op only")
            loss = self.trainer.step_set(x.set, x.ids, y, g.unbalanced) if from_set else self.trainer.step(x, y, g.unbalanced)
        elif from_set:
            loss, prob, _ = self.trainer.grad_set(x.set, x.ids, y, g.unbalanced, want_prob=True, want_grad=False)
        else:
            loss, prob, _ = self.trainer.grad(x, y, g.unbalanced, want_prob=True, want_grad=False)
        out = []
        for f in flist:
            if f is g.train_op:
                out.append(None)
            elif f is g.loss_op:
                out.append(np.float32(loss))
            elif f is g.prediction:
                out.append(prob)
            elif f is g.mfpred:
                out.append(np.argmax(prob, 1).astype(np.int64))
            elif f is g.accuracy or f is g.auc_op[1] or f is g.mpre[1] or f is g.mspf[1]:
                pred, lab = np.argmax(prob, 1), np.argmax(y, 1)
                tp = float(((pred == 1) & (lab == 1)).sum())
                if f is g.accuracy:
                    out.append(np.float32((pred == lab).mean()))
                elif f is g.mpre[1]:
                    out.append(np.float32(tp / max(float((pred == 1).sum()), 1.0)))
                elif f is g.mspf[1]:
                    out.append(np.float32(tp / max(float((lab == 1).sum()), 1.0)))
                else:
                    from .siteperf import roc_auc
                    both = 0 < int(lab.sum()) < len(lab)
                    out.append(np.float32(roc_auc(lab, prob[:, 1]) if both else 0.0))
            else:
                raise ValueError("cannot fetch %r" % (f,))
        return out[0] if single else out


# ---------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------
FEATURE_PATTERN = "*.xy.gz"
MAX_DEPTH = 4                        # sub-folder levels searched with --recursive 1


def getTFiles1(folder1, moptions):
    """The feature files of one folder: the folder itself, then (--recursive 1) one to four levels of sub-folders, each level in sorted order.
    Under --test P,<pct> (moptions['test'] == ['0', fraction]) only a share of them trains: the first int(n * fraction) files for a
    fraction above one half, else the last int(n * fraction)."""
    depths = range(MAX_DEPTH + 1) if moptions['recursive'] == 1 else range(1)
    found = []
    for depth in depths:
        found += sorted(glob.glob(os.path.join(folder1, *(["*"] * depth), FEATURE_PATTERN)))
    kind, *rest = moptions['test']
    if kind == '0':
        keep = int(len(found) * rest[0])
        found = found[:keep] if rest[0] > 0.5 else found[len(found) - keep:]
    print("%s: %d feature files" % (folder1, len(found)))
    sys.stdout.flush()
    return found


def getDataFromFile_new(fn, moptions, mfind0ld=None):
    """One feature file (text rows: position | 2 labels | 7 features) -> (windows float32 [k,21,7], labels int [k,2], None): one window of
    windowsize rows around every labelled row.  Rows with both labels below 0.01 carry no label.  --test E,a,b (['-', lo, hi]) leaves out
    rows with lo < position < hi, ['+', lo, hi] keeps only those.  A window that holds a NaN is dropped and the file is named once.  A
    labelled row without a whole window inside the file is an error that names file and row.  ([], [], None) when nothing is left."""
    table = np.loadtxt(fn, dtype=np.float32, ndmin=2)
    rows = labelled_rows(table, moptions, fn)
    if len(rows) == 0:
        return ([], [], None)
    half = int(moptions['windowsize'] / 2)
    index = rows[:, None] + np.arange(-half, half + 1)[None, :]
    return (np.ascontiguousarray(table[:, 3:][index]), table[rows, 1:3].astype(int), None)


def labelled_rows(table, moptions, fn):
    """The selection of getDataFromFile_new on a loaded table: the rows whose windows it returns, ascending (`predict` states its device
    selection against this)."""
    position, labels, feats = table[:, 0], table[:, 1:3], table[:, 3:]
    half = int(moptions['windowsize'] / 2)
    wanted = ~((labels[:, 0] < 0.01) & (labels[:, 1] < 0.01))
    kind = moptions['test'][0]
    if kind in ('-', '+'):
        ipos = position.astype(int)
        inside = (moptions['test'][1] < ipos) & (ipos < moptions['test'][2])
        wanted &= ~inside if kind == '-' else inside
    rows = np.flatnonzero(wanted)
    short = rows[(rows < half) | (rows + half >= len(feats))]
    if len(short):
        raise ValueError("%s: labelled row %d is closer than %d rows to the edge of the file (%d rows): no whole window" %
                         (fn, int(short[0]), half, len(feats)))
    if len(rows) == 0:
        return rows
    bad_before = np.concatenate(([0], np.cumsum(np.isnan(feats).any(axis=1))))
    clean = bad_before[rows + half + 1] == bad_before[rows - half]
    if not clean.all():
        print("Warning: NaN in a window of %s: such windows are dropped" % fn)
    return rows[clean]


# ---------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------
class _GroupReader:
    """The files of one group, read in order; the position is kept between rounds."""

    def __init__(self, files, moptions):
        self.files, self.moptions, self.next = list(files), moptions, 0

    def exhausted(self):
        return self.next >= len(self.files)

    def pool(self, windows_wanted, wrap):
        """Read whole files until at least windows_wanted windows are pooled.  wrap: start over at the end of the list (the smaller groups are
        recycled against the leading one); otherwise stop there."""
        xs, ys, have, idle = [], [], 0, 0
        while have < windows_wanted:
            if self.exhausted():
                if not wrap:
                    break
                self.next = 0
            x, y, _ = getDataFromFile_new(self.files[self.next], self.moptions)
            self.next += 1
            if len(y) > 0:
                xs.append(x)
                ys.append(y)
                have += len(y)
                idle = 0
            else:
                idle += 1
                if idle > len(self.files):
                    raise ValueError("no labelled window in any of the %d files of a group (first: %s)" % (len(self.files), self.files[0]))
        if not xs:
            return np.zeros((0, WIN, NFEAT), np.float32), np.zeros((0, 2), int)
        return np.concatenate(xs, axis=0), np.concatenate(ys, axis=0)


class ResidentCatalogue:
    """What `train --resident 1` knows of its files once they are loaded: per file its number of windows, its first window id in the set
    (-1: the file has no window and therefore no segment) and y int [k,2] of its windows.  A window's id is its index over the concatenated
    segments, in load order.  Host data only."""

    def __init__(self):
        self.windows, self.first, self.y, self.total = {}, {}, {}, 0

    def __contains__(self, fn):
        return fn in self.windows

    def add(self, fn, y):
        k = len(y)
        self.windows[fn] = k
        self.first[fn] = self.total if k > 0 else -1
        self.y[fn] = np.asarray(y, dtype=int).reshape(k, 2)
        self.total += k


class _ResidentReader:
    """_GroupReader on a catalogue: pool() names the windows it would have read - (ids int64 [k], y int [k,2]) - with the same file order,
    position, recycling and errors."""

    def __init__(self, files, catalogue):
        self.files, self.catalogue, self.next = list(files), catalogue, 0

    def exhausted(self):
        return self.next >= len(self.files)

    def pool(self, windows_wanted, wrap):
        ids, ys, have, idle = [], [], 0, 0
        while have < windows_wanted:
            if self.exhausted():
                if not wrap:
                    break
                self.next = 0
            fn = self.files[self.next]
            self.next += 1
            k = self.catalogue.windows[fn]
            if k > 0:
                first = self.catalogue.first[fn]
                ids.append(np.arange(first, first + k, dtype=np.int64))
                ys.append(self.catalogue.y[fn])
                have += k
                idle = 0
            else:
                idle += 1
                if idle > len(self.files):
                    raise ValueError("no labelled window in any of the %d files of a group (first: %s)" % (len(self.files), self.files[0]))
        if not ids:
            return np.zeros(0, np.int64), np.zeros((0, 2), int)
        return np.concatenate(ids), np.concatenate(ys, axis=0)


RESIDENT_BYTES = "DEEPMOD_RESIDENT_BYTES"


class ResidentData:
    """--resident 1: every file of every group, once through XYLoader.load under the run's moptions['test'] (device parser and selection, host
    fallback with its note) and appended to one xyload.XYSet; gunzip runs ahead on --threads host threads.  A labelled row without a whole
    window is the loader's error, raised here and not when the schedule reaches the file.  The set larger than DEEPMOD_RESIDENT_BYTES, or a
    device allocation that fails, ends the run in one line before its first step."""

    def __init__(self, filelists, moptions, device: int = 0, initial_rows: int = 1 << 16):
        from concurrent.futures import ThreadPoolExecutor
        from . import predict, xyload
        self.catalogue = ResidentCatalogue()
        files = list(dict.fromkeys(fn for group in filelists for fn in group))
        budget = os.environ.get(RESIDENT_BYTES)
        budget = int(budget) if budget not in (None, "") else None
        threads = max(int(moptions.get('threads') or 1), 1)
        started = time.time()
        rows_total = 0
        self.set = xyload.XYSet(device, initial_rows)
        loader = xyload.XYLoader(device)

        def too_large(fn, why):
            return SystemExit("Error: --resident: %s at %s (file %d of %d) with %d bytes held%s: run without --resident" %
                              (why, fn, len(self.catalogue.windows) + 1, len(files), self.set.nbytes(),
                               "" if budget is None else ", budget %s=%d" % (RESIDENT_BYTES, budget)))
        try:
            with ThreadPoolExecutor(threads) as pool:
                ahead, nxt = [], 0                      # at most 2 * threads texts in flight
                for _ in files:
                    while nxt < len(files) and len(ahead) < 2 * threads:
                        ahead.append((files[nxt], pool.submit(predict.read_text, files[nxt])))
                        nxt += 1
                    fn, fut = ahead.pop(0)
                    try:
                        rows, n, _ = loader.load(fut.result(), moptions, fn)
                        y = np.zeros((0, 2), int)
                        if n > 0:
                            y = loader.fetch_head()[loader.fetch_selection()[0], 1:3].astype(int)
                            self.set.append(loader)
                    except _lib.DeepModHipError as exc:
                        if exc.code != _lib.DM_ENOMEM:
                            raise
                        for _, other in ahead:
                            other.cancel()
                        raise too_large(fn, "the device has no room for the training files")
                    if budget is not None and self.set.nbytes() > budget:
                        for _, other in ahead:
                            other.cancel()
                        raise too_large(fn, "the training files pass the budget")
                    self.catalogue.add(fn, y)
                    rows_total += rows
        except BaseException:
            self.close()
            raise
        finally:
            loader.close()
        print("resident: %d files, %d rows, %d windows stay on the device: %d bytes (%.2f s)" %
              (len(files), rows_total, self.catalogue.total, self.set.nbytes(), time.time() - started))
        sys.stdout.flush()

    def close(self):
        if getattr(self, "set", None) is not None:
            self.set.close()
            self.set = None


def _progress_interval(n_files):
    """Files of the leading group between two progress lines: 1 % of them, at least 2, in tens above 10, at most 100."""
    every = n_files / 100
    if every < 2:
        every = 2
    if every > 10:
        every = int(every / 10) * 10
    return min(every, 100)


def _mid_epoch_folder(percent, single_group):
    """Folder suffix of a checkpoint inside an epoch, or None: '.50' at half of the leading group's files; a run with one group also saves at
    10 ... 90 % ('0.1' ... '0.9')."""
    if percent == 50:
        return '.50'
    if single_group and percent in (10, 20, 30, 40, 60, 70, 80, 90):
        return str(round(percent / 100.0, 2))
    return None


STATE_VERSION = 1


def wrkbase_folders(moptions) -> List[str]:
    """Every folder --wrkBase names, groups and their folders in the order given."""
    return [folder for folder in moptions['wrkBase'].replace(';', ',').split(',') if folder]


def _relative(fn, folders):
    """'<index of the --wrkBase folder>:<path below it>' of a file (the longest folder that holds it), so that a data set that moved is the same."""
    best = None
    for i, folder in enumerate(folders):
        base = os.path.join(os.path.abspath(folder), "")
        if os.path.abspath(fn).startswith(base) and (best is None or len(base) > len(best[1])):
            best = (i, base)
    if best is None:
        return os.path.abspath(fn)
    return "%d:%s" % (best[0], os.path.abspath(fn)[len(best[1]):].replace(os.sep, "/"))


def filelists_digest(filelists, moptions) -> str:
    """SHA-256 of the ordered file lists (after file_groups: --test P slicing, shuffle, the largest group first), paths relative to their
    --wrkBase folder."""
    folders = wrkbase_folders(moptions) if moptions.get('wrkBase') else []
    text = json.dumps([[_relative(fn, folders) for fn in files] for files in filelists])
    return hashlib.sha256(text.encode("utf-8")).hexdigest()


def _json_form(value):
    return json.loads(json.dumps(value))


def schedule_state(epoch, closed, readers, t, batchsize, moptions, digest):
    """What <prefix>.train.json holds: the schedule's position at a save and what the schedule depends on."""
    return {"version": STATE_VERSION, "epoch": int(epoch), "epoch_closed": bool(closed), "next": [int(r.next) for r in readers], "t": int(t),
            "batchsize": int(batchsize), "unbalanced": int(moptions.get('unbalanced') or 0), "test": _json_form(list(moptions['test'])),
            "files_digest": digest}


def write_json(path, obj):
    with open(path, 'w') as fh:
        json.dump(obj, fh, indent=1, sort_keys=True)
        fh.write('\n')


def read_schedule_state(prefix, n_readers, batchsize, moptions, digest):
    """<prefix>.train.json for --resume; refused in one line that names the difference when the file is missing or was written by another
    command line (batchsize, unbalanced, test, the file lists)."""
    path = prefix + ".train.json"
    if not os.path.isfile(path):
        raise SystemExit("Error: --resume: no state file %s (checkpoints written before the schedule kept its state cannot be resumed; "
                         "--startFrom takes their weights)" % path)
    with open(path) as fh:
        state = json.load(fh)
    if state.get("version") != STATE_VERSION:
        raise SystemExit("Error: --resume: %s has format version %r, this build reads version %d" % (path, state.get("version"), STATE_VERSION))
    now = schedule_state(0, False, [], 0, batchsize, moptions, digest)
    for key, flag in (("batchsize", "--batchsize"), ("unbalanced", "--unbalanced"), ("test", "--test")):
        if state.get(key) != now[key]:
            raise SystemExit("Error: --resume: %s differs: the checkpoint was written with %r, this command line gives %r" % (flag, state.get(key), now[key]))
    if state.get("files_digest") != digest:
        raise SystemExit("Error: --resume: the feature files under --wrkBase differ from those the checkpoint was trained on "
                         "(digest of the ordered file lists %s..., now %s...)" % (str(state.get("files_digest"))[:12], digest[:12]))
    if len(state.get("next", [])) != n_readers:
        raise SystemExit("Error: --resume: %s holds %d reader positions, --wrkBase gives %d groups" % (path, len(state.get("next", [])), n_readers))
    return state


def check_run_options(moptions):
    """The combinations of --resume / --startFrom / --validate that are refused, each in one line."""
    if moptions.get('resume') and moptions.get('startFrom'):
        raise SystemExit("Error: --resume and --startFrom exclude each other: one continues a run, the other starts a new one from a model's weights")
    if int(moptions.get('validate') or 0) < 0:
        raise SystemExit("Error: --validate must be non-negative (got %d)" % moptions['validate'])
    if int(moptions.get('validate') or 0) > 0 and moptions['test'][0] not in ('-', '0'):
        raise SystemExit("Error: --validate needs --test: without it no data is held out")


class HeldOut:
    """--validate K: at least K windows of the data --test holds out, on the device.  The files are predict.predict_files of every --wrkBase
    folder, taken one per folder in turn - whole files, until K windows are held - each through XYLoader.load under predict.loader_options and
    then appended to an xyload.XYSet.  score() is what `predict` computes for the same files: same kernels, same inputs per file."""

    def __init__(self, moptions, k, device: int = 0, initial_rows: int = 1 << 16):
        from . import predict, xyload
        self.device = device
        folders = wrkbase_folders(moptions)
        per_folder = [predict.predict_files(folder, moptions) for folder in folders]
        order = [files[i] for i in range(max([len(f) for f in per_folder] + [0])) for files in per_folder if i < len(files)]
        lopt = predict.loader_options(moptions)
        self.files, self.names, self.seg_names = [], [], []
        self.base = dict(files=0, fallback_files=0, rows=0, windows=0)
        self.set = xyload.XYSet(device, initial_rows)
        loader = xyload.XYLoader(device)
        try:
            for fn in order:
                if self.base['windows'] >= k:
                    break
                rows, n, fallback = loader.load(predict.read_text(fn), lopt, fn)
                self.files.append(fn)
                self.names.append(_relative(fn, folders))
                self.base['files'] += 1
                self.base['rows'] += rows
                self.base['fallback_files'] += int(fallback)
                if n < 1:
                    continue
                self.set.append(loader)
                self.seg_names.append(fn)
                self.base['windows'] += n
        finally:
            loader.close()
        self.seg_windows = [int(n) for n in self.set.segments()[1]]
        print("validate: %d windows of %d held-out files (%d rows) stay on the device: %d bytes" %
              (self.base['windows'], self.base['files'], self.base['rows'], self.set.nbytes()))
        sys.stdout.flush()

    def close(self):
        self.set.close()

    def score(self, w):
        """The held-out windows through a model of the weight blob w -> predict's stats."""
        from . import model as _model, predict
        model = _model.BiLSTMModel(unflatten_weights(w), self.device, precision=os.environ.get("DEEPMOD_PRECISION", "f16x3"))
        try:
            total, probs, labels = np.zeros(4, np.int64), [], []
            for seg, (fn, n) in enumerate(zip(self.seg_names, self.seg_windows)):
                prob1, cls, label = self.set.classify(model, seg, n)
                total += predict.piece_lines(cls, label, fn)[1]
                probs.append(prob1)
                labels.append(label)
            return predict.finish_stats(dict(self.base), total, probs, labels, model)
        finally:
            model.close()


def best_checkpoint(table):
    """The entry with the largest AUC; ties go to the earliest, an AUC of None ranks last."""
    best = None
    for entry in table:
        if best is None or (entry['auc'] is not None and (best['auc'] is None or entry['auc'] > best['auc'])):
            best = entry
    return best


def train_save_model(filelists, num_input, mhidden, timesteps, moptions, batchsize: int = batchsize, session_factory=None, resume=None,
                     start_from=None, validate: int = 0, resident: bool = False):
    """Four epochs over the file groups; filelists[0] leads.  One round of an epoch:
      * the leading group reads files until it has 25 * batchsize windows (or runs out) and cuts them into int(windows / batchsize) equal
        steps (np.array_split: batchsize .. 2 batchsize - 1 windows each); a round that cannot fill one step is skipped with a note;
      * every other group reads on from where it stopped, recycling its files, until it has batchsize windows per step, and is cut into as
        many steps; when the round has fewer than 20 steps a group is first cut back to 1.2 * batchsize windows per step;
      * step by step, every group's piece is one training step, in group order;
      * checkpoints: <outFolder><epoch - 1>.50/<FileID> when the round ends at half of the leading files, with one group also
        <outFolder><epoch - 1>0.1 ... 0.9, and <outFolder><epoch>/<FileID> after every epoch.
    A step larger than the trainer's tape makes the session grow it (TrainSession).  The progress line shows loss, accuracy, precision, recall
    and the exact ROC AUC (siteperf.roc_auc) of the round's first step of the last group, not tf.metrics.auc's 200-threshold figure.
    session_factory(init) -> a session-like object (tests record with it); it may bring its own `saver`.
    Every save also writes <prefix>.train.json (schedule_state; t counts the steps fed so far).  resume: a checkpoint prefix of an earlier run
    of the same command line - the schedule takes its position from the .train.json, the saver (restore_training, if it has one) the trainer's
    state from the bundle, and the run goes on: inside the epoch of a mid-epoch checkpoint, with the next epoch after an epoch's last, not at
    all after the run's last.  start_from: a bundle whose 14 variables replace the initial values; the schedule is the whole one.
    validate: HeldOut of that many windows, scored at every save of a GPU session (<prefix>.valid.json, <outFolder><FileID>_valid.json).
    resident: ResidentData holds every training file on the device from before the first step; the readers answer from its catalogue and a
    step's X is a SetWindows of window ids.  The schedule, and with it every checkpoint and .train.json, is the host-fed run's."""
    from . import model as _model
    check_run_options(dict(moptions, resume=resume, startFrom=start_from, validate=validate))
    if resident and session_factory is not None:
        raise SystemExit("Error: --resident needs the GPU session: it cannot run with a session_factory")
    graph_options = dict(moptions, max_batch=2 * batchsize - 1)
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        _model.mCreateSession(num_input, mhidden, timesteps, graph_options)
    tokens = (accuracy, X, Y, auc_op, mpre, mspf, init_l, mfpred)
    readers = [_GroupReader(files, moptions) for files in filelists]
    lead, others = readers[0], readers[1:]
    every = _progress_interval(len(lead.files))
    full_round = SUMPSIZE
    digest = filelists_digest(filelists, moptions)
    t, first_epoch, inside = 0, 1, False
    if resume is not None:
        state = read_schedule_state(resume, len(readers), batchsize, moptions, digest)
        for reader, position in zip(readers, state["next"]):
            if not 0 <= position <= len(reader.files):
                raise SystemExit("Error: --resume: reader position %d outside the %d files of its group" % (position, len(reader.files)))
            reader.next = position
        t, inside = state["t"], not state["epoch_closed"]
        first_epoch = state["epoch"] if inside else state["epoch"] + 1
        if first_epoch > TRAINING_STEPS:
            print("--resume %s: this is the last checkpoint of its run (epoch %d of %d closed): the run is complete, nothing is written" %
                  (resume, state["epoch"], TRAINING_STEPS))
            return tokens
        print("--resume %s: step count %d, going on %s epoch %d" % (resume, t, "inside" if inside else "with", first_epoch))
    if (resume is not None or start_from is not None) and 'seed' in moptions:
        print("Note: --seed %s is not used: the weights come from %s" % (moptions['seed'], resume or start_from))
    data = None
    if resident:
        data = ResidentData(filelists, moptions, int(moptions.get("device", 0)))
        for i, reader in enumerate(readers):
            readers[i] = _ResidentReader(reader.files, data.catalogue)
            readers[i].next = reader.next
        lead, others = readers[0], readers[1:]

    def windows(x):
        return x if data is None else SetWindows(data.set, x)

    sess = session_factory(init) if session_factory else _model.new_session(int(moptions.get("device", 0)))
    saver = getattr(sess, "saver", saver)
    held, table = None, []

    def save(folder, epoch, closed):
        os.makedirs(folder, exist_ok=True)
        prefix = folder + '/' + moptions['FileID']
        saver.save(sess, prefix)
        write_json(prefix + ".train.json", schedule_state(epoch, closed, readers, t, batchsize, moptions, digest))
        if held is not None:
            if saver.last_saved[1] != t:
                raise _lib.DeepModHipError("the trainer has made %d steps, the schedule has fed %d" % (saver.last_saved[1], t))
            stats = held.score(saver.last_saved[0])
            stats.update(checkpoint=os.path.relpath(prefix, moptions['outFolder']).replace(os.sep, "/"), t=t)
            write_json(prefix + ".valid.json", stats)
            table.append(stats)
            print("validate %s: t=%d windows=%d acc=%.4f p=%.4f r=%.4f AUC=%s" % (stats['checkpoint'], t, stats['windows'], stats['accuracy'],
                  stats['precision'], stats['recall'], "none" if stats['auc'] is None else "%.4f" % stats['auc']))
            sys.stdout.flush()

    started = time.time()
    try:
        sess.run(init)
        restore = getattr(saver, "restore_training", None)
        if restore is not None and resume is not None:
            restore(sess, resume, t, True)
        elif restore is not None and start_from is not None:
            restore(sess, start_from, 0, False)
        if validate > 0 and session_factory is None:
            held = HeldOut(moptions, validate, int(moptions.get("device", 0)))
        for epoch in range(first_epoch, TRAINING_STEPS + 1):
            print("epoch %d of %d" % (epoch, TRAINING_STEPS))
            sys.stdout.flush()
            if not inside:
                lead.next = 0
            inside = False
            shown_at = -1
            while not lead.exhausted():
                x0, y0 = lead.pool(batchsize * full_round, wrap=False)
                steps = len(y0) // batchsize
                if steps < 1:
                    print("Note: %d windows left in the leading group do not fill a step of %d: round skipped" % (len(y0), batchsize))
                    continue
                pieces = [(np.array_split(x0, steps), np.array_split(y0, steps))]
                for reader in others:
                    xk, yk = reader.pool(batchsize * steps, wrap=True)
                    cap = int(steps * batchsize * 1.2)
                    if steps < full_round * 0.8 and cap < len(yk):
                        xk, yk = xk[:cap], yk[:cap]
                    pieces.append((np.array_split(xk, steps), np.array_split(yk, steps)))
                report = lead.next + 1 - shown_at >= every
                if report:
                    px, py = pieces[min(3, len(pieces) - 1)]
                    sess.run(init_l)
                    loss, auc, acc, prec, rec = sess.run([loss_op, auc_op[1], accuracy, mpre[1], mspf[1]], feed_dict={X: windows(px[0]), Y: py[0]})
                    print("files %d/%d: loss=%.3f AUC=%.3f acc=%.3f p=%.3f r=%.3f (%d s)" %
                          (lead.next, len(lead.files), loss, auc, acc, prec, rec, time.time() - started))
                    sys.stdout.flush()
                    shown_at = (lead.next + 1) - ((lead.next + 1) % every)
                for i in range(steps):
                    for px, py in pieces:
                        sess.run([train_op, loss_op], feed_dict={X: windows(px[i]), Y: py[i]})
                        t += 1
                suffix = _mid_epoch_folder(int(lead.next * 100 / float(len(lead.files))), not others)
                if suffix is not None:
                    save(moptions['outFolder'] + str(epoch - 1) + suffix, epoch, False)
            save(moptions['outFolder'] + str(epoch), epoch, True)
        print("Training Finished!")
        if held is not None:
            best = best_checkpoint(table)
            for entry in table:
                print("%s %-24s t=%-8d acc=%.4f AUC=%s" % ("*" if entry is best else " ", entry['checkpoint'], entry['t'], entry['accuracy'],
                      "none" if entry['auc'] is None else "%.4f" % entry['auc']))
            if best is not None:
                print("best checkpoint by AUC on the held-out windows: %s" % best['checkpoint'])
            write_json(moptions['outFolder'] + moptions['FileID'] + '_valid.json',
                       dict(checkpoints=table, best=None if best is None else best['checkpoint'], held_out_files=held.names,
                            resident_bytes=held.set.nbytes()))
    finally:
        if held is not None:
            held.close()
        if data is not None:
            data.close()
        if hasattr(sess, "close"):
            sess.close()
    return tokens


def file_groups(moptions) -> List[List[str]]:
    """--wrkBase "a,b;c" -> one file list per group (';' separates groups, ',' the folders of a group), each shuffled by numpy's legacy
    generator seeded with 3 (one seeding, the groups in the order given), and the first largest group moved to the front."""
    groups = []
    for spec in moptions['wrkBase'].split(';'):
        files = []
        for folder in spec.split(','):
            if folder:
                files += getTFiles1(folder, moptions)
        groups.append(files)
    np.random.seed(3)
    for files in groups:
        np.random.shuffle(files)
    largest = max(range(len(groups)), key=lambda i: (len(groups[i]), -i))
    groups[0], groups[largest] = groups[largest], groups[0]
    return groups


def mMult_RNN_LSTM_train(moptions, batchsize: int = batchsize, session_factory=None):
    check_run_options(moptions)
    filelists = file_groups(moptions)
    if moptions.get('modfile') is not None:
        print("Note: --modfile %s is accepted and ignored: training always starts from a fresh initialisation" % (moptions['modfile'],))
    if len(filelists[0]) == 0:
        raise SystemExit("Error: no *.xy.gz feature file under --wrkBase %r" % (moptions['wrkBase'],))
    return train_save_model(filelists, moptions['fnum'], moptions['hidden'], moptions['windowsize'], moptions, batchsize=batchsize,
                            session_factory=session_factory, resume=moptions.get('resume'), start_from=moptions.get('startFrom'),
                            validate=int(moptions.get('validate') or 0), resident=bool(int(moptions.get('resident') or 0)))
