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
"""
from __future__ import annotations

import ctypes
import glob
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
        """-> (loss, prob float32[n,2] or None, gradient blob float32[408402] or None); the state does not change."""
        x, y = self._xy(x, y)
        n = x.shape[0]
        loss = ctypes.c_float(0.0)
        prob = np.empty((n, 2), np.float32) if want_prob else None
        grad = np.empty(_lib.DM_WEIGHT_FLOATS, np.float32) if want_grad else None
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

    def save(self, sess: "TrainSession", prefix: str):
        w, m, v, t = sess.trainer.get_state()
        tfbundle.write_bundle(prefix, checkpoint_tensors(w, m, v, t))
        return prefix


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


class TrainSession:
    """The training side of model.Session (which creates one at the first fetch of a training token): run(init) creates the trainer from the
    seeded initial values, run([train_op, loss_op], feed) is one dm_trainer_step, a fetch without train_op is one dm_trainer_grad (loss,
    accuracy, precision, recall, AUC of that batch: the metrics are reset before every progress line, so they are the batch's own).  A
    batch larger than the tape makes the trainer grow, state kept."""

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
        x, y = np.asarray(feed_dict[g.X]), np.asarray(feed_dict[g.Y])
        self._fit(len(x))
        prob = None
        if any(f is g.train_op for f in flist):
            if any(f is not g.train_op and f is not g.loss_op for f in flist):
                raise ValueError("train_op can be fetched together with loss_op only")
            loss = self.trainer.step(x, y, g.unbalanced)
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


def train_save_model(filelists, num_input, mhidden, timesteps, moptions, batchsize: int = batchsize, session_factory=None):
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
    session_factory(init) -> a session-like object (tests record with it); it may bring its own `saver`."""
    from . import model as _model
    graph_options = dict(moptions, max_batch=2 * batchsize - 1)
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        _model.mCreateSession(num_input, mhidden, timesteps, graph_options)
    sess = session_factory(init) if session_factory else _model.new_session(int(moptions.get("device", 0)))
    saver = getattr(sess, "saver", saver)
    readers = [_GroupReader(files, moptions) for files in filelists]
    lead, others = readers[0], readers[1:]
    every = _progress_interval(len(lead.files))
    full_round = SUMPSIZE

    def save(folder):
        os.makedirs(folder, exist_ok=True)
        saver.save(sess, folder + '/' + moptions['FileID'])

    started = time.time()
    try:
        sess.run(init)
        for epoch in range(1, TRAINING_STEPS + 1):
            print("epoch %d of %d" % (epoch, TRAINING_STEPS))
            sys.stdout.flush()
            lead.next = 0
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
                    loss, auc, acc, prec, rec = sess.run([loss_op, auc_op[1], accuracy, mpre[1], mspf[1]], feed_dict={X: px[0], Y: py[0]})
                    print("files %d/%d: loss=%.3f AUC=%.3f acc=%.3f p=%.3f r=%.3f (%d s)" %
                          (lead.next, len(lead.files), loss, auc, acc, prec, rec, time.time() - started))
                    sys.stdout.flush()
                    shown_at = (lead.next + 1) - ((lead.next + 1) % every)
                for i in range(steps):
                    for px, py in pieces:
                        sess.run([train_op, loss_op], feed_dict={X: px[i], Y: py[i]})
                suffix = _mid_epoch_folder(int(lead.next * 100 / float(len(lead.files))), not others)
                if suffix is not None:
                    save(moptions['outFolder'] + str(epoch - 1) + suffix)
            save(moptions['outFolder'] + str(epoch))
        print("Training Finished!")
    finally:
        if hasattr(sess, "close"):
            sess.close()
    return (accuracy, X, Y, auc_op, mpre, mspf, init_l, mfpred)


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
    filelists = file_groups(moptions)
    if moptions.get('modfile') is not None:
        print("Note: --modfile %s is accepted and ignored: training always starts from a fresh initialisation" % (moptions['modfile'],))
    if len(filelists[0]) == 0:
        raise SystemExit("Error: no *.xy.gz feature file under --wrkBase %r" % (moptions['wrkBase'],))
    return train_save_model(filelists, moptions['fnum'], moptions['hidden'], moptions['windowsize'], moptions, batchsize=batchsize,
                            session_factory=session_factory)
