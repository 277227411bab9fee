"""Golden vectors for the host side of `train`, produced by running the REFERENCE's own Python
(/root/reference/bin/DeepMod_scripts/myMultiBiRNN.py) in the build container with a stub `tensorflow` (not installed), as make_golden_host.py
does for detect.  `glob.glob` is patched to sorted order (the reference's file order is whatever the file system returns) and `batchsize` to 8,
so that a handful of small files walks every branch of the schedule.

Writes (plain data, tests/golden/train/):
  pos/*.xy.gz, pos/sub/*.xy.gz, neg/*.xy.gz   feature files in the reference's format: position | 2 labels | 7 features, np.savetxt('%.3f');
                    they include unlabelled rows, a NaN row inside windows, and positions inside the region --test E,1,2 leaves out
  loader.npz        what getDataFromFile_new returns for every file under --test N (none), E,1,2 and P,63
  schedule.npz      per run: the file lists after mMult_RNN_LSTM_train's shuffles, (n, CRC32 of the X bytes, column sums of Y) of every train_op
                    call, and the checkpoint paths saver.save was asked for.  Runs: two groups "neg;pos" (the larger group leads, the .50 folder),
                    one group "pos" under P,63 (the 80 % folder)

Run only here (needs /root/reference):  python tests/golden/make_golden_train.py
"""
from __future__ import annotations

import contextlib
import glob as _glob
import io
import json
import os
import sys
import tempfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "train")
BATCHSIZE = 8
TESTS = {"N": ["N", "100"], "E": ["-", 1 * 10 ** 6, 2 * 10 ** 6], "P": ["0", 63 / 100.0]}
RUNS = {"two_groups": ("neg;pos", "N"), "one_group": ("pos", "P")}


def write_fixture_files():
    rng = np.random.default_rng(20261018)
    layout = [("pos", 6, 1), ("pos/sub", 2, 1), ("neg", 3, 0)]
    k = 0
    for folder, count, label in layout:
        os.makedirs(os.path.join(OUT, folder), exist_ok=True)
        for i in range(count):
            rows = int(rng.integers(120, 170))
            m = np.zeros((rows, 10))
            # positions: most files far below the excluded region; two straddle its lower edge
            start = 999900 if (folder, i) in (("pos", 1), ("neg", 0)) else 10000 * (k + 1)
            m[:, 0] = start + np.arange(rows)
            base = rng.integers(0, 4, rows)
            m[np.arange(rows), 3 + base] = 1.0
            m[:, 7] = np.clip(rng.normal(0.0, 1.2, rows), -5, 5)
            m[:, 8] = np.abs(rng.normal(0.25, 0.15, rows))
            m[:, 9] = rng.geometric(0.12, rows)
            lab = rng.random(rows) < 0.45
            lab[:10] = lab[-10:] = False              # a labelled row closer than 10 rows to an edge makes the reference fail in np.reshape
            m[lab, 1 + label] = 1.0
            if label == 1:                            # a positive file also holds a few rows labelled negative
                other = lab & (rng.random(rows) < 0.1)
                m[other, 1], m[other, 2] = 1.0, 0.0
            if (folder, i) in (("pos", 2), ("neg", 1)):
                m[rows // 2, 8] = np.nan               # one NaN row: every window over it is dropped, one warning per file
            np.savetxt(os.path.join(OUT, folder, "f%02d.xy.gz" % k), m, fmt="%.3f")
            k += 1


def import_reference():
    tf = types.ModuleType("tensorflow")
    tf.constant = lambda *a, **k: None
    contrib = types.ModuleType("tensorflow.contrib")
    rnn = types.ModuleType("tensorflow.contrib.rnn")
    contrib.rnn = rnn
    tf.contrib = contrib
    sys.modules.update({"tensorflow": tf, "tensorflow.contrib": contrib, "tensorflow.contrib.rnn": rnn})
    sys.path.insert(0, "/root/reference/bin")
    from DeepMod_scripts import myMultiBiRNN
    return tf, myMultiBiRNN


class StubSession:
    def __init__(self, log):
        self.log = log

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def run(self, fetches, feed_dict=None):
        if feed_dict is None:
            return None
        if fetches == ["train_op", "loss_op"]:
            x = np.ascontiguousarray(feed_dict["X"], dtype=np.float32)
            y = np.asarray(feed_dict["Y"])
            self.log.append((len(x), zlib.crc32(x.tobytes()), int(y[:, 0].sum()), int(y[:, 1].sum())))
            return [None, 0.5]
        return [0.5] * len(fetches)


def relative(path, base):
    return os.path.relpath(path, base).replace(os.sep, "/")


def main():
    write_fixture_files()
    tf, ref = import_reference()
    ref.batchsize = BATCHSIZE
    real_glob = _glob.glob
    ref.glob.glob = lambda pattern: sorted(real_glob(pattern))
    quiet = io.StringIO()

    loader = {}
    files = sorted(real_glob(os.path.join(OUT, "*", "*.xy.gz")) + real_glob(os.path.join(OUT, "*", "*", "*.xy.gz")))
    for tname, test in TESTS.items():
        mo = {"test": list(test), "windowsize": 21}
        for fn in files:
            with contextlib.redirect_stdout(quiet):
                x, y, _ = ref.getDataFromFile_new(fn, mo)
            key = tname + "|" + relative(fn, OUT)
            loader[key + "|x"] = np.asarray(x, dtype=np.float32)
            loader[key + "|y"] = np.asarray(y, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "loader.npz"), **loader)

    schedule = {}
    for rname, (groups, tname) in RUNS.items():
        log, saves, lists = [], [], []
        tmp = tempfile.mkdtemp() + "/"
        ref.mCreateSession = lambda *a, **k: ("init", "init_l", "loss_op", "accuracy", "train_op", "X", "Y", saver, ("auc_v", "auc_u"), ("p_v", "p_u"),
                                              ("r_v", "r_u"), "mfpred")
        saver = types.SimpleNamespace(save=lambda sess, path: saves.append(relative(path, tmp)))
        tf.ConfigProto = lambda: types.SimpleNamespace(gpu_options=types.SimpleNamespace())
        tf.Session = lambda config=None: StubSession(log)
        real_tsm = ref.train_save_model

        def spy(filelists, *a, **k):
            lists.extend([[relative(f, OUT) for f in fl] for fl in filelists])
            return real_tsm(filelists, *a, **k)
        ref.train_save_model = spy
        mo = {"wrkBase": ";".join(",".join(os.path.join(OUT, f) for f in g.split(",")) for g in groups.split(";")), "recursive": 1,
              "test": list(TESTS[tname]), "fnum": 7, "hidden": 100, "windowsize": 21, "outFolder": tmp, "FileID": "mod_train", "modfile": None,
              "unbalanced": 0, "outputlayer": ""}
        with contextlib.redirect_stdout(quiet):
            ref.mMult_RNN_LSTM_train(mo)
        ref.train_save_model = real_tsm
        schedule[rname + "|steps"] = np.array(log, dtype=np.int64).reshape(-1, 4)
        schedule[rname + "|saves"] = np.array(saves)
        schedule[rname + "|filelists"] = np.array(json.dumps(lists))
        print(rname, "train_op calls", len(log), "saves", saves)
    np.savez_compressed(os.path.join(OUT, "schedule.npz"), **schedule)


if __name__ == "__main__":
    main()
