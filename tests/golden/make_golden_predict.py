"""Golden vectors for `predict`: the piece rule and the line format of the REFERENCE's own mPred
(bin/DeepMod_scripts/myMultiBiRNN.py:382-414), run under a stub `tensorflow` whose session returns a recorded class table, as
make_golden_train.py does for the trainer.

Writes tests/golden/predict/mpred.npz (plain data): per n in {1, 2047, 2048, 2049, 4096} windows of one file
  n<k>|cls    the classes the stub session returned, in window order (uint8)
  n<k>|label  labels.astype(int) of those windows, [n][2], as getDataFromFile_new returned them
  n<k>|lines  the text mPred wrote for the file, its path replaced by FILE

Needs the reference checkout at /root/reference:  python tests/golden/make_golden_predict.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "predict")
SIZES = (1, 2047, 2048, 2049, 4096)


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


def feature_file(path, n, rng):
    """n labelled rows (both classes) between 10 unlabelled rows at either end"""
    rows = n + 20
    m = np.zeros((rows, 10))
    m[:, 0] = 5000 + np.arange(rows)
    m[np.arange(rows), 3 + rng.integers(0, 4, rows)] = 1.0
    m[:, 7] = rng.normal(0.0, 1.0, rows)
    m[:, 8] = np.abs(rng.normal(0.25, 0.1, rows))
    m[:, 9] = rng.geometric(0.12, rows)
    positive = rng.random(n) < 0.4
    m[10:10 + n, 1] = ~positive
    m[10:10 + n, 2] = positive
    np.savetxt(path, m, fmt="%.3f")


class StubSession:
    def __init__(self, table, seen):
        self.table, self.seen, self.at = table, seen, 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def run(self, fetches, feed_dict=None):
        if feed_dict is None:
            return None
        k = len(feed_dict["X"])
        self.seen.append(np.asarray(feed_dict["Y"]))
        out = self.table[self.at:self.at + k]
        self.at += k
        return [out]


def main():
    os.makedirs(OUT, exist_ok=True)
    tf, ref = import_reference()
    assert ref.batchsize == 2048
    tf.ConfigProto = lambda: types.SimpleNamespace(gpu_options=types.SimpleNamespace())
    tf.train = types.SimpleNamespace(import_meta_graph=lambda path: types.SimpleNamespace(restore=lambda sess, ckpt: None), latest_checkpoint=lambda folder: folder)
    rng = np.random.default_rng(20261019)
    golden = {}
    tmp = tempfile.mkdtemp()
    for n in SIZES:
        fn = os.path.join(tmp, "n%d.xy.gz" % n)
        feature_file(fn, n, rng)
        table = (rng.random(n) < 0.45).astype(np.int64)
        seen = []
        tf.Session = lambda config=None: StubSession(table, seen)
        pf = os.path.join(tmp, "n%d_mpred.txt" % n)
        mo = {"test": ["N", "100"], "windowsize": 21}
        with contextlib.redirect_stdout(io.StringIO()):
            ref.mPred("m", "./", None, "X", "Y", [[fn]], pf, 7, None, None, None, "init_l", "mfpred", 21, mo)
        label = np.concatenate(seen)
        assert label.shape == (n, 2)
        golden["n%d|cls" % n] = table.astype(np.uint8)
        golden["n%d|label" % n] = label.astype(np.uint8)
        golden["n%d|lines" % n] = np.array(open(pf).read().replace(fn, "FILE"))
        print(n, "windows:", open(pf).read().count("\n"), "lines")
    np.savez_compressed(os.path.join(OUT, "mpred.npz"), **golden)


if __name__ == "__main__":
    main()
