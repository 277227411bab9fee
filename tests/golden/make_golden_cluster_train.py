"""Golden vectors for training the CpG-cluster model (deepmod_amd/cluster_train.py).  Runs only on the development machine, which holds the
reference; only the data it writes is committed.

1. tests/golden/cluster_train_case.npz: the reference's serialized TRAINING graph
   (train_deepmod/na12878_cluster_train_mod-keep_prob0.7-nb25-chr1/Cg.cov5.nb25.meta) evaluated through tools/graphdef_interp.py with the real
   weights (tests/golden/cluster_weights.npz), the two RandomUniform nodes replaced by recorded arrays: for n = 1 and n = 37 and keep_prob 0.7 and
   1.0 the arrays X, Y, u1, u2, keep_prob, output, Mean under the keys <name>_n<n>_kp<10 keep_prob>.  X is taken from cluster_case.npz, Y drawn in
   [0, 1] and rounded to 3 decimals.
2. tests/golden/cluster_truth_case.json: the reference's readBed (DeepMod_tools/hm_cluster_predict.py:20-41), that function alone compiled from
   the reference's file at generation time (the script around it imports TensorFlow), run on a small synthetic bedMethyl text: {'text', 'truth':
   [[chr, strand, pos, fraction], ...]}.

Run:  python tests/golden/make_golden_cluster_train.py
"""
import ast
import io
import json
import os
import sys
import tempfile
import time
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from graphdef_interp import GraphRunner, load_meta  # noqa: E402

REF = "/root/reference"
META = REF + "/train_deepmod/na12878_cluster_train_mod-keep_prob0.7-nb25-chr1/Cg.cov5.nb25.meta"
TOOL = REF + "/DeepMod_tools/hm_cluster_predict.py"
UNIFORM = {"dropout/random_uniform/RandomUniform": "u1", "dropout_1/random_uniform/RandomUniform": "u2"}


class TrainGraphRunner(GraphRunner):
    """GraphRunner + the ops of the loss (Transpose, Rank, Range, Square, Mean) and recorded arrays for the two RandomUniform nodes."""

    def __init__(self, nodes, variables, uniforms):
        super().__init__(nodes, variables)
        self.uniforms = uniforms

    def _eval(self, nd):
        ins = [i for i in nd.inputs if not i.startswith("^")]
        g = self._tensor
        if nd.op == "RandomUniform":
            u = np.asarray(self.uniforms[UNIFORM[nd.name]], np.float32)
            assert list(u.shape) == np.asarray(g(ins[0])).astype(int).tolist()
            return u
        if nd.op == "Rank":
            return np.int32(np.asarray(g(ins[0])).ndim)
        if nd.op == "Range":
            return np.arange(int(g(ins[0])), int(g(ins[1])), int(g(ins[2])), dtype=np.int32)
        if nd.op == "Sub" and nd.name.startswith("transpose"):           # integer arithmetic on the permutation
            return (np.asarray(g(ins[0])).astype(np.int32) - np.asarray(g(ins[1])).astype(np.int32)).astype(np.int32)
        if nd.op == "Transpose":
            return np.transpose(g(ins[0]), np.asarray(g(ins[1])).astype(int).tolist())
        if nd.op == "Square":
            x = g(ins[0]).astype(np.float32)
            return (x * x).astype(np.float32)
        if nd.op == "Mean":
            axes = tuple(np.asarray(g(ins[1])).astype(int).ravel().tolist())
            return np.mean(g(ins[0]).astype(np.float32), axis=axes, dtype=np.float32)
        return super()._eval(nd)


def graph_cases():
    nodes, _ = load_meta(META)
    weights = dict(np.load(os.path.join(HERE, "cluster_weights.npz")))
    xall = np.load(os.path.join(HERE, "cluster_case.npz"))["X"]
    rng = np.random.default_rng(20261019)
    out = {}
    for n in (1, 37):
        x = xall[100:100 + n].astype(np.float32)
        y = np.round(rng.random(n), 3).astype(np.float32)
        u1 = rng.random((n, 100), dtype=np.float32)
        u2 = rng.random((n, 20), dtype=np.float32)
        for kp in (0.7, 1.0):
            runner = TrainGraphRunner(nodes, weights, {"u1": u1, "u2": u2})
            output, mean = runner.run(["output:0", "Mean:0"], {"X": x, "Y": y, "keep_prob": np.float32(kp)})
            assert output.shape == (n, 1) and np.asarray(mean).shape == ()
            tag = "_n%d_kp%d" % (n, round(kp * 10))
            for name, val in (("X", x), ("Y", y), ("u1", u1), ("u2", u2), ("keep_prob", np.float32(kp)), ("output", output.astype(np.float32)),
                              ("Mean", np.float32(mean))):
                out[name + tag] = val
            print("n=%d keep_prob=%.1f Mean=%.6f output[0]=%.6f" % (n, kp, float(mean), float(output[0, 0])))
    np.savez_compressed(os.path.join(HERE, "cluster_train_case.npz"), **out)


BEDMETHYL = "\n".join([
    "track name=synthetic description=bisulfite",                                      # the first line is always skipped
    "chr1 100 101 . 12 + 100 101 0,255,0 12 83",
    "chr1 101 102 . 9 - 101 102 0,255,0 9 11",
    "short line",                                                                      # 20 characters or fewer: skipped
    "chr1 205 206 . 4 + 205 206 0,255,0 4 50",                                         # coverage 4: dropped
    "chr1 207 208 . 5 + 207 208 0,255,0 5 40",                                         # coverage 5: kept
    "chr1 100 101 . 30 + 100 101 0,255,0 30 7",                                        # a duplicate key: the later row wins
    "chr1 300 301 . 1000 - 300 301 255,0,0 1000 100",
    "chr2 100 101 . 8 + 100 101 0,255,0 8 0",
    "chr2\t150\t151\t.\t17\t-\t150\t151\t0,255,0\t17\t33",                             # tabs
    "",
]) + "\n"


def truth_case():
    tree = ast.parse(open(TOOL).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "readBed"]
    ns = {"defaultdict": defaultdict, "time": time, "sys": sys, "cov_thrd": 5}
    exec(compile(ast.Module(body=fn, type_ignores=[]), TOOL, "exec"), ns)
    with tempfile.NamedTemporaryFile("w", suffix=".bed", delete=False) as fh:
        fh.write(BEDMETHYL)
    stdout, sys.stdout = sys.stdout, io.StringIO()
    try:
        d = ns["readBed"](fh.name)
    finally:
        sys.stdout = stdout
        os.unlink(fh.name)
    rows = [[c, s, int(p), float(v)] for (c, s, p), v in d.items()]
    json.dump({"text": BEDMETHYL, "truth": rows}, open(os.path.join(HERE, "cluster_truth_case.json"), "w"), indent=1)
    print("readBed:", rows)


if __name__ == "__main__":
    graph_cases()
    truth_case()
