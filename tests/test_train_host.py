"""CPU: the host side of `train` (deepmod_amd/train.py, bin/DeepMod.py train) against recordings of the reference's own Python
(tests/golden/make_golden_train.py -> tests/golden/train/), and the teeth of the gradient oracle (tests/train_oracle.py): of the per-tensor rule, and
of the block rule with the conditions its GPU cases must meet."""
import contextlib
import importlib.util
import io
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from deepmod_amd import train

FIX = os.path.join(GOLDEN, "train")
TESTS = {"N": ["N", "100"], "E": ["-", 1 * 10 ** 6, 2 * 10 ** 6], "P": ["0", 63 / 100.0]}
RUNS = {"two_groups": ("neg;pos", "N"), "one_group": ("pos", "P")}

spec = importlib.util.spec_from_file_location('deepmod_cli_train', os.path.join(ROOT, 'bin', 'DeepMod.py'))
cli = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cli)


def test_loader_returns_what_the_reference_returns():
    z = np.load(os.path.join(FIX, "loader.npz"))
    keys = sorted({k.rsplit("|", 1)[0] for k in z.files})
    assert len(keys) == 3 * 11
    dropped_nan = excluded = 0
    for key in keys:
        tname, rel = key.split("|")
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            x, y, third = train.getDataFromFile_new(os.path.join(FIX, rel), {"test": list(TESTS[tname]), "windowsize": 21})
        assert third is None
        wx, wy = z[key + "|x"], z[key + "|y"]
        assert np.asarray(x).shape == wx.shape and np.asarray(y).shape == wy.shape, key
        assert np.array_equal(np.asarray(x, np.float32), wx) and np.array_equal(np.asarray(y, np.int64), wy), key
        assert np.asarray(x).dtype == np.float32 and len(wx) > 0
        assert out.getvalue().count("Warning: NaN in a window") in (0, 1)          # one warning per file
        dropped_nan += out.getvalue().count("Warning: NaN in a window")
        if tname == "E":
            excluded += len(z["N|" + rel + "|x"]) - len(wx)
    assert dropped_nan == 3 * 2 and excluded > 0                             # the fixtures do hold NaN windows and excluded positions


def test_edge_rows_are_refused_with_file_and_row(tmp_path):
    m = np.zeros((40, 10))
    m[:, 0] = np.arange(40)
    m[:, 3] = 1.0
    m[15, 2] = 1.0
    m[33, 1] = 1.0                       # 6 rows from the end: the reference fails in np.reshape
    fn = str(tmp_path / "edge.xy.gz")
    np.savetxt(fn, m, fmt="%.3f")
    with pytest.raises(ValueError) as exc:
        train.getDataFromFile_new(fn, {"test": ["N", "100"], "windowsize": 21})
    assert "edge.xy.gz" in str(exc.value) and "row 33" in str(exc.value)
    m[33, 1] = 0.0
    m[4, 1] = 1.0                        # and at the start
    np.savetxt(fn, m, fmt="%.3f")
    with pytest.raises(ValueError) as exc:
        train.getDataFromFile_new(fn, {"test": ["N", "100"], "windowsize": 21})
    assert "row 4" in str(exc.value)
    m[4, 1] = 0.0
    np.savetxt(fn, m, fmt="%.3f")
    x, y, _ = train.getDataFromFile_new(fn, {"test": ["N", "100"], "windowsize": 21})
    assert x.shape == (1, 21, 7) and y.tolist() == [[0, 1]]


class RecordingSession:
    """The stub session of the fixture generator, behind train_save_model's session_factory."""

    def __init__(self, log, saves, out_folder):
        self.log = log
        self.saver = type("S", (), {"save": staticmethod(lambda sess, path: saves.append(os.path.relpath(path, out_folder).replace(os.sep, "/")))})()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def run(self, fetches, feed_dict=None):
        if feed_dict is None:
            return None
        flist = list(fetches)
        if len(flist) == 2 and flist[0].name == "train_op" and flist[1].name == "loss_op":
            x = np.ascontiguousarray(next(v for k, v in feed_dict.items() if k.name == "X"), dtype=np.float32)
            y = np.asarray(next(v for k, v in feed_dict.items() if k.name == "Y"))
            self.log.append((len(x), zlib.crc32(x.tobytes()), int(y[:, 0].sum()), int(y[:, 1].sum())))
            return [None, 0.5]
        return [0.5] * len(flist)


@pytest.mark.parametrize("run", sorted(RUNS))
def test_schedule_feeds_and_saves_what_the_reference_does(run, tmp_path):
    z = np.load(os.path.join(FIX, "schedule.npz"))
    groups, tname = RUNS[run]
    out_folder = str(tmp_path) + "/"
    mo = {"wrkBase": ";".join(",".join(os.path.join(FIX, f) for f in g.split(",")) for g in groups.split(";")), "recursive": 1,
          "test": list(TESTS[tname]), "fnum": 7, "hidden": 100, "windowsize": 21, "outFolder": out_folder, "FileID": "mod_train", "modfile": None,
          "unbalanced": 0, "outputlayer": ""}
    with contextlib.redirect_stdout(io.StringIO()):
        lists = train.file_groups(dict(mo))
    assert [[os.path.relpath(f, FIX).replace(os.sep, "/") for f in fl] for fl in lists] == json.loads(str(z[run + "|filelists"]))
    log, saves = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        train.mMult_RNN_LSTM_train(dict(mo), batchsize=8, session_factory=lambda init: RecordingSession(log, saves, out_folder))
    want = z[run + "|steps"]
    assert len(log) == len(want) and len(want) > 100
    assert np.array_equal(np.array(log, dtype=np.int64), want)               # the same batches in the same order
    assert saves == [str(s) for s in z[run + "|saves"]]                      # saved to the same paths
    assert 8 <= want[:, 0].min() and want[:, 0].max() < 16                   # array_split: batchsize .. 2 batchsize - 1 windows per step
    for s in saves:
        assert os.path.isdir(os.path.join(out_folder, os.path.dirname(s)))


def test_getTFiles1_sorts_and_slices(tmp_path):
    for rel in ("b.xy.gz", "a.xy.gz", "s/d.xy.gz", "s/c.xy.gz", "s/t/e.xy.gz", "x.txt"):
        os.makedirs(os.path.dirname(str(tmp_path / rel)), exist_ok=True)
        open(str(tmp_path / rel), "w").close()

    def names(mo):
        with contextlib.redirect_stdout(io.StringIO()):
            return [os.path.relpath(f, str(tmp_path)) for f in train.getTFiles1(str(tmp_path), mo)]
    assert names({"recursive": 1, "test": ["N", "100"]}) == ["a.xy.gz", "b.xy.gz", "s/c.xy.gz", "s/d.xy.gz", "s/t/e.xy.gz"]
    assert names({"recursive": 0, "test": ["N", "100"]}) == ["a.xy.gz", "b.xy.gz"]
    assert names({"recursive": 1, "test": ["0", 0.8]}) == ["a.xy.gz", "b.xy.gz", "s/c.xy.gz", "s/d.xy.gz"]
    assert names({"recursive": 1, "test": ["0", 0.2]}) == ["s/t/e.xy.gz"]


def test_train_command_line():
    p = cli.build_parser()
    a = p.parse_args(['train', '--wrkBase', 'a,b;c'])
    for k, v in dict(fnum=7, hidden=100, windowsize=21, modfile=None, test=None, outputlayer='', unbalanced=0, seed=0, batchsize=2048, wrkBase2=None,
                     FileID='mod', outFolder='./mod_output', recursive=1).items():
        assert getattr(a, k) == v, k
    mo = cli.train_options(a)
    assert mo['test'] == ['N', '100'] and mo['outFolder'] == './mod_output/'
    assert cli.train_options(p.parse_args(['train', '--wrkBase', 'a', '--test', 'E,1,2']))['test'] == ['-', 1000000, 2000000]
    assert cli.train_options(p.parse_args(['train', '--wrkBase', 'a', '--test', 'P,63']))['test'] == ['0', 0.63]
    for bad in (['--test', 'X,1'], ['--test', 'E,1'], ['--fnum', '57'], ['--hidden', '50'], ['--windowsize', '51'], ['--outputlayer', 'sigmoid']):
        with pytest.raises(SystemExit) as exc:
            cli.train_options(p.parse_args(['train', '--wrkBase', 'a'] + bad))
        assert 'Error' in str(exc.value), bad
    with pytest.raises(SystemExit) as exc:
        cli.train_options(p.parse_args(['train', '--wrkBase', 'a', '--hidden', '50']))
    assert 'fnum=7 hidden=100 windowsize=21 only' in str(exc.value)          # the message detect's geometry refusal carries
    with pytest.raises(SystemExit) as exc:
        cli.train_options(p.parse_args(['train', '--wrkBase', 'a', '--outputlayer', 'sigmoid']))
    assert 'sigmoid is not used by any shipped model and is not built' in str(exc.value)
    with pytest.raises(SystemExit):
        p.parse_args(['train']).func(None)


def test_initial_values_and_checkpoint_names():
    w = train.initial_weights(0)
    assert [k for k, _ in train.blob_names()] == list(w)
    flat = train.flatten_weights(w)
    assert flat.size == 408402 and np.array_equal(train.flatten_weights(train.unflatten_weights(flat)), flat)
    for name, arr in w.items():
        if name.endswith("bias"):
            assert not arr.any()
        elif name.endswith("kernel"):
            a = np.sqrt(6.0 / sum(arr.shape))
            assert np.abs(arr).max() <= a and np.abs(arr).max() > 0.99 * a
        else:
            assert np.abs(arr).max() <= 2.0 and (arr.size < 100 or 0.8 < arr.std() < 0.95)       # N(0, 1) cut at 2 sigma: std 0.88
    assert not np.array_equal(train.initial_weights(1)["Variable"], w["Variable"])
    want = json.load(open(os.path.join(GOLDEN, "index_tables.json")))["rnn_conmodC_P100wd21_f7ne1u0_4"]["entries"]
    got = train.checkpoint_tensors(flat, flat * 0, flat * 0, 3)
    assert sorted(got) == sorted(want)
    for name, e in want.items():
        assert tuple(got[name].shape) == tuple(e["shape"]), name
    assert got["beta1_power"] == np.float32(0.9 ** 4) and got["beta2_power"] == np.float32(0.999 ** 4)


def test_the_gradient_oracle_has_teeth():
    """The float64 oracle with the forget bias omitted, or with the backward stack fed rows 0..10, must miss the float64 gradient of the right
    architecture by at least 100 times the acceptance bound R e32 + 2^-23 of tests/test_gpu_train.py - else that bound could not tell a wrong
    kernel from a right one.  Without the forget bias every tensor misses; the wrong rows reach the forward stack only through the shared head
    (its tensors move by ~4e-5 of their scale), so that variant is held on the backward stack and the head kernel, which it changes directly."""
    import re
    import train_oracle as oracle
    from deepmod_amd import model, synth
    R = float(re.search(r"^R = ([0-9.]+)$", open(os.path.join(ROOT, "tests", "test_gpu_train.py")).read(), re.M).group(1))
    flat = model.flatten_weights(synth.synthetic_weights(5, 1.0))
    n = 33
    x = synth.synthetic_windows(n, seed=1)
    y = np.eye(2, dtype=np.float32)[np.random.default_rng(2).integers(0, 2, n)]
    _, g64, _ = oracle.loss_and_grad(flat, x, y)
    _, g32, _ = oracle.loss_and_grad(flat, x, y, dtype=oracle.torch.float32)
    bound = {k: R * e + 2.0 ** -23 for k, e in oracle.tensor_errors(g32, g64).items()}
    _, g_nobias, _ = oracle.loss_and_grad(flat, x, y, forget_bias=0.0)
    _, g_rows, _ = oracle.loss_and_grad(flat, x, y, bw_rows=range(11))
    e_nobias, e_rows = oracle.tensor_errors(g_nobias, g64), oracle.tensor_errors(g_rows, g64)
    for k in bound:
        assert e_nobias[k] >= 100 * bound[k], k
    for k in bound:
        if k.startswith("bw") or k == "out/W":
            assert e_rows[k] >= 100 * bound[k], k


def test_a_round_that_cannot_fill_a_step_is_skipped(tmp_path):
    """Fewer windows than batchsize left in the leading group: the reference fails in np.array_split; here the round is skipped with a note and
    the epoch checkpoints are still written."""
    m = np.zeros((60, 10))
    m[:, 0] = np.arange(60)
    m[:, 3] = 1.0
    m[20:25, 2] = 1.0                    # 5 labelled rows
    os.makedirs(str(tmp_path / "g"))
    np.savetxt(str(tmp_path / "g" / "a.xy.gz"), m, fmt="%.3f")
    out_folder = str(tmp_path / "out") + "/"
    mo = {"wrkBase": str(tmp_path / "g"), "recursive": 1, "test": ["N", "100"], "fnum": 7, "hidden": 100, "windowsize": 21, "outFolder": out_folder,
          "FileID": "m", "modfile": None, "unbalanced": 0, "outputlayer": ""}
    log, saves, text = [], [], io.StringIO()
    with contextlib.redirect_stdout(text):
        train.mMult_RNN_LSTM_train(dict(mo), batchsize=8, session_factory=lambda init: RecordingSession(log, saves, out_folder))
    assert log == [] and saves == ["1/m", "2/m", "3/m", "4/m"] and text.getvalue().count("round skipped") == 4
    log, saves = [], []
    with contextlib.redirect_stdout(io.StringIO()):
        train.mMult_RNN_LSTM_train(dict(mo), batchsize=5, session_factory=lambda init: RecordingSession(log, saves, out_folder))
    assert [s[0] for s in log] == [5] * 4 and saves == ["1/m", "2/m", "3/m", "4/m"]


# ---------------------------------------------------------------------------------------------
# the block rule of tests/test_gpu_train.py, on the reference alone
# ---------------------------------------------------------------------------------------------
def _gpu_test_constant(name):
    import re
    return float(re.search(r"^%s = ([0-9.]+)$" % name, open(os.path.join(ROOT, "tests", "test_gpu_train.py")).read(), re.M).group(1))


def test_blocks_are_a_partition_of_the_blob():
    import train_oracle as oracle
    assert len(oracle.BLOCKS) == 195 and len({name for name, _, _ in oracle.BLOCKS}) == 195
    seen = np.zeros(oracle.NW, np.int64)
    spans = {name: (a, b) for name, a, b, _ in oracle.SLICES}
    for name, tensor, idx in oracle.BLOCKS:
        assert idx.ndim == 1 and idx.size > 0, name
        np.add.at(seen, idx, 1)
        a, b = spans[tensor]
        assert a <= idx.min() and idx.max() < b, name            # inside one tensor
    assert np.array_equal(seen, np.ones(oracle.NW, np.int64))    # every index once, the union is range(NW)
    sizes = {name: idx.size for name, _, idx in oracle.BLOCKS}
    assert sizes["fw0/kernel[length,i,u96-99]"] == 4 and sizes["bw0/kernel[recurrent,o,u0-95]"] == 9600 and sizes["fw2/kernel[input,j,u96-99]"] == 400
    assert sizes["bw1/bias[f,u0-95]"] == 96 and sizes["out/W[fw]"] == sizes["out/W[bw]"] == 200 and sizes["out/b"] == 2
    # a gate block holds that gate's columns: the forget-gate block of a bias is where BasicLSTMCell's kernel columns 200..299 land
    name, _, idx = next(b for b in oracle.BLOCKS if b[0] == "fw0/bias[f,u96-99]")
    assert idx.tolist() == [107 * 400 + 296 + i for i in range(4)]


def test_block_errors_resolve_what_tensor_errors_average_away():
    import train_oracle as oracle
    g64 = np.random.default_rng(0).standard_normal(oracle.NW)
    g = g64.copy()
    i = next(idx for name, _, idx in oracle.BLOCKS if name == "bw1/kernel[recurrent,o,u96-99]")[7]
    g[i] += 0.5
    eb, et = oracle.block_errors(g, g64), oracle.tensor_errors(g, g64)
    assert [k for k, v in eb.items() if v > 0] == ["bw1/kernel[recurrent,o,u96-99]"] and [k for k, v in et.items() if v > 0] == ["bw1/kernel"]
    assert eb["bw1/kernel[recurrent,o,u96-99]"] > et["bw1/kernel"]


@pytest.mark.parametrize("case", __import__("train_oracle").ALL_CASES, ids=__import__("train_oracle").case_id)
def test_every_gpu_gradient_case_resolves_every_block(case):
    """What the block rule of tests/test_gpu_train.py needs from a case, on the reference alone: no block of the float64 gradient is all zero and
    every block has a yardstick > 0 (the largest e32 of three float32 evaluations in three summation orders) - for all 195 blocks, none skipped
    or merged.  A case that fails this gets another seed or n."""
    import train_oracle as oracle
    ref = oracle.reference(case)
    a = np.abs(ref["g64"])
    assert np.isfinite(ref["l64"]) and np.isfinite(a).all()
    for name, _, idx in oracle.BLOCKS:
        assert a[idx].max() > 0, name
        assert 0 < ref["e32_blocks"][name] < np.inf, name
    assert ref["e32_prob"] > 0 or ref["p64"].shape[0] == 1
    assert ref["x"].shape[0] == ref["p64"].shape[0] == ref["p32"].shape[0]


def test_train_command_line_unbalanced_reaches_the_graph():
    p = cli.build_parser()
    for flag, want in (([], False), (["--unbalanced", "0"], False), (["--unbalanced", "1"], True)):
        mo = cli.train_options(p.parse_args(["train", "--wrkBase", "a"] + flag))
        assert train.TrainGraph(mo["fnum"], mo["hidden"], mo["windowsize"], mo).unbalanced is want, flag


TEETH = (  # (case, delta, the per-tensor rule accepts it)
    (("tail", 1), 1e-3, True),
    (("tail", 17), 5e-4, True),
    (("synth", "synthetic", 1, False), 1e-3, False),
)


@pytest.mark.parametrize("case,delta,accepted", TEETH, ids=lambda v: __import__("train_oracle").case_id(v) if isinstance(v, tuple) else str(v))
def test_the_block_rule_has_teeth_where_the_tensor_rule_has_none(case, delta, accepted):
    """Two wrong gradients a dW kernel could produce - the recurrent rows of fw0/kernel (one operand segment) and units 96..99 of the forget gate
    of bw2/kernel (the last, partial 16-unit tile) scaled by 1 + delta - stay inside the per-tensor bound R e32(T) + 2^-23 in every tensor and
    miss the block bound R_B e32*(B) + 2^-23 by at least 10 times in a block of the mutated rows or units.  On read-shaped windows the length row
    is 100 to 500 times the mutated blocks (the tensor rule accepts delta up to 1.5e-3 at n = 1, 1.7e-3 at n = 17).  On the synthetic n = 1 case
    it is 10 to 15 times, and the tensor rule accepts delta only up to 8e-5 and 4e-5: there delta = 1e-3 is rejected by both rules, by the
    block rule by the wider margin (fw0/kernel: 6.6e-5 against the tensor bound 5.2e-6; 1e-3 against a block bound of 6e-6)."""
    import train_oracle as oracle
    R, R_B, U = _gpu_test_constant("R"), _gpu_test_constant("R_B"), 2.0 ** -23
    ref = oracle.reference(case)
    g64 = ref["g64"]
    tensor_bound = {k: R * e + U for k, e in oracle.tensor_errors(ref["g32"].astype(np.float64), g64).items()}
    block_bound = {k: R_B * e + U for k, e in ref["e32_blocks"].items()}
    spans = {name: (a, b, shape) for name, a, b, shape in oracle.SLICES}
    mutants = {}
    a, b, shape = spans["fw0/kernel"]
    g = g64.copy()
    g[a:b].reshape(shape)[oracle.NFEAT:, :] *= 1.0 + delta
    mutants["fw0/kernel recurrent rows"] = (g, "fw0/kernel[recurrent")
    a, b, shape = spans["bw2/kernel"]
    g = g64.copy()
    g[a:b].reshape(shape)[:, 2 * oracle.HID + 96:3 * oracle.HID] *= 1.0 + delta
    mutants["bw2/kernel forget gate units 96..99"] = (g, "bw2/kernel[")
    for what, (g, prefix) in mutants.items():
        et, eb = oracle.tensor_errors(g, g64), oracle.block_errors(g, g64)
        worst = max((eb[k] / block_bound[k], k) for k in eb)
        worst_tensor = max(et[k] / tensor_bound[k] for k in et)
        print("%s %s delta=%g: tensor %.3g of its bound, worst block %s at %.3g times its bound" %
              (oracle.case_id(case), what, delta, worst_tensor, worst[1], worst[0]))
        assert [k for k, v in eb.items() if v > 0 and not k.startswith(prefix)] == []       # the mutation is where it was put
        if accepted:
            for k in et:
                assert et[k] <= tensor_bound[k], (what, k)          # today's rule accepts it
        else:
            assert worst_tensor < worst[0]
        assert worst[0] >= 10 and worst[1].startswith(prefix), (what, worst)
