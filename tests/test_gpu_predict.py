"""`DeepMod.py predict` end to end on the GPU.  Reference: the chain np.loadtxt -> train.getDataFromFile_new / labelled_rows (the '+' branch of
myMultiBiRNN.py:327-328 for --test E) -> dm_predict_read_at on the host table -> numpy counts cut by mPred's piece rule (:398-412), on a
checkpoint the bundle writer wrote from the test weight set."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import ROOT, trained_like_weights
from deepmod_amd import model, predict, siteperf, tfbundle, train

pytestmark = pytest.mark.gpu


def feature_table(rows, start, labelled, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((rows, 10))
    t[:, 0] = start + np.arange(rows)
    t[np.arange(rows), 3 + rng.integers(0, 4, rows)] = 1.0
    t[:, 7] = np.clip(rng.normal(0.0, 1.2, rows), -5, 5)
    t[:, 8] = np.abs(rng.normal(0.25, 0.15, rows))
    t[:, 9] = rng.geometric(0.12, rows)
    lab = np.zeros(rows, bool)
    lab[10:rows - 10] = rng.random(rows - 20) < labelled
    positive = rng.random(rows) < 0.5
    t[lab & positive, 2] = 1.0
    t[lab & ~positive, 1] = 1.0
    return t


@pytest.fixture(scope="module")
def world(tmp_path_factory, gpu_device):
    base = tmp_path_factory.mktemp("predict")
    prefix = str(base / "ckpt" / "mod")
    os.makedirs(os.path.dirname(prefix))
    weights = trained_like_weights()
    tfbundle.write_bundle(prefix, weights)
    data = base / "xy"
    (data / "sub").mkdir(parents=True)
    big = feature_table(2300, 999000, 1.0, 1)                     # 2280 windows, positions across 1 Mb
    assert (big[:, 1:3].sum(axis=1) > 0).sum() >= 2049
    np.savetxt(str(data / "a_big.xy.gz"), big, fmt="%.3f")
    np.savetxt(str(data / "b_unlabelled.xy.gz"), feature_table(60, 5000, 0.0, 2), fmt="%.3f")
    np.savetxt(str(data / "sub" / "c_sub.xy.gz"), feature_table(300, 1999900, 0.4, 3), fmt="%.3f")
    spec = importlib.util.spec_from_file_location("dmcli_gpu_predict", os.path.join(ROOT, "bin", "DeepMod.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    m = model.BiLSTMModel(weights, gpu_device, precision=os.environ.get("DEEPMOD_PRECISION", "f16x3"))
    yield {"base": base, "data": data, "prefix": prefix, "cli": cli, "model": m}
    m.close()


def host_chain(m, files, test):
    """-> (text of _mpred.txt, [tp, fp, fn, tn], labels, probabilities of class 1, rows)"""
    mo = {"windowsize": 21, "test": test}
    lines, total, labs, probs, n_rows = [], np.zeros(4, np.int64), [], [], 0
    for fn in files:
        table = np.loadtxt(fn, dtype=np.float32, ndmin=2)
        n_rows += len(table)
        rows = train.labelled_rows(table, mo, fn)
        x, y, _ = train.getDataFromFile_new(fn, mo)
        assert len(y) == len(rows)
        if len(rows) == 0:
            continue
        assert np.array_equal(x, table[:, 3:][rows[:, None] + np.arange(-10, 11)[None, :]])
        prob, cls = m.predict_read_at(table[:, 3:], rows.astype(np.int32))
        label = (np.asarray(y)[:, 1] == 1).astype(np.uint8)
        ls, counts = predict.piece_lines(cls, label, fn)
        lines += ls
        total += counts
        labs.append(label)
        probs.append(prob[:, 1])
    return "".join(lines), total.tolist(), np.concatenate(labs), np.concatenate(probs), n_rows


def run_predict(world, capsys, name, *extra, folder=None):
    out = world["base"] / ("out_" + name)
    args = world["cli"].build_parser().parse_args(["predict", "--wrkBase", str(folder or world["data"]), "--modfile", world["prefix"], "--FileID", name,
                                                   "--outFolder", str(out), "--threads", "2", *extra])
    args.func(args)
    printed = capsys.readouterr().out
    stats = json.load(open(out / (name + "_mpred.json")))
    assert json.loads(printed.strip().splitlines()[-1]) == stats
    return open(out / (name + "_mpred.txt")).read(), stats, printed


def all_files(world):
    d = world["data"]
    return [str(d / "a_big.xy.gz"), str(d / "b_unlabelled.xy.gz"), str(d / "sub" / "c_sub.xy.gz")]


@pytest.mark.parametrize("name, extra, test, pick", [("all", (), ['N', '100'], slice(None)), ("region", ("--test", "E,1,2"), ['+', 1000000, 2000000], slice(None)),
                                                     ("files", ("--test", "P,50"), ['0', 0.5], slice(0, 2))])
def test_the_command_gives_the_lines_and_counts_of_the_host_chain(world, capsys, name, extra, test, pick):
    files = all_files(world)[pick]
    text, stats, _ = run_predict(world, capsys, name, *extra)
    want_text, want_counts, labels, probs, n_rows = host_chain(world["model"], files, test)
    capsys.readouterr()
    assert text == want_text and want_text.count("\n") >= (3 if name == "all" else 1)
    assert [stats[k] for k in ("tp", "fp", "fn", "tn")] == want_counts
    assert (stats["files"], stats["fallback_files"], stats["rows"], stats["windows"]) == (len(files), 0, n_rows, len(labels))
    assert stats["auc"] == siteperf.roc_auc(labels, probs)
    assert stats["accuracy"] == (want_counts[0] + want_counts[3]) / len(labels)
    assert stats["precision_mode"] == os.environ.get("DEEPMOD_PRECISION", "f16x3")
    if name == "region":
        assert 0 < len(labels) < 2280                                  # the region cuts through the first file


def test_a_file_with_a_nan_row_goes_through_the_host_loader(world, capsys):
    folder = world["base"] / "with_nan"
    folder.mkdir()
    t = feature_table(200, 7000, 0.6, 4)
    t[100, 8] = np.nan
    np.savetxt(str(folder / "n.xy.gz"), t, fmt="%.3f")
    np.savetxt(str(folder / "o.xy.gz"), feature_table(120, 9000, 0.5, 5), fmt="%.3f")
    files = [str(folder / "n.xy.gz"), str(folder / "o.xy.gz")]
    text, stats, printed = run_predict(world, capsys, "nan", folder=folder)
    want_text, want_counts, labels, probs, n_rows = host_chain(world["model"], files, ['N', '100'])
    assert "Warning: NaN in a window of %s" % files[0] in capsys.readouterr().out     # the chain's own loader says it too
    assert text == want_text and [stats[k] for k in ("tp", "fp", "fn", "tn")] == want_counts
    assert (stats["files"], stats["fallback_files"], stats["rows"], stats["windows"]) == (2, 1, n_rows, len(labels))
    assert "Warning: NaN in a window of %s" % files[0] in printed and "%s: line 101" % files[0] in printed
