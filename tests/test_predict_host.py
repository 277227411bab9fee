"""`DeepMod.py predict` without a GPU: which files it reads, the reference's piece rule and line format, and what the command refuses.
Reference: myMultiBiRNN.py - getTFiles1 (:233-251) for the file sets, mPred (:398-412) for the lines: tests/golden/predict/mpred.npz is a
recording of the reference's own mPred (tests/golden/make_golden_predict.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "bin", "DeepMod.py")

from deepmod_amd import predict, train  # noqa: E402


@pytest.mark.parametrize("pct", [0, 20, 50, 51, 80, 100])
@pytest.mark.parametrize("n_files", [0, 1, 2, 5, 7])
def test_test_P_reads_exactly_the_files_train_left_out(tmp_path, n_files, pct, capsys):
    for i in range(n_files):
        sub = tmp_path / ("sub" if i % 3 == 2 else "")
        sub.mkdir(exist_ok=True)
        (sub / ("f%02d.xy.gz" % i)).write_bytes(b"")
    mo = {"recursive": 1, "test": ['0', pct / 100.0]}
    everything = train.getTFiles1(str(tmp_path), dict(mo, test=['N', '100']))
    trained = train.getTFiles1(str(tmp_path), mo)
    scored = predict.predict_files(str(tmp_path), mo)
    assert len(everything) == n_files
    assert not set(trained) & set(scored)
    assert sorted(trained + scored) == sorted(everything)
    assert scored == [f for f in everything if f in set(scored)]          # getTFiles1's order
    assert predict.predict_files(str(tmp_path), dict(mo, test=['N', '100'])) == everything
    assert predict.predict_files(str(tmp_path), dict(mo, test=['-', 1000000, 2000000])) == everything


def test_test_E_selects_the_region_train_left_out():
    assert predict.loader_options({"test": ['-', 1000000, 2000000], "x": 1}) == {"test": ['+', 1000000, 2000000], "x": 1}
    assert predict.loader_options({"test": ['N', '100']})["test"] == ['N', '100']


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 4096])
def test_pieces_and_lines_are_the_reference_mpreds(n):
    z = np.load(os.path.join(GOLDEN, "predict", "mpred.npz"))
    cls, label = z["n%d|cls" % n], z["n%d|label" % n]
    assert len(cls) == n
    lines, total = predict.piece_lines(cls, (label[:, 1] == 1).astype(np.uint8), "FILE")
    assert "".join(lines) == str(z["n%d|lines" % n])
    assert len(lines) == int(n / 2048) + 1 and int(total.sum()) == n


def run_cli(*args):
    return subprocess.run([sys.executable, CLI, "predict", *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """A bundle of synthetic weights, written by the project's own writer."""
    from deepmod_amd import synth, tfbundle
    prefix = str(tmp_path_factory.mktemp("ckpt") / "mod")
    tfbundle.write_bundle(prefix, synth.synthetic_weights(seed=3))
    return prefix


@pytest.mark.parametrize("flag, value, words", [("--fnum", "53", "fnum=7 hidden=100 windowsize=21"), ("--hidden", "64", "fnum=7 hidden=100 windowsize=21"),
                                                ("--windowsize", "51", "fnum=7 hidden=100 windowsize=21"), ("--outputlayer", "sigmoid", "--outputlayer sigmoid")])
def test_the_command_refuses_another_geometry_and_the_sigmoid_head(tmp_path, checkpoint, flag, value, words):
    r = run_cli("--wrkBase", str(tmp_path), "--modfile", checkpoint, "--outFolder", str(tmp_path / "out"), flag, value)
    assert r.returncode != 0 and words in r.stderr and r.stderr.strip().count("\n") == 0, r.stderr


def test_the_command_refuses_a_missing_checkpoint(tmp_path):
    r = run_cli("--wrkBase", str(tmp_path), "--modfile", str(tmp_path / "nothing"), "--outFolder", str(tmp_path / "out"))
    assert r.returncode != 0 and "no TF checkpoint" in r.stderr and r.stderr.strip().count("\n") == 0, r.stderr


def test_the_command_refuses_to_run_without_a_gpu(tmp_path, checkpoint, monkeypatch):
    """The library reports no device: one line, nothing written, the model never created."""
    import importlib.util
    import types
    from deepmod_amd import _lib
    spec = importlib.util.spec_from_file_location('dmcli_predict', CLI)
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(dm_device_count=lambda: 0))
    monkeypatch.setattr(predict, "pred_entry", lambda mo: pytest.fail("pred_entry reached without a GPU"))
    out = tmp_path / "out"
    args = cli.build_parser().parse_args(["predict", "--wrkBase", str(tmp_path), "--modfile", checkpoint, "--outFolder", str(out)])
    with pytest.raises(SystemExit) as exc:
        args.func(args)
    assert "no gfx950 GPU visible" in str(exc.value) and "\n" not in str(exc.value)
    assert not out.exists()


def test_a_bad_test_value_is_refused(tmp_path, checkpoint):
    r = run_cli("--wrkBase", str(tmp_path), "--modfile", checkpoint, "--test", "Q,1")
    assert r.returncode != 0 and "Unknown option for test" in r.stderr
