"""GPU: `train --resume`, `--startFrom` and `--validate` (deepmod_amd/train.py, xyload.XYSet over dm_xyset_* of the C ABI) on the fixture folders
of tests/golden/train/ with --batchsize 8.  Every equality here is exact: a resumed run writes the bytes of the uninterrupted one, the resident
set gives the bytes of the loader, a validation pass gives the figures of `predict` on the same files."""
import contextlib
import importlib.util
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, trained_like_weights
from deepmod_amd import model, predict, tfbundle, train, xyload

pytestmark = pytest.mark.gpu

FIX = os.path.join(GOLDEN, "train")
NEG, POS = os.path.join(FIX, "neg"), os.path.join(FIX, "pos")
KINDS = (".index", ".data-00000-of-00001", ".train.json", ".valid.json")

spec = importlib.util.spec_from_file_location("dmcli_gpu_train_resume", os.path.join(ROOT, "bin", "DeepMod.py"))
cli = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cli)


# form -> (--wrkBase, --test, the same as moptions['test'], held-out windows, files read, files with windows, host-fallback files): the sets were
# computed on the CPU (train.getDataFromFile_new under predict.loader_options).  Under P,80 two GROUPS have no checkpoint inside an epoch (the
# leading group's six files fill one round), so the runs are one group of both folders.  The region form is not trained here (its run takes
# twice as long): its held-out set is scored with a checkpoint of the P,80 run.
FORMS = {"p80": (NEG + "," + POS, "P,80", ["0", 0.8], 164, 3, 3, 0),
         "p50": (NEG + "," + POS, "P,50", ["0", 0.5], 313, 6, 6, 2),
         "e12": (NEG + ";" + POS, "E,1,2", ["-", 10 ** 6, 2 * 10 ** 6], 34, 11, 2, 2)}       # every file is read; f02 and f09 hold a nan


def run_train(out, form, *extra):
    """bin/DeepMod.py train in this process -> (checkpoints in save order, what it printed)."""
    args = cli.build_parser().parse_args(["train", "--wrkBase", FORMS[form][0], "--FileID", "mod_train", "--outFolder", str(out), "--batchsize", "8",
                                          "--test", FORMS[form][1], "--validate", "1000", *extra])
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        args.func(args)
    saved = [line.split()[1].rstrip(":") for line in text.getvalue().splitlines() if line.startswith("validate ") and "/" in line.split()[1]]
    return saved, text.getvalue()


@pytest.fixture(scope="module")
def runs(tmp_path_factory, gpu_device):
    """Run A of a form, once: the full command with --seed 4."""
    base = tmp_path_factory.mktemp("resume")
    done = {}

    def get(form):
        if form not in done:
            folder = str(base / ("A_" + form)) + "/"
            saved, text = run_train(folder, form, "--seed", "4")
            done[form] = {"folder": folder, "saved": saved, "text": text, "base": base}
        return done[form]
    return get


def same_files(a, b, checkpoint):
    da, db = os.path.join(a, os.path.dirname(checkpoint)), os.path.join(b, os.path.dirname(checkpoint))
    assert sorted(os.listdir(da)) == sorted(os.listdir(db)) == sorted(["checkpoint"] + ["mod_train" + k for k in KINDS])
    for name in os.listdir(da):
        assert open(os.path.join(da, name), "rb").read() == open(os.path.join(db, name), "rb").read(), (checkpoint, name)


@pytest.mark.parametrize("form,checkpoint,first", [("p80", "1.50/mod_train", "2/mod_train"), ("p80", "2/mod_train", "2.50/mod_train"),
                                                   ("p50", "10.8/mod_train", "2/mod_train")])
def test_a_resumed_run_writes_the_bytes_of_the_uninterrupted_one(runs, form, checkpoint, first):
    a = runs(form)
    assert len(a["saved"]) == 8 and checkpoint in a["saved"] and "Training Finished!" in a["text"]
    out = str(a["base"] / ("B_%s_%s" % (form, checkpoint.split("/")[0]))) + "/"
    saved, text = run_train(out, form, "--resume", a["folder"] + checkpoint, "--seed", "9")
    rest = a["saved"][a["saved"].index(checkpoint) + 1:]
    assert saved == rest and rest[0] == first and rest[-1] == "4/mod_train"
    for ck in rest:
        same_files(a["folder"], out, ck)
    assert sorted(os.listdir(out)) == sorted({ck.split("/")[0] for ck in rest} | {"mod_train_valid.json"})       # nothing before the resume point
    assert "--seed 9 is not used" in text and "Training Finished!" in text
    summary = json.load(open(out + "mod_train_valid.json"))
    assert [e["checkpoint"] for e in summary["checkpoints"]] == rest


def test_resume_into_the_same_folder_rewrites_the_same_bytes(runs, tmp_path):
    import shutil
    a = runs("p50")
    copy = str(tmp_path / "again") + "/"
    shutil.copytree(a["folder"], copy)
    for ck in ("3/mod_train", "30.8/mod_train", "4/mod_train"):
        shutil.rmtree(os.path.join(copy, os.path.dirname(ck)))
    saved, _ = run_train(copy, "p50", "--resume", copy + "20.8/mod_train")
    assert saved == ["3/mod_train", "30.8/mod_train", "4/mod_train"]
    for ck in a["saved"]:
        same_files(a["folder"], copy, ck)


def bundle_blobs(prefix):
    back = tfbundle.load_bundle(prefix)
    return [train.flatten_weights({name: back[name + suffix] for name, _ in train.blob_names()}) for suffix in ("", "/Adam", "/Adam_1")]


def fresh_session(seed):
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        model.mCreateSession(7, 100, 21, {"outputlayer": "", "unbalanced": 0, "seed": seed, "max_batch": 15})
    return model.new_session(0), saver, (train_op, loss_op, X, Y)


def test_the_restored_state_is_the_checkpoints(runs, gpu_device):
    prefix = runs("p80")["folder"] + "1.50/mod_train"
    t = json.load(open(prefix + ".train.json"))["t"]
    w, m, v = bundle_blobs(prefix)
    assert t > 0 and m.any() and v.any()
    x, y, _ = train.getDataFromFile_new(os.path.join(POS, "f00.xy.gz"), {"test": ["N", "100"], "windowsize": 21})
    x, y = x[:13], np.asarray(y[:13], np.float32)
    sess, saver, (train_op, loss_op, X, Y) = fresh_session(1)
    try:
        saver.restore_training(sess, prefix, t, True)                          # --resume
        got = sess._train.trainer.get_state()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], (w, m, v))) and got[3] == t
        with pytest.raises(SystemExit) as exc:
            saver.restore_training(sess, prefix, t + 1, True)
        assert "beta1_power" in str(exc.value)
    finally:
        sess.close()
    sess, saver, (train_op, loss_op, X, Y) = fresh_session(2)
    ref = train.Trainer(w, device=gpu_device, max_batch=15)
    try:
        saver.restore_training(sess, prefix, 0, False)                         # --startFrom
        got = sess._train.trainer.get_state()
        assert got[0].tobytes() == w.tobytes() and not got[1].any() and not got[2].any() and got[3] == 0
        loss = sess.run([train_op, loss_op], feed_dict={X: x, Y: y})[1]
        assert np.float32(loss).tobytes() == np.float32(ref.step(x, y)).tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(sess._train.trainer.get_state()[:3], ref.get_state()[:3]))
    finally:
        sess.close()
        ref.close()


def test_start_from_runs_the_whole_schedule_from_the_models_weights(runs):
    a = runs("p50")
    out = str(a["base"] / "S_p50") + "/"
    saved, text = run_train(out, "p50", "--startFrom", a["folder"] + "4/mod_train", "--seed", "4")
    assert saved == a["saved"] and "--seed 4 is not used" in text
    for ck in saved:                                                           # the schedule is the full one, the weights are not run A's
        assert json.load(open(out + ck + ".train.json")) == json.load(open(a["folder"] + ck + ".train.json"))
    assert open(out + "00.8/mod_train.data-00000-of-00001", "rb").read() != open(a["folder"] + "00.8/mod_train.data-00000-of-00001", "rb").read()
    assert [e["t"] for e in json.load(open(out + "mod_train_valid.json"))["checkpoints"]] == \
        [e["t"] for e in json.load(open(a["folder"] + "mod_train_valid.json"))["checkpoints"]]


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_the_resident_set_gives_what_the_loader_gives(gpu_device, precision, capsys):
    region, half, everything = ["+", 10 ** 6, 2 * 10 ** 6], ["0", 0.5], ["N", "100"]
    cases = [(os.path.join(POS, "f01.xy.gz"), region, 16, False), (os.path.join(POS, "f00.xy.gz"), region, 0, False),
             (os.path.join(POS, "f02.xy.gz"), half, 50, True), (os.path.join(NEG, "f10.xy.gz"), everything, 52, False)]
    m = model.BiLSTMModel(trained_like_weights(), gpu_device, precision=precision)
    loader, resident = xyload.XYLoader(gpu_device), xyload.XYSet(gpu_device, initial_rows=32)
    try:
        want, rows_of, added = [], [], []
        for fn, test, n_want, fallback_want in cases:
            rows, n, fallback = loader.load(predict.read_text(fn), {"test": test, "windowsize": 21}, fn)
            assert (n, fallback) == (n_want, fallback_want) and rows > 32          # every table is larger than the first block: the set grows
            if n:
                want.append(loader.classify(m))
                rows_of.append(rows)
            added.append(resident.append(loader))
        assert added == [True, False, True, True]                                  # a file without a window adds no segment
        loader.close()                                                             # the set has its own copies
        seg_rows, seg_windows = resident.segments()
        assert seg_rows.tolist() == rows_of and seg_windows.tolist() == [16, 50, 52]
        assert resident.nbytes() == 28 * sum(rows_of) + 5 * (16 + 50 + 52)
        for again in range(2):
            for seg in (2, 0, 1):                                                  # in any order, any number of times
                got = resident.classify(m, seg)
                for a, b in zip(got, want[seg]):
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (seg, again)
        assert sum(int(w[2].sum()) for w in want) > 0 and sum(int((1 - w[2]).sum()) for w in want) > 0
        assert all(np.isfinite(w[0]).all() for w in want)
        with pytest.raises(Exception) as exc:
            resident.classify(m, 3, 1)
        assert "segment 3 of 3" in str(exc.value)
    finally:
        loader.close()
        resident.close()
        m.close()
    capsys.readouterr()


def predict_stats(prefix, files, test, pf):
    mo = {"test": list(test), "windowsize": 21, "threads": 2, "outputlayer": ""}
    model.mCreateSession(7, 100, 21, mo)
    with contextlib.redirect_stdout(io.StringIO()):
        return predict.mPred(prefix, os.path.dirname(prefix) + "/", None, None, None, [files], pf, 7, None, None, None, None, None, 21, mo)


def held_out(form, k):
    with contextlib.redirect_stdout(io.StringIO()):
        return train.HeldOut({"wrkBase": FORMS[form][0], "recursive": 1, "test": list(FORMS[form][2]), "windowsize": 21}, k, 0)


def rel(files):
    return [os.path.relpath(f, FIX).replace(os.sep, "/") for f in files]


@pytest.mark.parametrize("form", ["p80", "p50"])
def test_validation_at_every_checkpoint_is_what_predict_computes(runs, tmp_path, form):
    a = runs(form)
    _, _, test, windows, n_files, with_windows, fallback = FORMS[form]
    held = held_out(form, 1000)                                                    # the files of --validate 1000, in its order
    try:
        files, names = list(held.files), list(held.names)
        assert (held.base["windows"], held.base["files"], len(held.seg_windows), held.base["fallback_files"]) == (windows, n_files, with_windows, fallback)
        assert held.set.nbytes() == 28 * int(held.set.segments()[0].sum()) + 5 * windows
    finally:
        held.close()
    table = []
    for ck in a["saved"]:
        prefix = a["folder"] + ck
        got = json.load(open(prefix + ".valid.json"))
        want = predict_stats(prefix, files, test, str(tmp_path / "mpred.txt"))
        assert set(want) == {"files", "fallback_files", "rows", "windows", "tp", "fp", "fn", "tn", "accuracy", "precision", "recall", "auc", "precision_mode"}
        assert {k: got[k] for k in want} == json.loads(json.dumps(want)), ck
        assert set(got) == set(want) | {"checkpoint", "t"}
        assert got["checkpoint"] == ck and got["t"] == json.load(open(prefix + ".train.json"))["t"]
        assert (got["windows"], got["files"], got["fallback_files"]) == (windows, n_files, fallback)
        assert 0 < got["tp"] + got["fn"] < windows and got["auc"] is not None       # both labels present
        table.append(got)
    summary = json.load(open(a["folder"] + "mod_train_valid.json"))
    assert summary["checkpoints"] == table and len(table) == 8                     # this run's checkpoints in save order
    aucs = [e["auc"] for e in table]
    assert summary["best"] == a["saved"][int(np.argmax(aucs))]                     # np.argmax: the first of equal maxima
    assert summary["held_out_files"] == names and summary["resident_bytes"] > 0
    assert "best checkpoint by AUC on the held-out windows: " + summary["best"] in a["text"]


def test_a_held_out_region_scores_as_predict_does(runs, tmp_path):
    """--test E,1,2 over two groups: every file is read, two hold windows of the region; scored with the last checkpoint of the P,80 run."""
    _, _, test, windows, n_files, with_windows, fallback = FORMS["e12"]
    prefix = runs("p80")["folder"] + "4/mod_train"
    held = held_out("e12", 1000)
    try:
        assert (held.base["windows"], held.base["files"], len(held.seg_windows), held.base["fallback_files"]) == (windows, n_files, with_windows, fallback)
        assert held.set.nbytes() == 28 * int(held.set.segments()[0].sum()) + 5 * windows
        with contextlib.redirect_stdout(io.StringIO()):
            got = held.score(train.flatten_weights(tfbundle.load_bundle(prefix)))
        want = predict_stats(prefix, held.files, test, str(tmp_path / "mpred.txt"))
        assert got == want and 0 < got["tp"] + got["fn"] < windows and got["auc"] is not None       # both labels present
    finally:
        held.close()


def test_k_cuts_by_whole_files_one_per_folder_in_turn():
    for k, files in ((1, ["neg/f10.xy.gz"]), (52, ["neg/f10.xy.gz"]), (53, ["neg/f10.xy.gz", "pos/sub/f06.xy.gz"]), (60, ["neg/f10.xy.gz", "pos/sub/f06.xy.gz"]),
                     (119, ["neg/f10.xy.gz", "pos/sub/f06.xy.gz", "pos/sub/f07.xy.gz"])):
        held = held_out("p80", k)
        try:
            assert rel(held.files) == files, k
            assert held.names == [("0:" if f.startswith("neg/") else "1:") + f.split("/", 1)[1] for f in files]
            assert held.base["windows"] == sum({"neg/f10.xy.gz": 52, "pos/sub/f06.xy.gz": 66, "pos/sub/f07.xy.gz": 46}[f] for f in files)
        finally:
            held.close()
