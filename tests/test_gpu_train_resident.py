"""GPU: `train --resident 1` (deepmod_amd/train.py, xyload.XYSet.gather, Trainer.step_set / grad_set over dm_xyset_gather and
dm_trainer_step_set / _grad_set of the C ABI, csrc/xygather.hip.inc).  Every comparison is exact: the gather gives the bytes of
train.getDataFromFile_new's windows, a step from the set the bytes of the host-fed step, a resident run the checkpoints of the host-fed run."""
import contextlib
import gzip
import importlib.util
import io
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, trained_like_weights
from deepmod_amd import _lib, model, train, xyload

pytestmark = pytest.mark.gpu

FIX = os.path.join(GOLDEN, "train")
NEG, POS = os.path.join(FIX, "neg"), os.path.join(FIX, "pos")
MO = {"test": ["N", "100"], "windowsize": 21}
KINDS = (".index", ".data-00000-of-00001", ".train.json")

spec = importlib.util.spec_from_file_location("dmcli_gpu_train_resident", os.path.join(ROOT, "bin", "DeepMod.py"))
cli = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cli)


def built_text(path, rows, labelled, seed):
    """A feature file of `rows` rows whose labelled rows are `labelled`, written with three decimals."""
    rng = np.random.default_rng(seed)
    table = np.zeros((rows, 10))
    table[:, 0] = 5000 + np.arange(rows)
    table[:, 3:] = rng.normal(0.0, 1.5, (rows, 7))
    for i, r in enumerate(labelled):
        table[r, 1 + i % 2] = 1.0
    text = io.BytesIO()
    np.savetxt(text, table, fmt='%.3f')
    with gzip.open(path, "wb") as fh:
        fh.write(text.getvalue())
    return path


@pytest.fixture(scope="module")
def resident(tmp_path_factory, gpu_device):
    """Five files in one set that had to grow, and what the host loader makes of them: (set, x [W,21,7], y [W,2], window prefix sums)."""
    tmp = tmp_path_factory.mktemp("resident_set")
    rows_b = 57
    files = [os.path.join(POS, "f00.xy.gz"), os.path.join(POS, "f02.xy.gz"),                      # f02 holds a nan: loaded on the host
             built_text(str(tmp / "a.xy.gz"), 21, [10], 1), os.path.join(NEG, "f08.xy.gz"),
             built_text(str(tmp / "b.xy.gz"), rows_b, [10, rows_b - 11], 2)]
    xyset, loader = xyload.XYSet(gpu_device, initial_rows=32), xyload.XYLoader(gpu_device)
    xs, ys, fallbacks = [], [], 0
    with contextlib.redirect_stdout(io.StringIO()):
        for fn in files:
            rows, n, fallback = loader.load(gzip.decompress(open(fn, "rb").read()), MO, fn)
            assert n > 0 and xyset.append(loader)
            fallbacks += int(fallback)
            x, y, _ = train.getDataFromFile_new(fn, MO)
            assert len(y) == n
            xs.append(x)
            ys.append(y)
    loader.close()
    assert fallbacks == 1 and [len(y) for y in ys][2] == 1 and [len(y) for y in ys][4] == 2
    rows, windows = xyset.segments()
    assert rows.sum() > 32 and windows.tolist() == [len(y) for y in ys]
    x = np.ascontiguousarray(np.concatenate(xs), dtype=np.float32)
    x.setflags(write=False)
    y = np.concatenate(ys).astype(np.float32)
    y.setflags(write=False)
    yield xyset, x, y, np.concatenate(([0], np.cumsum(windows)))
    xyset.close()


def crossing(total, length, stride, start):
    return (start + stride * np.arange(length, dtype=np.int64)) % total


def test_gather_gives_the_host_loaders_windows(resident):
    xyset, x, y, off = resident
    total = int(off[-1])
    every = np.arange(total, dtype=np.int64)
    edges = np.array([i for k in range(len(off) - 1) for i in (off[k], off[k + 1] - 1)], np.int64)
    lists = {"ascending": every, "reversed": every[::-1], "duplicates": np.array([3, 3, 0, total - 1, 3, total - 1, 0], np.int64),
             "one": np.array([off[2]], np.int64), "segment edges": edges}
    for length in (1, 15, 16, 17, 64, 65):
        lists["%d contiguous over a boundary" % length] = crossing(total, length, 1, int(off[1]) - length // 2)
        lists["%d strided over all segments" % length] = crossing(total, length, 11, int(off[3]) - 1)
    for name, ids in lists.items():
        got = xyset.gather(ids)
        assert got.shape == (len(ids), 21, 7) and got.dtype == np.float32, name
        assert got.tobytes() == x[ids].tobytes(), name
    assert xyset.gather(np.zeros(0, np.int64)).shape == (0, 21, 7)


INITIAL = None


def initial_state():
    global INITIAL
    if INITIAL is None:
        INITIAL = train.flatten_weights(trained_like_weights())
        INITIAL.setflags(write=False)
    return INITIAL


@pytest.mark.parametrize("n", [1, 15, 16, 17, 65])
def test_a_step_from_the_set_is_the_host_fed_step(resident, gpu_device, n):
    xyset, x, y, off = resident
    total = int(off[-1])
    w0, zero = initial_state(), np.zeros(_lib.DM_WEIGHT_FLOATS, np.float32)
    a, b = train.Trainer(w0, gpu_device, max_batch=65), train.Trainer(w0, gpu_device, max_batch=65)
    try:
        for unbalanced in (False, True):
            a.set_state(w0, zero, zero, 0)
            b.set_state(w0, zero, zero, 0)
            for k in range(3):
                ids = crossing(total, n, 13, int(off[1 + k]) - 1)
                la = a.step(x[ids], y[ids], unbalanced)
                lb = b.step_set(xyset, ids, y[ids], unbalanced)
                assert np.float32(la).tobytes() == np.float32(lb).tobytes(), (unbalanced, k)
                sa, sb = a.get_state(), b.get_state()
                assert sa[3] == sb[3] == k + 1
                assert all(p.tobytes() == q.tobytes() for p, q in zip(sa[:3], sb[:3])), (unbalanced, k)
        ids = crossing(total, n, 7, int(off[2]))
        ga, gb = a.grad(x[ids], y[ids], True), b.grad_set(xyset, ids, y[ids], True)
        assert np.float32(ga[0]).tobytes() == np.float32(gb[0]).tobytes() and ga[1].tobytes() == gb[1].tobytes() and ga[2].tobytes() == gb[2].tobytes()
        assert gb[1].shape == (n, 2) and gb[2].any()
        assert all(p.tobytes() == q.tobytes() for p, q in zip(a.get_state()[:3], b.get_state()[:3]))          # grad leaves the state alone
    finally:
        a.close()
        b.close()


def test_a_session_fed_from_the_set_grows_its_trainer_and_goes_on(resident, gpu_device):
    xyset, x, y, off = resident
    total = int(off[-1])
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        model.mCreateSession(7, 100, 21, {"outputlayer": "", "unbalanced": 0, "seed": 6, "max_batch": 15})
    sess = model.new_session(gpu_device)
    ref = train.Trainer(train.initial_weights(6), gpu_device, max_batch=32)
    try:
        for k, n in enumerate((8, 20, 9)):                             # the second step is larger than the tape of 15
            ids = crossing(total, n, 5, int(off[1]) - 3 + k)
            loss = sess.run([train_op, loss_op], feed_dict={X: train.SetWindows(xyset, ids), Y: y[ids]})[1]
            assert np.float32(loss).tobytes() == np.float32(ref.step(x[ids], y[ids])).tobytes(), n
            assert sess._train.trainer.max_batch >= n
            assert all(p.tobytes() == q.tobytes() for p, q in zip(sess._train.trainer.get_state()[:3], ref.get_state()[:3])), n
        assert sess._train.trainer.max_batch > 15
        ids = crossing(total, 12, 3, 0)
        got = sess.run([loss_op, accuracy], feed_dict={X: train.SetWindows(xyset, ids), Y: y[ids]})
        want = ref.grad(x[ids], y[ids], want_grad=False)
        assert np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes()
        assert got[1] == np.float32((np.argmax(want[1], 1) == np.argmax(y[ids], 1)).mean())
    finally:
        sess.close()
        ref.close()


def test_ids_outside_the_set_and_batches_beyond_the_tape_are_refused(resident, gpu_device):
    xyset, x, y, off = resident
    total = int(off[-1])
    tr = train.Trainer(initial_state(), gpu_device, max_batch=16)
    try:
        tr.step_set(xyset, np.arange(5), y[:5])
        before = tr.get_state()
        for bad, at in ((-1, 3), (total, 0), (total + 7, 8)):
            ids = np.arange(9, dtype=np.int64)
            ids[at] = bad
            for call in (lambda: tr.step_set(xyset, ids, y[:9]), lambda: tr.grad_set(xyset, ids, y[:9]), lambda: xyset.gather(ids)):
                with pytest.raises(_lib.DeepModHipError) as exc:
                    call()
                assert exc.value.code == _lib.DM_EINVAL and "id %d at position %d" % (bad, at) in str(exc.value), str(exc.value)
                assert "\n" not in str(exc.value)
        ids = np.array([4, -2, total, 1], np.int64)                    # the first offender is the one named
        with pytest.raises(_lib.DeepModHipError) as exc:
            tr.step_set(xyset, ids, y[:4])
        assert "id -2 at position 1" in str(exc.value)
        with pytest.raises(_lib.DeepModHipError) as exc:
            tr.step_set(xyset, np.arange(17), y[:17])
        assert exc.value.code == _lib.DM_EINVAL and "max_batch" in str(exc.value)
        lib = _lib.load()
        loss = np.zeros(1, np.float32)
        assert lib.dm_trainer_step_set(None, xyset._h, ids.ctypes.data, y.ctypes.data, 1, 0, None) == _lib.DM_EINVAL
        assert lib.dm_trainer_step_set(tr._h, None, ids.ctypes.data, y.ctypes.data, 1, 0, None) == _lib.DM_EINVAL
        assert lib.dm_xyset_gather(None, ids.ctypes.data, 1, loss.ctypes.data) == _lib.DM_EINVAL
        after = tr.get_state()
        assert after[3] == before[3] == 1 and all(p.tobytes() == q.tobytes() for p, q in zip(before[:3], after[:3]))
        good = np.arange(9, dtype=np.int64)                            # and the trainer goes on as if nothing had been asked
        ref = train.Trainer(initial_state(), gpu_device, max_batch=16)
        try:
            ref.step(x[:5], y[:5])
            assert np.float32(ref.step(x[good], y[good])).tobytes() == np.float32(tr.step_set(xyset, good, y[good])).tobytes()
        finally:
            ref.close()
    finally:
        tr.close()


# ---- the command ---------------------------------------------------------------------------------------------------------------
FORMS = {"one_group_p50": (NEG + "," + POS, ["--test", "P,50", "--validate", "1000"]),        # f02 and f09 (nan) are loaded on the host
         "two_groups": (NEG + ";" + POS, [])}                                                     # recycling and the 1.2x cut


def run_train(out, form, *extra):
    args = cli.build_parser().parse_args(["train", "--wrkBase", FORMS[form][0], "--FileID", "mod_train", "--outFolder", str(out), "--batchsize", "8",
                                          *FORMS[form][1], *extra])
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        args.func(args)
    return text.getvalue()


def checkpoints(folder):
    return sorted(d for d in os.listdir(folder) if os.path.isfile(os.path.join(folder, d, "mod_train.index")))


@pytest.fixture(scope="module")
def runs(tmp_path_factory, gpu_device):
    """form -> the host-fed run and the resident run of the same command line, each once."""
    base = tmp_path_factory.mktemp("resident_runs")
    done = {}

    def get(form):
        if form not in done:
            host, res = str(base / ("host_" + form)) + "/", str(base / ("resident_" + form)) + "/"
            done[form] = dict(base=base, host=host, resident=res, host_text=run_train(host, form, "--seed", "4"),
                              resident_text=run_train(res, form, "--seed", "4", "--resident", "1", "--threads", "2"))
        return done[form]
    return get


def same_checkpoint(a, b, ck, valid):
    kinds = KINDS + ((".valid.json",) if valid else ())
    da, db = os.path.join(a, ck), os.path.join(b, ck)
    assert sorted(os.listdir(da)) == sorted(os.listdir(db)) == sorted(["checkpoint"] + ["mod_train" + k for k in kinds]), ck
    for name in os.listdir(da):
        assert open(os.path.join(da, name), "rb").read() == open(os.path.join(db, name), "rb").read(), (ck, name)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_a_resident_run_writes_the_checkpoints_of_the_host_fed_run(runs, form):
    r = runs(form)
    assert "Training Finished!" in r["host_text"] and "Training Finished!" in r["resident_text"]
    assert "resident:" not in r["host_text"]
    line = [ln for ln in r["resident_text"].splitlines() if ln.startswith("resident: ")]
    assert len(line) == 1 and " files, " in line[0] and " windows stay on the device: " in line[0] and " bytes (" in line[0]
    if form == "one_group_p50":
        assert r["resident_text"].count("is loaded on the host") >= 2
    saved = checkpoints(r["host"])
    assert saved == checkpoints(r["resident"]) and "4" in saved and len(saved) >= 4
    for ck in saved:
        same_checkpoint(r["host"], r["resident"], ck, valid=form == "one_group_p50")
    assert sorted(os.listdir(r["host"])) == sorted(os.listdir(r["resident"]))
    if form == "one_group_p50":
        assert open(r["host"] + "mod_train_valid.json", "rb").read() == open(r["resident"] + "mod_train_valid.json", "rb").read()


def test_a_host_fed_run_resumed_resident_writes_the_uninterrupted_bytes(runs):
    r = runs("one_group_p50")
    saved = [line.split()[1].rstrip(":") for line in r["host_text"].splitlines() if line.startswith("validate ") and "/" in line.split()[1]]
    mid = "10.8/mod_train"
    assert mid in saved and not json.load(open(r["host"] + mid + ".train.json"))["epoch_closed"]
    out = str(r["base"] / "resumed_resident") + "/"
    text = run_train(out, "one_group_p50", "--resume", r["host"] + mid, "--resident", "1")
    rest = [os.path.dirname(ck) for ck in saved[saved.index(mid) + 1:]]
    assert "Training Finished!" in text and len(rest) >= 3 and checkpoints(out) == sorted(rest)
    for ck in rest:
        same_checkpoint(r["host"], out, ck, valid=True)


def test_a_budget_the_files_pass_ends_the_run_before_its_first_step(tmp_path, monkeypatch, gpu_device):
    monkeypatch.setenv("DEEPMOD_RESIDENT_BYTES", "1000")
    out = str(tmp_path / "over_budget") + "/"
    with pytest.raises(SystemExit) as exc:
        run_train(out, "two_groups", "--resident", "1")
    message = str(exc.value)
    assert "\n" not in message and "--resident" in message and "1000" in message and ".xy.gz" in message and "bytes held" in message
    assert not os.path.isdir(out) or os.listdir(out) == []           # no checkpoint folder
