"""CPU: the schedule's state beside every checkpoint (<prefix>.train.json), `train --resume`, `--startFrom` and the refusals of `--validate`
(deepmod_amd/train.py, bin/DeepMod.py train), on the recorded schedules of tests/golden/train/ with a recording session: a resumed schedule
feeds exactly the steps the uninterrupted one feeds after the checkpoint, and saves exactly its remaining checkpoints."""
import contextlib
import importlib.util
import io
import json
import os
import shutil
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from deepmod_amd import tfbundle, train

FIX = os.path.join(GOLDEN, "train")
TESTS = {"N": ["N", "100"], "E": ["-", 1 * 10 ** 6, 2 * 10 ** 6], "P": ["0", 63 / 100.0]}
RUNS = {"two_groups": ("neg;pos", "N"), "one_group": ("pos", "P")}

spec = importlib.util.spec_from_file_location('deepmod_cli_train_resume', os.path.join(ROOT, 'bin', 'DeepMod.py'))
cli = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cli)


class RecordingSession:
    """The stub session of tests/test_train_host.py, with a saver that also records what it is asked to restore and how many steps had been
    logged at every save."""

    def __init__(self, log, saves, out_folder, restores=None, steps_at_save=None):
        self.log = log

        def save(sess, path):
            saves.append(os.path.relpath(path, out_folder).replace(os.sep, "/"))
            if steps_at_save is not None:
                steps_at_save.append(len(log))

        members = {"save": staticmethod(save)}
        if restores is not None:
            members["restore_training"] = staticmethod(lambda sess, prefix, t, slots: restores.append((prefix, t, slots)))
        self.saver = type("S", (), members)()

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


def options(run, out_folder, base=FIX, **more):
    groups, tname = RUNS[run]
    mo = {"wrkBase": ";".join(",".join(os.path.join(base, f) for f in g.split(",")) for g in groups.split(";")), "recursive": 1,
          "test": list(TESTS[tname]), "fnum": 7, "hidden": 100, "windowsize": 21, "outFolder": out_folder, "FileID": "mod_train", "modfile": None,
          "unbalanced": 0, "outputlayer": ""}
    mo.update(more)
    return mo


def record(mo, batchsize=8, with_restore=True):
    log, saves, restores, at_save, text = [], [], [], [], io.StringIO()
    with contextlib.redirect_stdout(text):
        train.mMult_RNN_LSTM_train(dict(mo), batchsize=batchsize, session_factory=lambda init: RecordingSession(
            log, saves, mo["outFolder"], restores if with_restore else None, at_save))
    return dict(log=log, saves=saves, restores=restores, at_save=at_save, text=text.getvalue())


@pytest.fixture(scope="module")
def full_runs(tmp_path_factory):
    """The uninterrupted runs, once: run -> (out folder, recording)."""
    out = {}
    for run in RUNS:
        folder = str(tmp_path_factory.mktemp("full_" + run)) + "/"
        out[run] = (folder, record(options(run, folder)))
    return out


@pytest.mark.parametrize("run", sorted(RUNS))
def test_every_save_leaves_the_schedule_state(run, full_runs):
    z = np.load(os.path.join(FIX, "schedule.npz"))
    folder, rec = full_runs[run]
    assert rec["saves"] == [str(s) for s in z[run + "|saves"]] and len(rec["saves"]) == 8
    assert np.array_equal(np.array(rec["log"], dtype=np.int64), z[run + "|steps"])           # the new file changes nothing that is fed
    with contextlib.redirect_stdout(io.StringIO()):
        lists = train.file_groups(options(run, folder))
    digest = train.filelists_digest(lists, options(run, folder))
    last_t = -1
    for save, steps_before in zip(rec["saves"], rec["at_save"]):
        state = json.load(open(os.path.join(folder, save + ".train.json")))
        assert state["version"] == train.STATE_VERSION
        assert state["t"] == steps_before and state["t"] > last_t                             # the schedule's own count of the steps fed
        last_t = state["t"]
        name = save.split("/")[0]
        closed = name in ("1", "2", "3", "4")
        assert state["epoch_closed"] is closed
        assert state["epoch"] == (int(name) if closed else int(name[0]) + 1)
        assert len(state["next"]) == len(lists)
        for position, files in zip(state["next"], lists):
            assert 0 <= position <= len(files)
        assert (state["next"][0] == len(lists[0])) is closed                                  # an epoch ends when the leading group is read
        assert state["batchsize"] == 8 and state["unbalanced"] == 0
        assert state["test"] == json.loads(json.dumps(TESTS[RUNS[run][1]]))
        assert state["files_digest"] == digest
    assert last_t == len(rec["log"])
    assert sorted(os.listdir(os.path.join(folder, "4"))) == ["mod_train.train.json"]          # the recording saver writes nothing itself


def test_the_digest_is_of_relative_paths_in_order(tmp_path):
    """The same files under another base folder give the same digest; another order or a missing file does not."""
    copy = str(tmp_path / "moved")
    shutil.copytree(FIX, copy)
    with contextlib.redirect_stdout(io.StringIO()):
        here = train.file_groups(options("two_groups", "x/"))
        there = train.file_groups(options("two_groups", "x/", base=copy))
    d = train.filelists_digest(here, options("two_groups", "x/"))
    assert d == train.filelists_digest(there, options("two_groups", "x/", base=copy)) and len(d) == 64
    assert d != train.filelists_digest([here[0][::-1], here[1]], options("two_groups", "x/"))
    assert d != train.filelists_digest([here[0][:-1], here[1]], options("two_groups", "x/"))
    assert d != train.filelists_digest([here[1], here[0]], options("two_groups", "x/"))


@pytest.mark.parametrize("run,checkpoint", [("two_groups", "1.50/mod_train"), ("two_groups", "2/mod_train"), ("one_group", "10.8/mod_train"),
                                            ("one_group", "2/mod_train")])
def test_a_resumed_schedule_feeds_and_saves_the_rest(run, checkpoint, full_runs, tmp_path):
    folder, full = full_runs[run]
    at = full["saves"].index(checkpoint)
    t = full["at_save"][at]
    assert 0 < t < len(full["log"])
    out_folder = str(tmp_path) + "/"
    rec = record(options(run, out_folder, resume=folder + checkpoint, seed=4))
    assert rec["log"] == full["log"][t:]                                                      # size, CRC32 and label sums of every later step
    assert rec["saves"] == full["saves"][at + 1:]
    assert rec["restores"] == [(folder + checkpoint, t, True)]
    assert "--seed 4 is not used" in rec["text"]
    for save in rec["saves"]:                                                                 # and the states written on the way are the full run's
        assert open(os.path.join(out_folder, save + ".train.json"), "rb").read() == open(os.path.join(folder, save + ".train.json"), "rb").read()
    # a session whose saver cannot restore (tests/test_train_host.py's) still resumes the schedule
    again = record(options(run, out_folder, resume=folder + checkpoint), with_restore=False)
    assert again["log"] == rec["log"] and again["saves"] == rec["saves"]


@pytest.mark.parametrize("run", sorted(RUNS))
def test_resuming_the_last_checkpoint_does_nothing(run, full_runs, tmp_path):
    folder, _ = full_runs[run]
    out_folder = str(tmp_path / "out") + "/"
    rec = record(options(run, out_folder, resume=folder + "4/mod_train"))
    assert rec["log"] == [] and rec["saves"] == [] and rec["restores"] == []
    assert "the run is complete" in rec["text"] and not os.path.exists(out_folder)


def refusal(mo, batchsize=8):
    with pytest.raises(SystemExit) as exc:
        record(mo, batchsize=batchsize)
    message = str(exc.value)
    assert message.startswith("Error: ") and "\n" not in message
    return message


def test_refusals_name_their_cause(full_runs, tmp_path):
    folder, _ = full_runs["one_group"]
    out_folder = str(tmp_path / "out") + "/"
    prefix = folder + "2/mod_train"
    message = refusal(options("one_group", out_folder, resume=prefix), batchsize=9)
    assert "--batchsize" in message and "8" in message and "9" in message
    message = refusal(dict(options("one_group", out_folder, resume=prefix), test=["0", 0.5]))
    assert "--test" in message and "0.63" in message and "0.5" in message
    message = refusal(dict(options("one_group", out_folder, resume=prefix), unbalanced=1))
    assert "--unbalanced" in message
    copy = str(tmp_path / "fewer")
    shutil.copytree(FIX, copy)
    os.remove(os.path.join(copy, "pos", "f01.xy.gz"))
    message = refusal(options("one_group", out_folder, base=copy, resume=prefix))
    assert "feature files" in message and "differ" in message
    bare = str(tmp_path / "bare" / "mod_train")
    os.makedirs(os.path.dirname(bare))
    message = refusal(options("one_group", out_folder, resume=bare))
    assert bare + ".train.json" in message and "no state file" in message
    message = refusal(options("one_group", out_folder, resume=prefix, startFrom=prefix))
    assert "--resume" in message and "--startFrom" in message and "exclude" in message
    message = refusal(dict(options("one_group", out_folder, validate=100), test=["N", "100"]))
    assert "--validate" in message and "--test" in message
    assert not os.path.exists(out_folder)                                                     # every refusal comes before anything is written


def test_start_from_takes_the_variables_and_runs_the_whole_schedule(full_runs, tmp_path):
    w = train.initial_weights(11)
    prefix = str(tmp_path / "model" / "published")
    os.makedirs(os.path.dirname(prefix))
    tfbundle.write_bundle(prefix, w)                                                          # the 14 variables, no Adam slots, no beta powers
    folder, full = full_runs["two_groups"]
    out_folder = str(tmp_path / "out") + "/"
    rec = record(options("two_groups", out_folder, startFrom=prefix, seed=2))
    assert rec["restores"] == [(prefix, 0, False)]
    assert rec["log"] == full["log"] and rec["saves"] == full["saves"]
    assert "--seed 2 is not used" in rec["text"]
    assert json.load(open(out_folder + "0.50/mod_train.train.json")) == json.load(open(folder + "0.50/mod_train.train.json"))
    # what the GPU saver's restore hands the trainer: the bundle's variables bit for bit, zero slots
    got_w, got_m, got_v = train.load_training_state(prefix, 0, False)
    assert np.array_equal(got_w, train.flatten_weights(w)) and not got_m.any() and not got_v.any() and got_m is not got_v


def test_the_bundle_is_checked_before_it_is_used(tmp_path):
    flat = train.flatten_weights(train.initial_weights(5))
    m, v = flat * 0.25, flat * flat
    prefix = str(tmp_path / "ck")
    tfbundle.write_bundle(prefix, train.checkpoint_tensors(flat, m, v, 37))
    got = train.load_training_state(prefix, 37, True)
    assert all(np.array_equal(a, b) for a, b in zip(got, (flat, m, v)))
    with pytest.raises(SystemExit) as exc:
        train.load_training_state(prefix, 36, True)                                           # the step count of another checkpoint
    assert "beta1_power" in str(exc.value) and "t = 36" in str(exc.value)
    tensors = train.checkpoint_tensors(flat, m, v, 37)
    del tensors["Variable/Adam_1"]
    tfbundle.write_bundle(prefix, tensors)
    with pytest.raises(SystemExit) as exc:
        train.load_training_state(prefix, 37, True)
    assert "'Variable/Adam_1'" in str(exc.value) and "no tensor" in str(exc.value)
    assert np.array_equal(train.load_training_state(prefix, 0, False)[0], flat)              # --startFrom does not ask for the slots
    tensors = train.checkpoint_tensors(flat, m, v, 37)
    tensors["Variable_1"] = np.zeros(3, np.float32)
    tfbundle.write_bundle(prefix, tensors)
    for slots in (True, False):
        with pytest.raises(SystemExit) as exc:
            train.load_training_state(prefix, 37, slots)
        assert "'Variable_1'" in str(exc.value) and "shape" in str(exc.value)
    with pytest.raises(SystemExit) as exc:
        train.load_training_state(str(tmp_path / "nothing"), 0, False)
    assert "no TF checkpoint" in str(exc.value)


def test_best_checkpoint_by_auc():
    rows = [dict(checkpoint="a", auc=None), dict(checkpoint="b", auc=0.7), dict(checkpoint="c", auc=0.9), dict(checkpoint="d", auc=0.9)]
    assert train.best_checkpoint(rows)["checkpoint"] == "c"                                   # ties go to the earliest
    assert train.best_checkpoint(rows[:1])["checkpoint"] == "a" and train.best_checkpoint([]) is None
    assert train.best_checkpoint([rows[0], dict(checkpoint="e", auc=None)])["checkpoint"] == "a"


def test_command_line_of_the_new_flags(capsys):
    p = cli.build_parser()
    a = p.parse_args(['train', '--wrkBase', 'a'])
    assert (a.resume, a.startFrom, a.validate) == (None, None, 0)
    mo = cli.train_options(a)
    assert (mo['resume'], mo['startFrom'], mo['validate']) == (None, None, 0)
    mo = cli.train_options(p.parse_args(['train', '--wrkBase', 'a', '--resume', 'out/1.50/mod', '--test', 'P,80', '--validate', '1000']))
    assert (mo['resume'], mo['startFrom'], mo['validate'], mo['test']) == ('out/1.50/mod', None, 1000, ['0', 0.8])
    assert cli.train_options(p.parse_args(['train', '--wrkBase', 'a', '--startFrom', 'm/x']))['startFrom'] == 'm/x'
    for bad, words in ((['--resume', 'x', '--startFrom', 'y'], 'exclude each other'), (['--validate', '5'], '--validate needs --test'),
                       (['--validate', '-1', '--test', 'P,80'], 'non-negative')):
        with pytest.raises(SystemExit) as exc:
            cli.train_options(p.parse_args(['train', '--wrkBase', 'a'] + bad))
        assert str(exc.value).startswith('Error: ') and words in str(exc.value), bad
    assert 'resume' not in cli.train_options(p.parse_args(['predict', '--wrkBase', 'a']), cmd='predict', keys=('modfile', 'threads'))
    # --modfile keeps its note and still changes nothing
    out_folder = "unused/"
    with pytest.raises(SystemExit):
        train.mMult_RNN_LSTM_train(dict(options("one_group", out_folder, base="/nonexistent"), modfile="some/model"), batchsize=8,
                                   session_factory=lambda init: None)
    assert "--modfile some/model is accepted and ignored" in capsys.readouterr().out
