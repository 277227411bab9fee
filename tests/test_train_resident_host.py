"""CPU: the catalogue side of `train --resident 1` (deepmod_amd/train.py: ResidentCatalogue, _ResidentReader, SetWindows) on the fixture folders of
tests/golden/train/.  The set's layout is rebuilt on the host with the routines the device runs (xyload.load_host / select_host, the host
fallback for a text with nan): feature rows of all files with windows behind each other, centres relative to their file, a window's id its
index over the concatenated files.  The resident reader then has to name, pool call by pool call, exactly the windows _GroupReader reads."""
import contextlib
import gzip
import importlib.util
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from deepmod_amd import train, xyload

FIX = os.path.join(GOLDEN, "train")
TESTS = {"N": ["N", "100"], "P50": ["0", 0.5]}
GROUPS = {"one_group": "neg,pos", "two_groups": "neg;pos"}
BATCH = 8

spec = importlib.util.spec_from_file_location('deepmod_cli_train_resident', os.path.join(ROOT, 'bin', 'DeepMod.py'))
cli = importlib.util.module_from_spec(spec)
spec.loader.exec_module(cli)


def options(groups, test, **more):
    mo = {"wrkBase": ";".join(",".join(os.path.join(FIX, f) for f in g.split(",")) for g in groups.split(";")), "recursive": 1, "test": list(test),
          "fnum": 7, "hidden": 100, "windowsize": 21, "outFolder": "unused/", "FileID": "mod_train", "modfile": None, "unbalanced": 0, "outputlayer": ""}
    mo.update(more)
    return mo


def groups_of(mo):
    with contextlib.redirect_stdout(io.StringIO()):
        return train.file_groups(mo)


class HostSet:
    """What xyload.XYSet holds after the files were loaded in order, on the host: feats [rows of all segments][7], centre per window (relative to
    its segment), the two prefix sums; gather(ids) as the device resolves an id."""

    def __init__(self, files, mo):
        self.catalogue = train.ResidentCatalogue()
        feats, centres, self.row_off, self.win_off = [], [], [0], [0]
        for fn in files:
            with contextlib.redirect_stdout(io.StringIO()):
                table, flag, _ = xyload.load_host(gzip.decompress(open(fn, "rb").read()))
                if flag:
                    sel = train.labelled_rows(table, mo, fn)
                else:
                    lo, hi = (mo['test'][1], mo['test'][2]) if mo['test'][0] in ('-', '+') else (0, 0)
                    sel = xyload.select_host(table, mo['test'][0], lo, hi, fn)[0]
            self.catalogue.add(fn, table[sel, 1:3].astype(int))
            if len(sel):
                feats.append(table[:, 3:])
                centres.append(np.asarray(sel, np.int64))
                self.row_off.append(self.row_off[-1] + len(table))
                self.win_off.append(self.win_off[-1] + len(sel))
        self.feats = np.concatenate(feats) if feats else np.zeros((0, 7), np.float32)
        self.centre = np.concatenate(centres) if centres else np.zeros(0, np.int64)

    def gather(self, ids):
        ids = np.asarray(ids, np.int64)
        assert ((ids >= 0) & (ids < self.win_off[-1])).all()
        seg = np.searchsorted(np.asarray(self.win_off), ids, side="right") - 1
        first = np.asarray(self.row_off)[seg] + self.centre[ids] - 10
        return np.ascontiguousarray(self.feats[first[:, None] + np.arange(21)[None, :]])


def drive(lead, others, call, restart):
    """The pool calls train_save_model makes in two epochs: rounds of the leading group to exhaustion, every other group recycled against it."""
    for _ in range(2):
        restart(lead)
        while not lead.exhausted():
            y0 = call(lead, BATCH * train.SUMPSIZE, False)
            steps = len(y0) // BATCH
            if steps < 1:
                continue
            for other in others:
                call(other, BATCH * steps, True)


@pytest.mark.parametrize("test", sorted(TESTS))
@pytest.mark.parametrize("groups", sorted(GROUPS))
def test_the_resident_reader_names_the_windows_the_file_reader_reads(groups, test):
    mo = options(GROUPS[groups], TESTS[test])
    filelists = groups_of(mo)
    assert len(filelists) == (1 if groups == "one_group" else 2) and all(filelists)
    host = HostSet(list(dict.fromkeys(fn for files in filelists for fn in files)), mo)
    a = [train._GroupReader(files, mo) for files in filelists]
    b = [train._ResidentReader(files, host.catalogue) for files in filelists]
    pair = {id(ra): rb for ra, rb in zip(a, b)}
    calls, wrapped = [0], [0]
    digest = train.filelists_digest(filelists, mo)

    def call(reader, wanted, wrap):
        other = pair[id(reader)]
        before = reader.next
        with contextlib.redirect_stdout(io.StringIO()):
            x, y = reader.pool(wanted, wrap)
        ids, yb = other.pool(wanted, wrap)
        assert ids.dtype == np.int64 and ids.shape == (len(y),)
        assert np.asarray(yb).dtype == np.asarray(y).dtype and np.array_equal(yb, y)
        assert host.gather(ids).tobytes() == np.ascontiguousarray(x, dtype=np.float32).tobytes()
        assert other.next == reader.next and other.exhausted() == reader.exhausted()
        assert train.schedule_state(1, False, b, 7, BATCH, mo, digest) == train.schedule_state(1, False, a, 7, BATCH, mo, digest)
        calls[0] += 1
        wrapped[0] += int(wrap and reader.next <= before)
        return y

    def restart(reader):
        reader.next = pair[id(reader)].next = 0

    drive(a[0], a[1:], call, restart)
    assert calls[0] >= 4
    if groups == "two_groups":
        assert wrapped[0] >= 1                      # the smaller group started over at least once


def test_a_file_without_a_window_has_no_segment_and_idle_files_end_alike():
    mo = options("neg;pos", ["+", 10 ** 6, 2 * 10 ** 6])             # only f02 and f09 hold rows in the region; every other file is idle
    filelists = groups_of(mo)
    host = HostSet([fn for files in filelists for fn in files], mo)
    assert sorted(host.catalogue.first.values())[:2] == [-1, -1] and host.catalogue.total == host.win_off[-1] > 0
    assert len(host.win_off) - 1 == sum(1 for k in host.catalogue.windows.values() if k > 0) < len(host.catalogue.windows)
    for files in filelists:
        a, b = train._GroupReader(files, mo), train._ResidentReader(files, host.catalogue)
        with contextlib.redirect_stdout(io.StringIO()):
            x, y = a.pool(10 ** 6, False)
        ids, yb = b.pool(10 ** 6, False)
        assert np.array_equal(y, yb) and host.gather(ids).tobytes() == np.ascontiguousarray(x, np.float32).tobytes() and a.next == b.next == len(files)
    empty = options("neg;pos", ["+", 5 * 10 ** 7, 6 * 10 ** 7])       # no row of any file lies there
    filelists = groups_of(empty)
    host = HostSet([fn for files in filelists for fn in files], empty)
    assert host.catalogue.total == 0 and set(host.catalogue.first.values()) == {-1}
    files = filelists[1]
    a, b = train._GroupReader(files, empty), train._ResidentReader(files, host.catalogue)
    ids, yb = b.pool(8, False)
    assert ids.shape == (0,) and ids.dtype == np.int64 and np.asarray(yb).shape == (0, 2) and b.next == len(files)
    a.next = b.next = 0
    with pytest.raises(ValueError) as ea:
        a.pool(8, True)
    with pytest.raises(ValueError) as eb:
        b.pool(8, True)
    assert str(ea.value) == str(eb.value) and "no labelled window in any of the %d files" % len(files) in str(eb.value)
    assert a.next == b.next


def test_the_flag_on_the_command_line_and_its_refusal_with_a_recording_session(capsys):
    parser = cli.build_parser()
    args = parser.parse_args(["train", "--wrkBase", FIX, "--resident", "1", "--threads", "3"])
    mo = cli.train_options(args)
    assert mo["resident"] == 1 and mo["threads"] == 3
    assert cli.train_options(parser.parse_args(["train", "--wrkBase", FIX]))["resident"] == 0
    with pytest.raises(SystemExit):
        parser.parse_args(["train", "--wrkBase", FIX, "--resident", "2"])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        parser.parse_args(["train", "--help"])
    assert "--resident" in capsys.readouterr().out
    with pytest.raises(SystemExit) as exc, contextlib.redirect_stdout(io.StringIO()):
        train.mMult_RNN_LSTM_train(options("neg;pos", TESTS["N"], resident=1), batchsize=BATCH, session_factory=lambda init: None)
    assert "--resident" in str(exc.value) and "session_factory" in str(exc.value) and "\n" not in str(exc.value)


def test_set_windows_is_a_sized_wrapper():
    w = train.SetWindows(object(), [3, 1, 2])
    assert len(w) == 3 and w.ids.dtype == np.int64 and w.ids.tolist() == [3, 1, 2]
