#!/usr/bin/env python
"""Wall time of a whole `train` command on an MI355X, host-fed (the default) against `--resident 1`.

    python tools/train_input_rate.py [--files 8] [--rows 100000] [--labelled 0.25] [--batchsize 2048] [--runs 3] [--threads 4]

Writes --files feature files of --rows rows each (tools/validate_rate.py's table) into one folder - one group - and runs the command
`DeepMod.py train --wrkBase <folder> --batchsize <batchsize> --seed 4 --threads <threads>` in this process, alternately without and with
`--resident 1`, --runs times each after one uncounted round of both.  Per run: the host clock around the whole command (session, loading, four
epochs, every checkpoint), the device time and the number of steps from Trainer.profile() (HIP events around every step), and for the resident
run the one-off load seconds and the resident bytes of its `resident:` line.  The last checkpoints of every pair of runs must be byte-equal; the
tool fails if they are not.  Prints a section for profiles/train/README.md.  A run that finds no GPU fails; nothing is estimated.
"""
import argparse
import contextlib
import datetime
import importlib.util
import io
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--labelled", type=float, default=0.25)
    ap.add_argument("--batchsize", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=4)
    a = ap.parse_args()
    from deepmod_amd import _lib, train
    from validate_rate import feature_table
    if _lib.load().dm_device_count() < 1:
        raise SystemExit("train_input_rate: no gfx950 device visible")
    spec = importlib.util.spec_from_file_location("dmcli_train_input_rate", os.path.join(ROOT, "bin", "DeepMod.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)

    # the step clock of the run's trainer: switched on when the session creates it, read when the session closes
    profile = {}
    create, close = train.Trainer.__init__, train.TrainSession.close

    def created(self, *args, **kw):
        create(self, *args, **kw)
        self.profile(True)

    def closing(self):
        if self.trainer is not None:
            ms, steps = self.trainer.profile(False)
            profile["ms"], profile["steps"] = profile.get("ms", 0.0) + ms, profile.get("steps", 0) + steps
        close(self)
    train.Trainer.__init__, train.TrainSession.close = created, closing

    with tempfile.TemporaryDirectory() as base:
        data = os.path.join(base, "xy")
        os.makedirs(data)
        for i in range(a.files):
            np.savetxt(os.path.join(data, "f%03d.xy.gz" % i), feature_table(a.rows, 1000 + i * a.rows, a.labelled, i), fmt="%.3f")

        def run(tag, resident):
            out = os.path.join(base, tag) + "/"
            argv = ["train", "--wrkBase", data, "--FileID", "mod_train", "--outFolder", out, "--batchsize", str(a.batchsize), "--seed", "4",
                    "--threads", str(a.threads)] + (["--resident", "1"] if resident else [])
            args = cli.build_parser().parse_args(argv)
            profile.clear()
            text = io.StringIO()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(text):
                args.func(args)
            wall = time.perf_counter() - t0
            got = dict(wall=wall, ms=profile.get("ms", 0.0), steps=profile.get("steps", 0), load=None, nbytes=None, windows=None)
            line = re.search(r"^resident: (\d+) files, (\d+) rows, (\d+) windows stay on the device: (\d+) bytes \(([0-9.]+) s\)", text.getvalue(), re.M)
            if resident:
                if not line:
                    raise SystemExit("train_input_rate: the resident run printed no `resident:` line")
                got.update(windows=int(line.group(3)), nbytes=int(line.group(4)), load=float(line.group(5)))
            last = os.path.join(out, "4")
            got["last"] = {name: open(os.path.join(last, name), "rb").read() for name in sorted(os.listdir(last))}
            return got

        host, res = [], []
        for i in range(a.runs + 1):                              # the first round of both is not counted
            h, r = run("host_%d" % i, False), run("resident_%d" % i, True)
            if h["last"] != r["last"] or h["steps"] != r["steps"]:
                raise SystemExit("train_input_rate: the last checkpoints of round %d differ, or the step counts (%d / %d)" % (i, h["steps"], r["steps"]))
            if i:
                host.append(h)
                res.append(r)

    def med(runs, key, scale=1.0):
        v = [r[key] * scale for r in runs]
        return "%.2f (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))
    ratio = statistics.median(r["wall"] for r in host) / statistics.median(r["wall"] for r in res)
    lines = ["# A whole `train` command, host-fed against `--resident 1` (tools/train_input_rate.py)", "",
             "| input | wall, s: median (min .. max) of %d | device time of the steps, s | steps | load once, s | resident bytes |" % a.runs,
             "|---|---|---|---|---|---|",
             "| host-fed (default) | %s | %s | %d | - | - |" % (med(host, "wall"), med(host, "ms", 1e-3), host[0]["steps"]),
             "| `--resident 1` | %s | %s | %d | %s | %d |" % (med(res, "wall"), med(res, "ms", 1e-3), res[0]["steps"], med(res, "load"), res[0]["nbytes"]), "",
             "%d files x %d rows, %g labelled (%d windows), one group, --batchsize %d, four epochs, --threads %d; host-fed / resident wall = %.2f.  "
             "Wall is the host clock around the whole command in one process (session, loading, steps, every checkpoint); the device time is "
             "Trainer.profile()'s HIP events around every step, uploads and the two host round trips included.  The two were run alternately after one "
             "uncounted round of both; the last checkpoints (bundle, .train.json, `checkpoint`) of every pair were byte-equal (checked in the run)." %
             (a.files, a.rows, a.labelled, res[0]["windows"], a.batchsize, a.threads, ratio), "",
             "Measured %s, one run of `python tools/train_input_rate.py --files %d --rows %d --labelled %g --batchsize %d --runs %d --threads %d` (%s)." %
             (datetime.date.today().isoformat(), a.files, a.rows, a.labelled, a.batchsize, a.runs, a.threads, _lib.load().dm_version().decode()), ""]
    print("\n".join(lines))


if __name__ == "__main__":
    main()
