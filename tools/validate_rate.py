#!/usr/bin/env python
"""Wall time of one `train --validate` pass over a resident set on an MI355X, next to `predict` on the same files.

    python tools/validate_rate.py [--files 8] [--rows 100000] [--labelled 0.25] [--repeats 5] [--threads 4]

Writes --files feature files of --rows rows each (the size getfeatures' default --size_per_batch gives is 125,000 rows) into a temporary folder,
holds all of them out (--test E over every position), loads them once into train.HeldOut (xyload.XYSet) and then times, alternating:
  * HeldOut.score(weights): what every checkpoint pays - a model from the weight blob, one classifier launch per resident file, 6 bytes per
    window back, the statistics;
  * predict.mPred on the same files with --threads host threads: gunzip, upload of the text, parse, selection, the same launches.
Both are host clocks around work that ends in a device synchronise.  The two results must be equal; the tool fails if they are not.  Prints a
section for profiles/train/README.md.  A run that finds no GPU fails; nothing is estimated.
"""
import argparse
import contextlib
import datetime
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def feature_table(rows, start, labelled, seed):
    """position | 2 labels | one-hot base, mean, stdv, length: values of the shape getfeatures writes, labelled rows away from the edges."""
    rng = np.random.default_rng(seed)
    t = np.zeros((rows, 10))
    t[:, 0] = start + np.arange(rows)
    pick = np.flatnonzero(rng.random(rows) < labelled)
    pick = pick[(pick >= 10) & (pick < rows - 10)]
    positive = rng.random(len(pick)) < 0.5
    t[pick[positive], 2] = 1.0
    t[pick[~positive], 1] = 1.0
    t[np.arange(rows), 3 + rng.integers(0, 4, rows)] = 1.0
    t[:, 7] = np.clip(rng.normal(0.0, 1.2, rows), -5, 5)
    t[:, 8] = np.abs(rng.normal(0.25, 0.15, rows))
    t[:, 9] = rng.geometric(0.12, rows)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--labelled", type=float, default=0.25)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=4)
    a = ap.parse_args()
    from deepmod_amd import _lib, model, predict, tfbundle, train
    if _lib.load().dm_device_count() < 1:
        raise SystemExit("validate_rate: no gfx950 device visible")
    with tempfile.TemporaryDirectory() as base:
        folders = [os.path.join(base, "a"), os.path.join(base, "b")]
        for i in range(a.files):
            os.makedirs(folders[i % 2], exist_ok=True)
            np.savetxt(os.path.join(folders[i % 2], "f%03d.xy.gz" % i), feature_table(a.rows, 1000 + i * a.rows, a.labelled, i), fmt="%.3f")
        weights = train.initial_weights(0)
        prefix = os.path.join(base, "ckpt", "mod")
        os.makedirs(os.path.dirname(prefix))
        tfbundle.write_bundle(prefix, weights)
        flat = model.flatten_weights(weights)
        mo = {"wrkBase": ",".join(folders), "recursive": 1, "test": ["-", 0, 10 ** 12], "windowsize": 21, "threads": a.threads, "outputlayer": ""}
        quiet = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            held = train.HeldOut(mo, 10 ** 12, 0)
        load_s = time.perf_counter() - t0
        model.mCreateSession(7, 100, 21, mo)

        def by_predict():
            with contextlib.redirect_stdout(quiet):
                return predict.mPred(prefix, os.path.dirname(prefix) + "/", None, None, None, [held.files], os.path.join(base, "mpred.txt"), 7, None, None, None,
                                     None, None, 21, mo)
        try:
            resident, again = [], []
            for i in range(a.repeats + 1):                       # the first round warms both up and is not counted
                t0 = time.perf_counter()
                got = held.score(flat)
                t1 = time.perf_counter()
                want = by_predict()
                t2 = time.perf_counter()
                if got != want:
                    raise SystemExit("validate_rate: the resident pass and predict disagree: %r / %r" % (got, want))
                if i:
                    resident.append(t1 - t0)
                    again.append(t2 - t1)
            nbytes, stats = held.set.nbytes(), got
        finally:
            held.close()

    def ms(v):
        return "%.1f (%.1f .. %.1f)" % (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3)
    lines = ["# One `--validate` pass over a resident set (tools/validate_rate.py)", "",
             "| files | rows | windows | resident bytes | load once, s | resident pass, ms: median (min .. max) of %d | `predict` on the same files (%d threads), ms | predict / resident |"
             % (a.repeats, a.threads),
             "|---|---|---|---|---|---|---|---|",
             "| %d | %d | %d | %d | %.2f | %s | %s | %.1f |" % (stats["files"], stats["rows"], stats["windows"], nbytes, load_s, ms(resident), ms(again),
                                                              statistics.median(again) / statistics.median(resident)), "",
             "Both columns are host clocks around a whole pass (model creation from the weights, the launches, 6 bytes per window back, the statistics; "
             "`predict` also gunzips, uploads and parses the text) and give equal results (checked in the run: %s, accuracy %.4f).  The two were timed "
             "alternately after one uncounted round." % (stats["precision_mode"], stats["accuracy"]), "",
             "Measured %s, one run of `python tools/validate_rate.py --files %d --rows %d --labelled %g --repeats %d --threads %d` (%s)." %
             (datetime.date.today().isoformat(), a.files, a.rows, a.labelled, a.repeats, a.threads, _lib.load().dm_version().decode()), ""]
    print("\n".join(lines))


if __name__ == "__main__":
    main()
