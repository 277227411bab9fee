#!/usr/bin/env python
"""`DeepMod.py predict` on synthetic feature files of the size getfeatures writes by default (150,000 rows, about 10 MB of '%.3f' text): what
the host loader costs (gunzip, np.loadtxt), what the device loader costs (dm_xyload_parse / dm_xyload_select by HIP events, and the calls
by wall clock), and the whole command -> a markdown table for profiles/predict/README.md.  Recorded, not gated.

    python tools/predict_rate.py [--rows N] [--files F] [--runs K] [--threads T] [--out FILE]
"""
import argparse
import gzip
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def feature_text(rows, seed, labelled=0.02):
    rng = np.random.default_rng(seed)
    t = np.zeros((rows, 10))
    t[:, 0] = 100000 + np.arange(rows)
    t[np.arange(rows), 3 + rng.integers(0, 4, rows)] = 1.0
    t[:, 7] = np.clip(rng.normal(0.0, 1.2, rows), -5, 5)
    t[:, 8] = np.abs(rng.normal(0.25, 0.15, rows))
    t[:, 9] = rng.geometric(0.12, rows)
    lab = np.zeros(rows, bool)
    lab[10:rows - 10] = rng.random(rows - 20) < labelled
    positive = rng.random(rows) < 0.5
    t[lab & positive, 2] = 1.0
    t[lab & ~positive, 1] = 1.0
    out = io.BytesIO()
    np.savetxt(out, t, fmt='%.3f')
    return out.getvalue()


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=150000)
    ap.add_argument('--files', type=int, default=8)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--threads', type=int, default=4)
    ap.add_argument('--out')
    a = ap.parse_args()
    from deepmod_amd import model, synth, tfbundle, xyload
    work = tempfile.mkdtemp(prefix='predict_rate_')
    data = os.path.join(work, 'xy')
    os.makedirs(data)
    for k in range(a.files):
        with gzip.open(os.path.join(data, '%d.xy.gz' % k), 'wb', compresslevel=1) as fh:
            fh.write(feature_text(a.rows, k))
    first = os.path.join(data, '0.xy.gz')
    prefix = os.path.join(work, 'ckpt', 'mod')
    os.makedirs(os.path.dirname(prefix))
    tfbundle.write_bundle(prefix, synth.synthetic_weights(seed=11, scale=4.0))

    raw = open(first, 'rb').read()
    gunzip, loadtxt = [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        text = gzip.decompress(raw)
        gunzip.append(time.perf_counter() - t0)
    for _ in range(min(a.runs, 3)):
        t0 = time.perf_counter()
        table = np.loadtxt(io.BytesIO(text), dtype=np.float32, ndmin=2)
        loadtxt.append(time.perf_counter() - t0)

    loader = xyload.XYLoader(0)
    weights = synth.synthetic_weights(seed=11, scale=4.0)
    m = model.BiLSTMModel(weights, 0, precision='f16x3')
    parse_ms, select_ms, parse_wall, select_wall, classify_wall, table_wall = [], [], [], [], [], []
    for k in range(a.runs + 1):
        t0 = time.perf_counter()
        rows, flag, _ = loader.parse(text)
        t1 = time.perf_counter()
        n = loader.select('N')
        t2 = time.perf_counter()
        loader.classify(m)
        t3 = time.perf_counter()
        loader.fetch_table()
        t4 = time.perf_counter()
        if k == 0:
            continue                                     # the first call sizes the buffers
        p, s = loader.times()
        parse_ms.append(p)
        select_ms.append(s)
        parse_wall.append(1e3 * (t1 - t0))
        select_wall.append(1e3 * (t2 - t1))
        classify_wall.append(1e3 * (t3 - t2))
        table_wall.append(1e3 * (t4 - t3))
    assert flag == 0 and rows == len(table)
    loader.close()
    m.close()

    walls, stats = [], None
    for k in range(2):
        cmd = [sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'predict', '--wrkBase', data, '--modfile', prefix, '--outFolder', os.path.join(work, 'out%d' % k),
               '--threads', str(a.threads)]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True)
        walls.append(time.perf_counter() - t0)
        if r.returncode != 0:
            sys.exit(r.stdout[-2000:] + r.stderr[-2000:])
        stats = json.loads(r.stdout.strip().splitlines()[-1])
    lines = ['| one file | %d rows, %.1f MB of text, %.1f MB gzip level 1, %d labelled rows |' % (rows, len(text) / 1e6, len(raw) / 1e6, n),
             '| gunzip (host, one thread) | %.3f s (median of %d) |' % (med(gunzip), len(gunzip)),
             '| np.loadtxt(dtype=float32) of the text (host) | %.3f s (median of %d, %.3f - %.3f) |' % (med(loadtxt), len(loadtxt), min(loadtxt), max(loadtxt)),
             '| dm_xyload_parse, HIP events around its kernels | %.3f ms (median of %d, %.3f - %.3f) = %.2e B/s |' %
             (med(parse_ms), len(parse_ms), min(parse_ms), max(parse_ms), len(text) / (1e-3 * med(parse_ms))),
             '| dm_xyload_parse, the call (upload of the text from pageable memory included) | %.3f ms (median of %d) |' % (med(parse_wall), len(parse_wall)),
             '| dm_xyload_select, HIP events | %.3f ms (median of %d, %.3f - %.3f) |' % (med(select_ms), len(select_ms), min(select_ms), max(select_ms)),
             '| dm_xyload_select, the call | %.3f ms (median of %d) |' % (med(select_wall), len(select_wall)),
             '| dm_xyload_classify, the call: classifier, the gather of column 1, %d B back (6 per window) | %.3f ms (median of %d, %.3f - %.3f) |' %
             (6 * n, med(classify_wall), len(classify_wall), min(classify_wall), max(classify_wall)),
             '| for comparison only, not part of the command: the whole table to the host (dm_xyload_fetch, %d B) | %.3f ms (median of %d) |' %
             (40 * rows, med(table_wall), len(table_wall)),
             '| whole command (fresh process, --threads %d), %d files, %d windows | %.2f s, second run %.2f s = %.1f files/s, %.0f windows/s (2 runs) |' %
             (a.threads, stats['files'], stats['windows'], walls[0], walls[1], stats['files'] / walls[1], stats['windows'] / walls[1]),
             '| fallback files | %d |' % stats['fallback_files']]
    out = '| | |\n|---|---|\n' + '\n'.join(lines) + '\n'
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(out)


if __name__ == '__main__':
    main()
