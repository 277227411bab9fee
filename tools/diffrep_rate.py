#!/usr/bin/env python
"""The sweep of `diffmod --replicates 1` on a synthetic contig.

    python tools/diffrep_rate.py [LENGTH] [--shapes 3,3:8,8] [--depth 30] [--repeat 5] [--out diffrep_rate.json]

One contig of LENGTH positions (default 4,000,000); every second position, on alternating strands, carries a record in every replicate with
Poisson(--depth) coverage and a modified count drawn from a per-site rate with some spread between the replicates, the controls' from the same rate
except at 1 % of the sites.  The tables are filled on the device.  Per shape KA,KB and for alpha 0.05 and 1, each from HIP events as the median of
--repeat runs after one untimed run:
  count       ms of the counting pass (fates, tests, histogram, records per tile) and its scan
  write       ms of the writing pass (the tests again, the records in key order)
  bound       the ms the two passes need to read their 2 x 16 x (KA + KB) bytes per position once each at --hbm TB/s (default 8: the MI355X data sheet)
The counters are checked against numpy.  The input is generated in this process and is not part of any figure."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 8 << 20
COV = 5


def make_input(length, depth, K, KA, seed=3):
    rng = np.random.default_rng(seed)
    pos = np.arange(0, length, 2, dtype=np.int32)
    strand = ((pos >> 1) & 1).astype(np.uint8)
    rate = rng.choice(np.array([0.02, 0.1, 0.5, 0.9]), len(pos), p=(0.5, 0.2, 0.1, 0.2))
    other = np.where(rng.random(len(pos)) < 0.01, rng.random(len(pos)), rate)
    recs = []
    for j in range(K):
        cov = np.maximum(rng.poisson(depth, len(pos)), 1).astype(np.int32)
        r = np.clip((rate if j < KA else other) + 0.05 * rng.standard_normal(len(pos)), 0.0, 1.0)
        recs.append((pos, strand, cov, rng.binomial(cov, r).astype(np.int32)))
    return recs


def fill(dm, rec, length):
    dm.open('chr1', length)
    pos, strand, cov, mod = rec
    for lo in range(0, len(pos), CHUNK):                              # bounded uploads
        dm.add_records(pos[lo:lo + CHUNK], strand[lo:lo + CHUNK], cov[lo:lo + CHUNK], mod[lo:lo + CHUNK])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('length', type=int, nargs='?', default=4000000)
    ap.add_argument('--shapes', default='3,3:8,8')
    ap.add_argument('--depth', type=int, default=30)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--hbm', type=float, default=8.0, help='TB/s the bound is stated at')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from deepmod_amd import diffmod, merge

    def say(what):
        print('[diffrep_rate] %s' % what, file=sys.stderr, flush=True)

    length = args.length
    out = {'positions': length, 'depth': args.depth, 'repeat': args.repeat, 'hbm_tb_s': args.hbm, 'shapes': {}}
    for shape in args.shapes.split(':'):
        KA, KB = (int(v) for v in shape.split(','))
        K = KA + KB
        recs = make_input(length, args.depth, K, KA)
        covs = np.stack([r[2] for r in recs])
        deep = covs >= COV
        tested = int((deep[:KA].all(axis=0) & deep[KA:].all(axis=0) & (covs.sum(axis=0) <= diffmod.MAX_TOTAL)).sum())
        merges = [merge.DeviceMerge(0) for _ in range(K)]
        for dm, rec in zip(merges, recs):
            fill(dm, rec, length)
        tabs = [(dm.plus, dm.minus) for dm in merges]
        bytes_per_pass = 16 * K * length
        entry = {'tested_keys': tested, 'bytes_per_pass': bytes_per_pass, 'bound_ms_both_passes': 2 * bytes_per_pass / (args.hbm * 1e12) * 1e3}
        for alpha in (0.05, 1.0):
            dev = diffmod.RepDeviceEngine(COV, alpha, KA, KB)
            count, write = [], []
            for rep in range(args.repeat + 1):
                before = dev.times()
                counters, _ = dev.run(tabs[:KA], tabs[KA:], fetch_run=1 << 22)
                after = dev.times()
                if rep:
                    count.append(after[0] - before[0])
                    write.append(after[1] - before[1])
            assert int(counters[:, 0].sum()) == tested, (counters, tested)
            c, w = statistics.median(count), statistics.median(write)
            entry['alpha_%g' % alpha] = {'count_ms': c, 'write_ms': w, 'all_count_ms': count, 'all_write_ms': write, 'records': int(dev.n_records),
                                         'count_tb_s': bytes_per_pass / (c * 1e-3) / 1e12, 'write_tb_s': bytes_per_pass / (w * 1e-3) / 1e12 if w else None,
                                         'tested_keys_per_s_count': tested / (c * 1e-3)}
            say('%d,%d alpha %g: count %.3f ms, write %.3f ms (%d records of %d tested keys); the bound for both passes: %.3f ms' %
                (KA, KB, alpha, c, w, dev.n_records, tested, entry['bound_ms_both_passes']))
            dev.close()
        for dm in merges:
            dm.close()
        out['shapes'][shape] = entry
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
