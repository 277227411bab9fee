#!/usr/bin/env python
"""The kernels of `diffmod` on a synthetic contig.

    python tools/diffmod_rate.py [LENGTH] [--depth 30] [--repeat 5] [--out diffmod_rate.json]

One contig of LENGTH positions (default 4,600,000); every second position, on alternating strands, carries a sample and a control record with
Poisson(--depth) coverage and a modified count drawn from a per-site rate, the control's from the same rate except at 1 % of the sites.  The tables
are filled on the device.  Reported, each from HIP events as the median of --repeat runs after one untimed run:
  select      ms of the two select passes and their scan; keys (2 x positions) examined per second
  fisher      ms of the two test kernels and their scan; table terms (the sum of the supports S of the tested keys) per second
  deep key    the same contig with one key of cA = cB = 2^19, mA = mB = 2^18 added (S = 524,289): fisher ms again - a deep key should cost about its own
              terms at the rate above, not a wave's worth of waiting neighbours
  host twin   dm_diffmod_test_host on the same tables on this box's CPU (one thread), wall clock, for comparison; its counters and records must
              equal the device's and its p agree to 1e-9 relative
The input is generated in this process and is not part of any figure."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 8 << 20


def make_input(length, depth, seed=3):
    rng = np.random.default_rng(seed)
    pos = np.arange(0, length, 2, dtype=np.int32)
    strand = ((pos >> 1) & 1).astype(np.uint8)
    rate = rng.choice(np.array([0.02, 0.1, 0.5, 0.9]), len(pos), p=(0.5, 0.2, 0.1, 0.2))
    other = np.where(rng.random(len(pos)) < 0.01, rng.random(len(pos)), rate)
    recs = {}
    for role, r in (('sample', rate), ('control', other)):
        cov = np.maximum(rng.poisson(depth, len(pos)), 1).astype(np.int32)
        recs[role] = (pos, strand, cov, rng.binomial(cov, r).astype(np.int32))
    return recs


def fill(dm, recs, length, extra=None):
    dm.open('chr1', length)
    pos, strand, cov, mod = recs
    for lo in range(0, len(pos), CHUNK):                              # bounded uploads
        dm.add_records(pos[lo:lo + CHUNK], strand[lo:lo + CHUNK], cov[lo:lo + CHUNK], mod[lo:lo + CHUNK])
    if extra is not None:
        dm.add_records(*[np.array([v]) for v in extra])


def supports(recs, cov):
    cA, mA, cB, mB = (recs[k][j].astype(np.int64) for k in ('sample', 'control') for j in (2, 3))
    tested = (cA >= cov) & (cB >= cov)
    M = mA + mB
    return int((np.minimum(cA, M) - np.maximum(0, M - cB) + 1)[tested].sum()), int(tested.sum())


def timed(dev, tabs, repeat):
    sel, fis = [], []
    for rep in range(repeat + 1):
        before = dev.times()
        counters, got = dev.run(*tabs)
        after = dev.times()
        if rep:
            sel.append(after[0] - before[0])
            fis.append(after[1] - before[1])
    return counters, got, sel, fis


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('length', type=int, nargs='?', default=4600000)
    ap.add_argument('--depth', type=int, default=30)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from deepmod_amd import diffmod, merge

    def say(what):
        print('[diffmod_rate] %s' % what, file=sys.stderr, flush=True)

    length, cov = args.length, 5
    recs = make_input(length, args.depth)
    terms, n_tested = supports(recs, cov)
    say('%d positions, %d records per role, %d tested keys, %d table terms' % (length, len(recs['sample'][0]), n_tested, terms))
    sample, control = merge.DeviceMerge(0), merge.DeviceMerge(0)
    dev = diffmod.DeviceEngine(cov, 0.05)
    out = {'positions': length, 'depth': args.depth, 'repeat': args.repeat, 'tested_keys': n_tested, 'table_terms': terms}
    fill(sample, recs['sample'], length)
    fill(control, recs['control'], length)
    tabs = (sample.plus, sample.minus, control.plus, control.minus)
    counters, got, sel, fis = timed(dev, tabs, args.repeat)
    assert int(counters[:, 0].sum()) == n_tested
    t_sel, t_fis = statistics.median(sel) * 1e-3, statistics.median(fis) * 1e-3
    out['select'] = {'kernel_ms': statistics.median(sel), 'all_kernel_ms': sel, 'keys_per_s': 2 * length / t_sel}
    out['fisher'] = {'kernel_ms': statistics.median(fis), 'all_kernel_ms': fis, 'terms_per_s': terms / t_fis, 'records': int(len(got['p']))}
    say('select %.3f ms (%.3g keys/s), fisher %.3f ms (%.3g terms/s), %d records' % (out['select']['kernel_ms'], out['select']['keys_per_s'], out['fisher']['kernel_ms'],
                                                                                        out['fisher']['terms_per_s'], len(got['p'])))
    # the compiled twin on the same tables
    host = [(np.zeros(length, np.int32), np.zeros(length, np.int32)) for _ in range(4)]
    for r, role in enumerate(('sample', 'control')):
        pos, strand, cv, md = recs[role]
        for s in range(2):
            host[2 * r + s][0][pos[strand == s]] = cv[strand == s]
            host[2 * r + s][1][pos[strand == s]] = md[strand == s]
    t0 = time.perf_counter()
    counters2, _, rec2 = diffmod.host_routine(cov, 0.05, *host)
    wall = time.perf_counter() - t0
    assert counters2.tolist() == counters.tolist() and all(rec2[k].tolist() == got[k].tolist() for k in ('pos', 'strand', 'cA', 'mA', 'cB', 'mB')), 'device and twin disagree'
    assert (np.abs(rec2['p'] - got['p']) <= 1e-9 * rec2['p']).all(), 'p of the device and of the twin differ by more than 1e-9'
    out['host_twin'] = {'wall_s': wall, 'terms_per_s': terms / wall, 'equal_records': int(len(rec2['p']))}
    say('host twin %.2f s (%.3g terms/s)' % (wall, terms / wall))
    # one deep key more
    deep = 1 << 19
    spot = length - 1 if (length - 1) % 2 else length - 2             # a position without a record
    fill(sample, recs['sample'], length, (spot, 0, deep, deep // 2))
    fill(control, recs['control'], length, (spot, 0, deep, deep // 2))
    counters3, got3, sel3, fis3 = timed(dev, (sample.plus, sample.minus, control.plus, control.minus), args.repeat)
    assert int(counters3[:, 0].sum()) == n_tested + 1 and got3['p'][got3['pos'] == spot].tolist() == []       # p = 1: not a record
    t_deep = statistics.median(fis3) * 1e-3
    out['deep_key'] = {'support': deep + 1, 'fisher_kernel_ms': statistics.median(fis3), 'all_kernel_ms': fis3, 'extra_ms': statistics.median(fis3) - statistics.median(fis),
                       'its_terms_at_the_rate_above_ms': (deep + 1) / out['fisher']['terms_per_s'] * 1e3, 'terms_per_s': (terms + deep + 1) / t_deep}
    say('with the deep key: fisher %.3f ms' % statistics.median(fis3))
    for h in (dev, sample, control):
        h.close()
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
