#!/usr/bin/env python
"""Regenerates tests/golden/bsperf_case.json: a small input of `bsperf` and what the definition of docs/Reproducibility.md (Example 3, Step 5) makes
of it, computed WITHOUT deepmod_amd: the files are read with split() and int() into plain dicts, the labels and the join are dict look-ups, AUC and
average precision are sklearn.metrics', r is numpy.corrcoef's, the RMSE is computed directly.

    python tests/golden/make_golden_bsperf.py

Two contigs (chrA, chrB; chrC is in the replicates and not requested), two whole-genome replicates, three prediction files in two runs (chrA '+' in
both runs, chrB '-' in one; chrA '-' and chrB '+' have truth and no prediction).  The JSON holds data only: the texts, the options, the integers,
the scores and the report lines.  The script stops if a class is empty at a threshold, or if a printed digit depends on the last bits of a score.
"""
import json
import math
import os

import numpy as np
from sklearn.metrics import auc, average_precision_score, roc_curve

HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS, METHYLATED, UNMETHYLATED, PRED_COV, R = (2, 5, 10), 90, 0, 2, 2     # (a smallest threshold above 1: sites below it exist)
CONTIGS = {'chrA': 300, 'chrB': 150}


def make_inputs():
    rng = np.random.default_rng(20)
    reps = [['chrom\tstart\tend\tname\tscore\tstrand\tthickStart\tthickEnd\tcolor\tcoverage\tpercentage'] for _ in range(R)]
    pred = {'runA/mod_pos.chrA+.C.bed': [], 'runB/sub/mod_pos.chrA+.C.bed': [], 'runA/mod_pos.chrB-.C.bed': []}
    for chrom, length in list(CONTIGS.items()) + [('chrC', 30)]:
        for strand in '+-':
            for pos in range(length):
                u = rng.random()
                if u < 0.55:
                    continue
                kind = rng.choice(4, p=[0.35, 0.35, 0.2, 0.1])                 # methylated, unmethylated, intermediate, mixed
                level = (0.95, 0.03, 0.5, 0.7)[kind]
                for r in range(R):
                    if rng.random() < 0.08:
                        continue                                             # the site is missing from this replicate
                    cov = int(rng.choice([0, 1, 2, 4, 5, 6, 9, 10, 11, 30, 70000], p=[0.03, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.15, 0.02]))
                    pct = (int(rng.integers(90, 101)), 0, int(rng.integers(1, 90)), int(rng.choice([0, 89, 90, 100])))[kind]
                    sep = '\t' if r == 0 else ' '
                    reps[r].append(sep.join([chrom, str(pos), str(pos + 1), '.', str(min(cov, 1000)), strand, str(pos), str(pos + 1), '0,0,0', str(cov), str(pct)]))
                files = [f for f in pred if '.%s%s.' % (chrom, strand) in f]
                for f in files:
                    if rng.random() < 0.25:
                        continue
                    cov = int(rng.integers(1, 25))
                    mod = int(rng.binomial(cov, min(max(level + rng.normal(0, 0.25), 0.0), 1.0)))
                    pred[f].append('%s %d %d C %d %s %d %d 0,0,0 %d %d %d ' % (chrom, pos, pos + 1, cov, strand, pos, pos + 1, cov, mod * 100 // cov, mod))
        for r in range(R):                                                   # lines the rules pass over: another strand, short lines
            reps[r].append('\t'.join([chrom, '7', '8', '.', '3', '.', '7', '8', '0,0,0', '3', '100']))
            reps[r].append('%s 1 2 . 1 +' % chrom)
            reps[r].append('')
    for chrom, strand in (('chrA', '+'), ('chrB', '-')):                     # predicted positions without truth
        f = [k for k in pred if '.%s%s.' % (chrom, strand) in k][0]
        have = {int(ln.split()[1]) for ln in pred[f]}
        for pos in range(0, CONTIGS[chrom], 37):
            if pos not in have and not any(ln.split()[0] == chrom and ln.split()[1:2] == [str(pos)] and ln.split()[5] == strand for ln in reps[0][1:] if len(ln) > 20):
                pred[f].append('%s %d %d C 3 %s %d %d 0,0,0 3 33 1 ' % (chrom, pos, pos + 1, strand, pos, pos + 1))
    return ['\n'.join(lines) + '\n' for lines in reps], {f: '\n'.join(lines) + '\n' for f, lines in pred.items()}


def read_bed(text, counts):
    """readBed of hm_cluster_predict.py:20-41 with the two departures of the issue."""
    out = {}
    for no, line in enumerate(text.split('\n')[:-1]):
        counts['seen'] += 1
        if no == 0:
            counts['first_lines'] += 1
            continue
        line = line.strip()
        if len(line) <= 20:
            counts['short'] += 1
            continue
        f = line.split()
        assert len(f) == 11
        if f[5] not in '+-':
            counts['other_strand'] += 1
            continue
        if f[0] not in CONTIGS:
            counts['other_contig'] += 1
            continue
        if int(f[9]) == 0:
            counts['zero_coverage'] += 1
            continue
        key = (f[0], f[5], int(f[1]))
        assert key not in out
        out[key] = (min(int(f[9]), 65535), int(f[10]))
        counts['records'] += 1
    return out


def main():
    reps, pred_files = make_inputs()
    line_counts = [dict.fromkeys(('seen', 'records', 'first_lines', 'short', 'other_strand', 'other_contig', 'zero_coverage'), 0) for _ in range(R)]
    truth = [read_bed(t, c) for t, c in zip(reps, line_counts)]
    pred = {}
    for text in pred_files.values():
        for line in text.split('\n'):
            f = line.split()
            if f:
                e = pred.setdefault((f[0], f[5], int(f[1])), [0, 0])
                e[0] += int(f[9])
                e[1] += int(f[11])
    predicted = {k: (100 * m) // c for k, (c, m) in pred.items() if c >= PRED_COV}
    sites = sorted(set(truth[0]).intersection(*truth[1:]))
    T = len(THRESHOLDS)
    hist = np.zeros((3, T, 101), np.int64)
    unpredicted = np.zeros((3, T), np.int64)
    below = 0
    rows = []                                                                # (bucket, label, x, mean truth percentage)
    for k in sites:
        m = min(t[k][0] for t in truth)
        pcts = [t[k][1] for t in truth]
        bucket = sum(1 for c in THRESHOLDS if c <= m) - 1
        if bucket < 0:
            below += 1
            continue
        label = 1 if all(p >= METHYLATED for p in pcts) else 0 if all(p <= UNMETHYLATED for p in pcts) else 2
        if k in predicted:
            hist[label, bucket, predicted[k]] += 1
            rows.append((bucket, label, predicted[k], sum(pcts) / R))
        else:
            unpredicted[label, bucket] += 1
    with_truth = set(sites)
    untruthed = sum(1 for k in predicted if k not in with_truth)
    measures, report = {}, []
    for j, c in enumerate(THRESHOLDS):
        sel = [r for r in rows if r[0] >= j]
        two = [r for r in sel if r[1] < 2]
        label, score = np.array([r[1] for r in two]), np.array([r[2] for r in two], np.float64)
        assert 0 < label.sum() < len(label), 'a class is empty at threshold %d' % c
        fpr, tpr, _ = roc_curve(label, score)
        x, y = np.array([r[2] for r in sel], np.float64), np.array([r[3] for r in sel], np.float64)
        m = {'methylated': int(label.sum()), 'unmethylated': int(len(label) - label.sum()), 'methylated_unpredicted': int(unpredicted[1, j:].sum()),
             'unmethylated_unpredicted': int(unpredicted[0, j:].sum()), 'auc': float(auc(fpr, tpr)), 'ap': float(average_precision_score(label, score)),
             'n': len(sel), 'r': float(np.corrcoef(x, y)[0, 1]), 'rmse': float(math.sqrt(np.mean((x - y) ** 2)))}
        for key, digits in (('auc', 7), ('ap', 5), ('r', 5), ('rmse', 3)):      # no printed digit hangs on the last bits
            frac = (m[key] * 10 ** digits) % 1.0
            assert abs(frac - 0.5) > 1e-4, (key, m[key])
        measures[str(c)] = m
        report.append('raw cov>=%d methylated=%d unmethylated=%d methylated_unpredicted=%d unmethylated_unpredicted=%d auc=%.7f ap=%.5f n=%d r=%.5f rmse=%.3f'
                      % (c, m['methylated'], m['unmethylated'], m['methylated_unpredicted'], m['unmethylated_unpredicted'], m['auc'], m['ap'], m['n'], m['r'], m['rmse']))
    assert below > 0 and untruthed > 0 and (unpredicted.sum(axis=1) > 0).all() and (hist.sum(axis=2) > 0).all(), (below, untruthed, unpredicted, hist.sum(axis=2))
    case = {'options': {'chr': sorted(CONTIGS), 'cov': list(THRESHOLDS), 'methylated': METHYLATED, 'unmethylated': UNMETHYLATED, 'predCov': PRED_COV, 'Base': 'C'},
            'truth': reps, 'pred': pred_files, 'line_counts': line_counts, 'hist_nonzero': [[int(v) for v in k] + [int(hist[tuple(k)])] for k in np.argwhere(hist)], 'unpredicted': unpredicted.tolist(), 'below_threshold': below,
            'untruthed': untruthed, 'measures': measures, 'report': report}
    with open(os.path.join(HERE, 'bsperf_case.json'), 'w') as fh:
        json.dump(case, fh, separators=(',', ':'))
    print('\n'.join(report))
    print(os.path.getsize(os.path.join(HERE, 'bsperf_case.json')), 'bytes')


if __name__ == '__main__':
    main()
