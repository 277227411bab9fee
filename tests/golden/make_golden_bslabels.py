#!/usr/bin/env python
"""Regenerates tests/golden/bslabels_case.json: a small input of `bslabels` and what its definition makes of it, computed WITHOUT deepmod_amd: the
replicates are read with split() and int() into plain dicts (readBed's rules), a site is found by comparing the reference string with the motif
and its reverse complement letter by letter, and the class of a key is three if statements.

    python tests/golden/make_golden_bslabels.py

Three contigs of the run (chrA, chrB, and chrE, which has sites and no truth at all; chrC is in the replicates and not requested), two replicates,
both strands, motif CG with the modified base at offset 0, cov 5, methylated 90, unmethylated 10 (above 0, so that unmethylated + 1 is another
percentage than 1 above the least).  Forced in on chrA: every class on either strand, a key off the motif, a key in one replicate only, coverage
exactly cov and cov - 1, percentages exactly methylated, methylated - 1, unmethylated and unmethylated + 1, a coverage above 65,535.  The JSON holds
data only: the reference, the replicates' texts, the options, the three texts per contig, the key sets and the counts.  The script stops if a class
is empty on a strand of chrA.
"""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
COV, METHYLATED, UNMETHYLATED, R = 5, 90, 10, 2
MOTIF, K = 'CG', 0
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
HEADER = 'chrom\tstart\tend\tname\tscore\tstrand\tthickStart\tthickEnd\tcolor\tcoverage\tpercentage'


def make_reference(rng):
    ref = {}
    for name, length in (('chrA', 400), ('chrB', 90), ('chrC', 40), ('chrE', 33)):
        letters = []
        while len(letters) < length:
            letters += list('CG') if rng.random() < 0.3 else [rng.choice('ACGT')]
        ref[name] = ''.join(letters[:length])
    ref['chrB'] = ref['chrB'][:-1] + 'C'                                 # a C at the contig's end: no G follows, no site
    return ref


def is_site(seq, strand, pos):
    """The motif lies on the strand with its modified base at pos."""
    m = len(MOTIF)
    if strand == '+':
        first, pat = pos - K, MOTIF
    else:
        first, pat = pos - (m - 1 - K), ''.join(COMP[c] for c in reversed(MOTIF))
    return first >= 0 and first + m <= len(seq) and all(seq[first + j] == pat[j] for j in range(m))


def line(chrom, pos, strand, cov, pct, sep):
    return sep.join([chrom, str(pos), str(pos + 1), '.', str(min(cov, 1000)), strand, str(pos), str(pos + 1), '0,0,0', str(cov), str(pct)])


def make_replicates(rng, ref):
    reps = [[HEADER] for _ in range(R)]
    sites = {(c, s): [p for p in range(len(seq)) if is_site(seq, s, p)] for c, seq in ref.items() for s in '+-'}
    # (coverage, percentage) of replicate 0 and 1 (None: no record), in this order on the first sites of either strand of chrA
    forced = [((30, 95), (30, 100)),                                      # fulmod
              ((COV, METHYLATED), (70000, METHYLATED)),                   # fulmod: coverage exactly cov, percentage exactly methylated, a saturated coverage
              ((COV - 1, 100), (30, 100)),                                # anymod: coverage cov - 1
              ((30, METHYLATED - 1), (30, 100)),                          # anymod: methylated - 1
              ((30, 0), (30, 0)),                                         # nomod
              ((COV, UNMETHYLATED), (COV, 0)),                            # nomod: exactly unmethylated
              ((30, UNMETHYLATED + 1), (30, 0)),                          # anymod: unmethylated + 1
              ((COV - 1, 0), (30, 0)),                                    # anymod
              ((30, 100), None),                                          # anymod: one replicate only
              (None, (30, 0)),                                            # anymod
              ((30, 100), (30, 0)),                                       # anymod: the replicates disagree
              ((30, 50), (30, 50))]                                       # anymod: partial
    for strand in '+-':
        for p, pair in zip(sites[('chrA', strand)], forced):
            for r, rec in enumerate(pair):
                if rec:
                    reps[r].append(line('chrA', p, strand, rec[0], rec[1], '\t' if r == 0 else ' '))
        off = [p for p in range(len(ref['chrA'])) if not is_site(ref['chrA'], strand, p)][3]
        for r in range(R):                                                # a key off the motif, fully methylated in both
            reps[r].append(line('chrA', off, strand, 30, 100, '\t' if r == 0 else ' '))
    for chrom in ('chrA', 'chrB', 'chrC'):
        for strand in '+-':
            skip = len(forced) if chrom == 'chrA' else 0
            for p in sites[(chrom, strand)][skip:]:
                kind = rng.choice(['ful', 'no', 'mid', 'mixed', 'none'])
                if kind == 'none':
                    continue
                for r in range(R):
                    if rng.random() < 0.1:
                        continue
                    cov = rng.choice([0, 1, 4, 5, 6, 9, 30, 70000])
                    pct = {'ful': rng.randint(88, 100), 'no': rng.choice([0, 0, 0, 5, 10, 11]), 'mid': rng.randint(12, 87), 'mixed': rng.choice([0, 89, 90, 100])}[kind]
                    reps[r].append(line(chrom, p, strand, cov, pct, '\t' if r == 0 else ' '))
        for r in range(R):                                                # lines the rules pass over: another strand, short lines
            reps[r].append('\t'.join([chrom, '7', '8', '.', '3', '.', '7', '8', '0,0,0', '3', '100']))
            reps[r].append('%s 1 2 . 1 +' % chrom)
            reps[r].append('')
    return ['\n'.join(lines) + '\n' for lines in reps]


def read_bed(text, names, counts):
    """readBed of hm_cluster_predict.py:20-41 with bsperf's two departures -> {(contig, strand, position): (coverage, percentage)}."""
    out = {}
    for no, ln in enumerate(text.split('\n')[:-1]):
        counts['seen'] += 1
        if no == 0:
            counts['first_lines'] += 1
            continue
        ln = ln.strip()
        if len(ln) <= 20:
            counts['short'] += 1
            continue
        f = ln.split()
        assert len(f) == 11
        if f[5] not in '+-':
            counts['other_strand'] += 1
            continue
        if f[0] not in names:
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
    rng = random.Random(19)
    ref = make_reference(rng)
    texts = make_replicates(rng, ref)
    names = ['chrA', 'chrB', 'chrE']
    lines = [dict.fromkeys(('seen', 'records', 'first_lines', 'short', 'other_strand', 'other_contig', 'zero_coverage'), 0) for _ in range(R)]
    truth = [read_bed(t, names, c) for t, c in zip(texts, lines)]
    out = {'options': {'cov': COV, 'methylated': METHYLATED, 'unmethylated': UNMETHYLATED, 'motif': MOTIF, 'ModinMotif': K, 'Base': 'C', 'chr': names},
           'reference': ref, 'replicates': texts, 'lines': lines, 'contigs': {}}
    for chrom in names:
        seq = ref[chrom]
        keys = {w: [] for w in ('fulmod', 'anymod', 'nomod')}
        counts = {s: dict.fromkeys(('fulmod', 'anymod', 'nomod', 'off_motif', 'sites_without_truth'), 0) for s in '+-'}
        for pos in range(len(seq)):
            for strand in '+-':
                recs = [t.get((chrom, strand, pos)) for t in truth]
                site = is_site(seq, strand, pos)
                if all(r is None for r in recs):
                    counts[strand]['sites_without_truth'] += 1 if site else 0
                    continue
                if not site:
                    counts[strand]['off_motif'] += 1
                    continue
                which = 'anymod'
                if all(r is not None for r in recs) and min(r[0] for r in recs) >= COV:
                    if all(r[1] >= METHYLATED for r in recs):
                        which = 'fulmod'
                    elif all(r[1] <= UNMETHYLATED for r in recs):
                        which = 'nomod'
                keys[which].append([strand, pos])
                counts[strand][which] += 1
        if chrom == 'chrA':
            assert all(counts[s][w] > 0 for s in '+-' for w in counts[s]), counts
        out['contigs'][chrom] = {'counts': counts, 'keys': keys, 'texts': {w: ''.join('%s %s %d\n' % (chrom, s, p) for s, p in v) for w, v in keys.items()}}
    with open(os.path.join(HERE, 'bslabels_case.json'), 'w') as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write('\n')
    for chrom in names:
        print(chrom, {s: out['contigs'][chrom]['counts'][s] for s in '+-'})


if __name__ == '__main__':
    main()
