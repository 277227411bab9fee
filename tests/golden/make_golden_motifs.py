#!/usr/bin/env python
"""Regenerates tests/golden/motifs_case.json: a small input of the counting half of `motifs` and what its definition makes of it, computed WITHOUT
deepmod_amd and without numpy: the tables are plain dicts {position: (coverage, modified)}, the oriented letters are looked up one by one in the
reference string, and the fate of a key is a chain of if statements in the order of the rules.

    python tests/golden/make_golden_motifs.py

Two contigs (chrA of 320 bases with two N and two lower-case letters in it, chrB of 70), base A, cov 5, min_pct 50, max_ctrl_pct 10, flanks (3,3)
and (2,3), each with and without controls: four cases over the same tables.  The records are drawn so that coverages sit on both sides of cov in
the sample and in the controls, percentages on both sides of min_pct and max_ctrl_pct, and some records lie on letters that are not the base.  The
JSON holds data only: the reference, the records, the options, and per case the non-zero bins, the counters and off_base per contig.  The script
stops if a counter of a case is zero on a strand (no_control: of the cases with controls).
"""
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
BASE, COV, MIN_PCT, MAX_CTRL_PCT = 'A', 5, 50, 10
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
KEYS = ('tested', 'modified', 'shallow', 'no_control', 'edge')


def make_reference(rng):
    ref = {}
    for name, length in (('chrA', 320), ('chrB', 70)):
        letters = []
        while len(letters) < length:
            letters += list('GATC') if rng.random() < 0.25 else [rng.choice('ACGT')]
        ref[name] = letters[:length]
    ref['chrA'][40], ref['chrA'][201] = 'N', 'N'
    ref['chrA'][90], ref['chrA'][150] = 'a', 't'
    ref['chrA'][0], ref['chrA'][-1] = 'A', 'T'                          # a base on either strand whose context leaves the contig
    ref['chrB'][1], ref['chrB'][-2] = 'T', 'A'
    return {k: ''.join(v) for k, v in ref.items()}


def make_records(rng, ref, coverages, fractions, density):
    """{contig: {strand: {position: [coverage, modified]}}}"""
    out = {}
    for name, seq in ref.items():
        out[name] = {'+': {}, '-': {}}
        for strand in '+-':
            for p in range(len(seq)):
                if rng.random() < density:
                    cov = rng.choice(coverages)
                    out[name][strand][p] = [cov, min(cov, int(cov * rng.choice(fractions) + 0.5))]
    return out


def oriented(seq, strand, p, j):
    """The oriented letter at offset j of position p (None: outside the contig or none of A, C, G, T)."""
    q = p + j if strand == '+' else p - j
    if q < 0 or q >= len(seq) or seq[q] not in COMP:
        return None
    return seq[q] if strand == '+' else COMP[seq[q]]


def count(ref, sample, control, up, down):
    hist, contigs = {}, {}
    for name, seq in ref.items():
        contigs[name] = {s: dict.fromkeys(KEYS + ('off_base',), 0) for s in '+-'}
        for strand in '+-':
            c = contigs[name][strand]
            for p in range(len(seq)):
                cov, mod = sample[name][strand].get(p, (0, 0))
                if oriented(seq, strand, p, 0) != BASE:
                    if cov > 0:
                        c['off_base'] += 1
                    continue
                ctx = [oriented(seq, strand, p, j) for j in range(-up, down + 1) if j != 0]
                if None in ctx:
                    c['edge'] += 1
                    continue
                if cov < COV:
                    c['shallow'] += 1
                    continue
                ccov, cmod = (0, 0) if control is None else control[name][strand].get(p, (0, 0))
                if control is not None and ccov < COV:
                    c['no_control'] += 1
                    continue
                word = ''.join(ctx)
                word = word[:up].lower() + BASE + word[up:].lower()
                hist.setdefault(word, [0, 0])
                hist[word][0] += 1
                c['tested'] += 1
                if 100 * mod // cov >= MIN_PCT and (control is None or 100 * cmod // ccov <= MAX_CTRL_PCT):
                    hist[word][1] += 1
                    c['modified'] += 1
    return hist, contigs


def main():
    rng = random.Random(20)
    ref = make_reference(rng)
    sample = make_records(rng, ref, (1, 4, 5, 6, 20, 40), (0.0, 0.2, 0.5, 0.9, 1.0), 0.8)
    control = make_records(rng, ref, (2, 4, 5, 9, 30), (0.0, 0.0, 0.1, 0.12, 0.5), 0.7)
    cases = []
    for up, down in ((3, 3), (2, 3)):
        for ctrl in (False, True):
            hist, contigs = count(ref, sample, control if ctrl else None, up, down)
            for name in ('chrA',):
                for strand in '+-':
                    for k, v in contigs[name][strand].items():
                        assert v > 0 or (k == 'no_control' and not ctrl), (up, down, ctrl, name, strand, k)
            cases.append({'flank': [up, down], 'controls': ctrl, 'contexts': hist, 'contigs': contigs})
    doc = {'options': {'Base': BASE, 'cov': COV, 'min_pct': MIN_PCT, 'max_ctrl_pct': MAX_CTRL_PCT}, 'reference': ref, 'sample': sample, 'control': control,
           'cases': cases}
    with open(os.path.join(HERE, 'motifs_case.json'), 'w') as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
    print('wrote motifs_case.json:', {(tuple(c['flank']), c['controls']): sum(v[0] for v in c['contexts'].values()) for c in cases})


if __name__ == '__main__':
    main()
