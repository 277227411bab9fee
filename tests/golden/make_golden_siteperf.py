#!/usr/bin/env python
"""Regenerates tests/golden/siteperf_cases.json: small synthetic inputs and the lines the REFERENCE's own DeepMod_tools/cal_EcoliDetPerf.py prints
for them.

    python tests/golden/make_golden_siteperf.py <checkout of the reference DeepMod>

The reference script needs sklearn, scipy and matplotlib, and imports rpy2 (R, ggplot2) without using it for what it prints: an empty stub
package `rpy2` is created in the temporary directory and put on PYTHONPATH.  The JSON holds data only: the FASTA and BED texts and the printed
lines from the first `basetype=` line on, with the figure folder replaced by {FIG}.
Cases (tests/test_siteperf_host.py, tests/test_gpu_siteperf.py):
  1  Cg 0, no region: a 3,000-bp contig, run files for both strands, two control folders at different depths, the second on four fifths of the first one's positions
  2  gAtc 1: A files, a second contig; one control file holds both contigs
  3  gaAttc 2, a region whose edges fall on a site and next to one; the control files hold in-region lines only, the run files keep the others
  4  Cg 0 where no run line on a site reaches coverage 5: the positive class is empty at that threshold
  5  the departure: control files with odd runs of out-of-region lines before in-region ones, recorded from the reference as it is
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def contig(rng, n, motif, every):
    seq = rng.choice(list('ACGT'), n)
    m = len(motif)
    p = int(rng.integers(0, every))
    while p + m <= n:                                   # plant the motif so that long ones occur, on both strands' terms (palindromes or not)
        seq[p:p + m] = list(motif.upper())
        p += m + int(rng.integers(1, every))
    return ''.join(seq)


def sites(seq, motif, k):
    pat = motif.upper()
    rc = ''.join(COMP[c] for c in reversed(pat))
    m = len(pat)
    plus = {i for i in range(len(seq)) if i - k >= 0 and seq[i - k:i - k + m] == pat}
    minus = {i for i in range(len(seq)) if i - (m - 1 - k) >= 0 and seq[i - (m - 1 - k):i - (m - 1 - k) + m] == rc}
    return plus, minus


def bed_lines(rng, name, seq, motif, k, strand, keep, methylated, max_cov, other_base=0.0, positions=None, keep_other=0.08):
    """Lines as `detect` lays them out (one separator): the positions whose base on `strand` is B - sites thinned to `keep`, the others to
    `keep_other`, so that the file stays small - and a few lines of another base (`other_base`)."""
    B = motif[k]
    plus, minus = sites(seq, motif, k)
    site = plus if strand == '+' else minus
    out = []
    for i in (range(len(seq)) if positions is None else positions):
        b = seq[i] if strand == '+' else COMP[seq[i]]
        if b != B:
            if i in site or rng.random() >= other_base:
                continue                                 # never on a site (the reference's control reader fails there)
        elif rng.random() >= (keep if i in site else keep_other):
            continue
        cov = int(rng.integers(0, max_cov + 1))
        p = (0.3 + 0.7 * rng.random()) if (methylated and i in site) else 0.6 * rng.random() ** 1.5
        mod = int(rng.binomial(cov, p)) if cov else 0
        pct = int(mod * 100 / cov) if cov else 0
        out.append('%s %d %d %s %d %s %d %d 0,0,0 %d %d %d' % (name, i, i + 1, b, min(cov, 1000), strand, i, i + 1, cov, pct, mod))
    return out


def text(lines):
    return ''.join(ln + '\n' for ln in lines)


def make_cases():
    cases = []
    rng = np.random.default_rng(20261019)
    both = lambda *a, **kw: bed_lines(rng, *a[:4], '+', *a[4:], **kw) + bed_lines(rng, *a[:4], '-', *a[4:], **kw)
    # 1
    seq = contig(rng, 3000, 'CG', 60)
    run = {'mod_pos.plus.C.bed': text(bed_lines(rng, 'c1', seq, 'Cg', 0, '+', 0.2, True, 30, 0.01, keep_other=0.03)),
           'sub/mod_pos.minus.C.bed': text(bed_lines(rng, 'c1', seq, 'Cg', 0, '-', 0.2, True, 30, 0.01, keep_other=0.03))}
    first = [bed_lines(rng, 'c1', seq, 'Cg', 0, st, 0.3, False, 12, keep_other=0.03) for st in '+-']
    again = [bed_lines(rng, 'c1', seq, 'Cg', 0, st, 0.8, False, 8, 0.005, [int(ln.split()[1]) for ln in lines], keep_other=0.8) for st, lines in zip('+-', first)]
    c1 = {'mod_pos.c1.C.bed': text(first[0] + first[1])}
    c2 = {'a/b/mod_pos.c2.C.bed': text(again[0] + again[1])}          # the second control covers four fifths of the first one's positions
    cases.append({'name': 'cg', 'motif': 'Cg', 'k': 0, 'chr': '', 'start': -1, 'end': -1, 'fasta': '>c1 first contig\n' + wrap(seq), 'run': run, 'controls': [c1, c2]})
    # 2
    s1, s2 = contig(rng, 400, 'GATC', 30), contig(rng, 300, 'GATC', 30)
    run = {'mod_pos.one.A.bed': text(both('one', s1, 'gAtc', 1, 0.6, True, 20, 0.02)),
           'x/mod_pos.two.A.bed': text(both('two', s2, 'gAtc', 1, 0.6, True, 20))}
    c1 = {'mod_pos.both.A.bed': text(bed_lines(rng, 'two', s2, 'gAtc', 1, '+', 0.6, False, 10) + bed_lines(rng, 'one', s1, 'gAtc', 1, '-', 0.6, False, 10) +
                                      bed_lines(rng, 'one', s1, 'gAtc', 1, '+', 0.6, False, 10) + bed_lines(rng, 'two', s2, 'gAtc', 1, '-', 0.6, False, 10))}
    cases.append({'name': 'gatc', 'motif': 'gAtc', 'k': 1, 'chr': '', 'start': -1, 'end': -1, 'fasta': '>one\n' + wrap(s1) + '>two\tsecond\n' + wrap(s2), 'run': run,
                  'controls': [c1]})
    # 3
    seq = contig(rng, 600, 'GAATTC', 30)
    plus, minus = sites(seq, 'gaAttc', 2)
    ps = sorted(plus)
    start, end = ps[3], ps[-4] + 1                       # the first edge on a '+' site, the last edge one past a '+' site
    inside = range(start, end + 1)
    run = {'mod_pos.r.A.bed': text(both('eco', seq, 'gaAttc', 2, 0.6, True, 20, 0.02))}
    c1 = {'mod_pos.c.A.bed': text(both('eco', seq, 'gaAttc', 2, 0.6, False, 10, 0.0, inside))}
    c2 = {'d/mod_pos.c.A.bed': text(bed_lines(rng, 'eco', seq, 'gaAttc', 2, '-', 0.6, False, 10, 0.0, inside) + bed_lines(rng, 'eco', seq, 'gaAttc', 2, '+', 0.6, False, 10, 0.0, inside))}
    cases.append({'name': 'region', 'motif': 'gaAttc', 'k': 2, 'chr': 'eco', 'start': start, 'end': end, 'fasta': '>eco the only contig\n' + wrap(seq), 'run': run,
                  'controls': [c1, c2]})
    # 4
    seq = contig(rng, 300, 'CG', 25)
    run = {'mod_pos.low.C.bed': text(both('ctg', seq, 'Cg', 0, 0.6, True, 4))}
    c1 = {'mod_pos.c.C.bed': text(both('ctg', seq, 'Cg', 0, 0.6, False, 15))}
    cases.append({'name': 'empty_class', 'motif': 'Cg', 'k': 0, 'chr': '', 'start': -1, 'end': -1, 'fasta': '>ctg\n' + wrap(seq), 'run': run, 'controls': [c1]})
    # 5
    seq = contig(rng, 400, 'CG', 25)
    start, end = 131, 300
    run = {'mod_pos.r.C.bed': text(both('ctg', seq, 'Cg', 0, 0.6, True, 20))}
    plus_lines = bed_lines(rng, 'ctg', seq, 'Cg', 0, '+', 0.6, False, 12)
    minus_lines = bed_lines(rng, 'ctg', seq, 'Cg', 0, '-', 0.6, False, 12)
    before = [ln for ln in plus_lines if int(ln.split()[1]) < start]
    if len(before) % 2 == 0:
        plus_lines = plus_lines[1:]                      # an odd run of out-of-region lines before the first in-region line
    c1 = {'mod_pos.c.C.bed': text(plus_lines + minus_lines)}
    cases.append({'name': 'departure', 'motif': 'Cg', 'k': 0, 'chr': 'ctg', 'start': start, 'end': end, 'fasta': '>ctg\n' + wrap(seq), 'run': run, 'controls': [c1]})
    return cases


def wrap(seq, width=70):
    return ''.join(seq[i:i + width] + '\n' for i in range(0, len(seq), width))


def write_tree(root, files):
    for rel, content in files.items():
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(content)


def run_reference(script, case, tmp):
    root = os.path.join(tmp, case['name'])
    fig = os.path.join(root, 'fig')
    os.makedirs(fig)
    write_tree(os.path.join(root, 'run'), case['run'])
    controls = []
    for i, files in enumerate(case['controls']):
        controls.append(os.path.join(root, 'control%d' % i))
        write_tree(controls[-1], files)
    with open(os.path.join(root, 'ref.fa'), 'w') as fh:
        fh.write(case['fasta'])
    env = dict(os.environ, PYTHONPATH=os.path.join(tmp, 'stub') + os.pathsep + os.environ.get('PYTHONPATH', ''), MPLBACKEND='Agg')
    out = subprocess.run([sys.executable, '-W', 'ignore', script, os.path.join(root, 'run'), os.path.join(root, 'ref.fa'), case['motif'], str(case['k']), case['chr'],
                          str(case['start']), str(case['end']), fig, ','.join(controls)], env=env, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit('the reference failed on case %s:\n%s' % (case['name'], out.stderr[-3000:]))
    lines = out.stdout.splitlines()
    first = next(i for i, ln in enumerate(lines) if ln.startswith('basetype='))
    return [ln.replace(fig, '{FIG}') for ln in lines[first:]]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    script = os.path.join(sys.argv[1], 'DeepMod_tools', 'cal_EcoliDetPerf.py')
    cases = make_cases()
    with tempfile.TemporaryDirectory() as tmp:
        stub = os.path.join(tmp, 'stub', 'rpy2', 'robjects')
        os.makedirs(stub)
        open(os.path.join(tmp, 'stub', 'rpy2', '__init__.py'), 'w').close()
        open(os.path.join(stub, '__init__.py'), 'w').close()
        with open(os.path.join(stub, 'packages.py'), 'w') as fh:
            fh.write('def importr(name):\n    return None\n')
        for case in cases:
            case['lines'] = run_reference(script, case, tmp)
            print(case['name'], len(case['lines']), 'lines')
    import sklearn
    doc = {'reference': 'DeepMod_tools/cal_EcoliDetPerf.py', 'sklearn': sklearn.__version__, 'cases': cases}
    with open(os.path.join(HERE, 'siteperf_cases.json'), 'w') as fh:
        json.dump(doc, fh, indent=0)
    print(os.path.getsize(os.path.join(HERE, 'siteperf_cases.json')), 'bytes')


if __name__ == '__main__':
    main()
