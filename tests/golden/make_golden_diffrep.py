#!/usr/bin/env python
"""TEST INFRASTRUCTURE - not part of the product.  Writes tests/golden/diffrep_case.json: about 300 tested keys of `diffmod --replicates 1` (the
planted and random keys of tests/diffrep_synth.py over its replicate shapes, at the default least replicate counts and one below) with D, phi and p of
diffmod.rep_exact, D once more from mpmath's logarithms at 40 digits, and two second witnesses of the incomplete beta at the oracle's own nu and F = D / phi: scipy.stats.f.sf(F, 1, nu) on the float F,
and mpmath.betainc(nu / 2, 1 / 2, 0, nu / (nu + F), regularized=True) at 40 digits on the 50-digit F.  Under `command`: the report and the document the command
writes under RepHostEngine on the synthetic case of tests/diffrep_synth.py, for three option sets (command_case; `--command-only` rewrites that key alone
and needs neither scipy nor mpmath).  Needs scipy and mpmath; the tests read the JSON only.

    python tests/golden/make_golden_diffrep.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


PATH = os.path.join(ROOT, 'tests', 'golden', 'diffrep_case.json')
COMMAND_CASES = (('default', {}, (3, 2)), ('all', {'all': 1}, (3, 2)), ('low', {'all': 1, 'minReps': '2,2'}, (2, 2)))


def command_case():
    """{fileid: {'txt', 'json'}} of diffrep_synth.run_command for COMMAND_CASES: the bytes a later driver of the command has to write."""
    import tempfile

    import diffrep_synth as synth
    from deepmod_amd import diffmod
    out = {}
    with tempfile.TemporaryDirectory() as root:
        case = synth.write_case(root)
        for fileid, options, (a, b) in COMMAND_CASES:
            out[fileid] = synth.run_command(case, root, diffmod.RepHostEngine(synth.COV, 1.0 if options.get('all') else synth.FDR, a, b), fileid, **options)
    return out


def main():
    if '--command-only' in sys.argv:
        doc = json.load(open(PATH))
        doc['command'] = command_case()
        with open(PATH, 'w') as fh:
            json.dump(doc, fh, indent=0)
        return
    import mpmath
    import scipy
    from scipy import stats

    import diffrep_synth as synth
    from deepmod_amd import diffmod
    mpmath.mp.dps = 40
    rows, worst = [], {'scipy': 0.0, 'mpmath': 0.0}
    for KA, KB in synth.SHAPES:
        for a, b in sorted({(KA, KB), synth.low_min_reps(KA, KB)}):
            keys = synth.planted_keys(KA, KB, a, b) + synth.random_keys(KA, KB, 7 * KA + KB, 26 if (a, b) == (KA, KB) else 8)
            for key in keys:
                fate, ua, ub = synth.used_of(key, KA, synth.COV, a, b)
                if fate != 0:
                    continue
                e = diffmod.rep_exact(tuple(ua), tuple(ub))
                F = e['D'] / e['phi']
                row = {'shape': [KA, KB], 'minReps': [a, b], 'c': list(key[0]), 'm': list(key[1]), 'nu': e['nu'], 'equal': e['equal'], 'phi': float(e['phi']),
                       'F': float(F), 'p': float(e['p'])}
                if not e['equal']:
                    def h(M, C):
                        return sum(k * mpmath.log(mpmath.mpf(k) / C) for k in (M, C - M) if k > 0)
                    row['D'] = float(e['D'])
                    row['D_mpmath'] = float(2 * (h(e['mA'], e['cA']) + h(e['mB'], e['cB']) - h(e['mA'] + e['mB'], e['cA'] + e['cB'])))
                    row['scipy'] = float(stats.f.sf(float(F), 1, e['nu']))
                    row['mpmath'] = float(mpmath.betainc(mpmath.mpf(e['nu']) / 2, mpmath.mpf(1) / 2, 0, e['nu'] / (e['nu'] + mpmath.mpf(str(F))), regularized=True))
                    for w in worst:
                        worst[w] = max(worst[w], abs(row[w] - row['p']) / row['p'])
                rows.append(row)
    doc = {'made_with': {'scipy': scipy.__version__, 'mpmath': mpmath.__version__}, 'cov': synth.COV, 'worst_relative': worst, 'keys': rows, 'command': command_case()}
    path = PATH
    with open(path, 'w') as fh:
        json.dump(doc, fh, indent=0)
    print('%d keys, worst relative difference to the oracle: %r -> %s' % (len(rows), worst, path))


if __name__ == '__main__':
    main()
