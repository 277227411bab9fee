"""TEST INFRASTRUCTURE - not part of the product.  Writes tests/golden/diffmod_case.json:

  keys      300 random keys (coverages 1-300, tests/diffmod_synth.random_keys) and the keys of the GPU sweep that are tested, each with the p of
            diffmod.exact_p (exact rationals) and, as a second witness, the p of scipy.stats.fisher_exact - recorded here so that no test imports scipy
  contig    those keys laid out on both strands of a contig with cov 5 and alpha 0.05: the counters, the p histogram and the records
  command   the two outputs of the command under HostEngine on the synthetic case of tests/diffmod_synth.write_case

    python tests/golden/make_golden_diffmod.py

It checks what the tests rely on: that scipy and the exact rationals agree to 1e-12, that the generator dropped 1 % of the random keys at most, and
that every q of the command case is 1e-3 relative or more away from --fdr."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import diffmod_synth  # noqa: E402
from deepmod_amd import diffmod  # noqa: E402

MAX_TOTAL, SMALL = 1 << 20, 256
LENGTH, TILE = 2100, 1024


def main():
    from scipy.stats import fisher_exact
    keys, dropped = diffmod_synth.random_keys(3, 300)
    assert dropped <= 3, dropped
    special = [k for k in diffmod_synth.sweep_keys(SMALL, MAX_TOTAL) if k[0] >= diffmod_synth.COV and k[2] >= diffmod_synth.COV and k[0] + k[2] <= MAX_TOTAL]
    rows, worst, worst_large = [], 0.0, 0.0
    for cA, mA, cB, mB in keys + special:
        exact = diffmod.exact_p(cA, mA, cB, mB)
        witness = float(fisher_exact([[mA, cA - mA], [mB, cB - mB]])[1])
        if exact >= 1e-290 and cA + cB <= 4096:
            worst = max(worst, abs(witness - exact) / exact)
        elif exact >= 1e-290:
            worst_large = max(worst_large, abs(witness - exact) / exact)
        rows.append({'key': [cA, mA, cB, mB], 'exact': exact, 'scipy': witness})
    assert worst <= 1e-12 and worst_large <= 1e-6, (worst, worst_large)
    recs = diffmod_synth.layout(keys[:120] + diffmod_synth.sweep_keys(SMALL, MAX_TOTAL), LENGTH, TILE, 1)
    eng = diffmod.HostEngine(diffmod_synth.COV, diffmod_synth.FDR)
    tabs = diffmod_synth.host_tables(recs['sample'], LENGTH) + diffmod_synth.host_tables(recs['control'], LENGTH)
    counters, rec = eng.run(*tabs)
    contig = {'length': LENGTH, 'cov': diffmod_synth.COV, 'alpha': diffmod_synth.FDR,
              'sample': [a.tolist() for a in recs['sample']], 'control': [a.tolist() for a in recs['control']],
              'counters': counters.tolist(), 'hist': eng.fetch_hist().tolist(), 'records': {k: v.tolist() for k, v in rec.items()}}
    with tempfile.TemporaryDirectory() as root:
        case = diffmod_synth.write_case(root)
        command = diffmod_synth.run_command(case, root, diffmod.HostEngine(diffmod_synth.COV, diffmod_synth.FDR), 'golden')
        everything = diffmod_synth.run_command(case, root, diffmod.HostEngine(diffmod_synth.COV, 1.0), 'golden_all', all=1)
    gaps = [abs(r[-1] - diffmod_synth.FDR) / diffmod_synth.FDR for r in diffmod_synth.parse_report(everything['txt'])]
    assert min(gaps) >= 1e-3, min(gaps)
    doc = {'keys': rows, 'scipy_worst_relative': worst, 'scipy_worst_relative_above_4096': worst_large, 'dropped_of_300': dropped, 'contig': contig, 'command': command, 'smallest_q_gap': min(gaps)}
    with open(os.path.join(HERE, 'diffmod_case.json'), 'w') as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
    print('scipy against exact: %.3g; dropped %d of 300; smallest |q - fdr| / fdr: %.3g; %d lines listed of m = %d' %
          (worst, dropped, min(gaps), command['json']['listed'], command['json']['m']))


if __name__ == '__main__':
    main()
