"""CPU: `diffmod` without a GPU.  diffmod.HostEngine (exact rationals) and the compiled host twin dm_diffmod_test_host against
tests/golden/diffmod_case.json (tests/golden/make_golden_diffmod.py; the p-values of scipy.stats.fisher_exact are recorded there as a second witness),
the symmetries of the test, bh_qvalues against its definition, the command under HostEngine on the synthetic case of tests/diffmod_synth.py, the
refusals of the command line, and the host twin under the address sanitizer (tests/diffmod_driver.cpp).  The bound on p is the derived one of
DESIGN.md 21 (diffmod_synth.check_p): relative 1e-9 for cA + cB <= 4096, 1e-6 above, and <= 1e-289 for an exact p below 1e-290."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import diffmod

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import diffmod_synth  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'diffmod_case.json')))
COV, FDR = diffmod_synth.COV, diffmod_synth.FDR


def twin_p(keys, cov=1):
    """p of every key through the compiled twin: the keys on consecutive positions of the '+' strand, alpha 1."""
    a = np.array(keys, np.int64).reshape(-1, 4)
    z = np.zeros(len(a), np.int64)
    counters, hist, rec = diffmod.host_routine(cov, 1.0, (a[:, 0], a[:, 1]), (z, z), (a[:, 2], a[:, 3]), (z, z))
    assert counters[0, 0] == len(a) == len(rec['p']) == hist.sum() and rec['pos'].tolist() == list(range(len(a)))
    return rec['p']


def test_exact_p_and_host_twin_equal_the_golden_keys(hip_lib):
    rows = GOLDEN['keys']
    assert len(rows) >= 300 and GOLDEN['dropped_of_300'] <= 3 and GOLDEN['scipy_worst_relative'] <= 1e-12
    keys = [tuple(r['key']) for r in rows]
    got = twin_p(keys)
    seen_large = seen_tiny = 0
    for r, key, p in zip(rows, keys, got.tolist()):
        exact = diffmod.exact_p(*key)
        assert exact == r['exact'], key                               # the oracle itself has not moved
        if exact >= 1e-290 and key[0] + key[2] <= 4096:
            assert abs(r['scipy'] - exact) <= 1e-12 * exact, key      # the second witness
        diffmod_synth.check_p(p, exact, key[0] + key[2], key)
        seen_large += key[0] + key[2] > 4096
        seen_tiny += exact < 1e-290
    assert seen_large >= 3 and seen_tiny >= 1 and any(k[0] + k[2] == diffmod.max_total() for k in keys)


def golden_contig_tables():
    c = GOLDEN['contig']
    sample, control = (tuple(np.array(a, np.int64) for a in c[k]) for k in ('sample', 'control'))
    return c, diffmod_synth.host_tables(sample, c['length']) + diffmod_synth.host_tables(control, c['length'])


def test_host_engine_and_host_twin_equal_the_golden_contig(hip_lib):
    c, tabs = golden_contig_tables()
    eng = diffmod.HostEngine(c['cov'], c['alpha'])
    counters, rec = eng.run(*tabs)
    assert counters.tolist() == c['counters'] and eng.fetch_hist().tolist() == c['hist']
    assert {k: v.tolist() for k, v in rec.items()} == c['records']
    assert all(v > 0 for row in c['counters'] for v in row)           # every fate, on both strands
    assert sum(c['hist']) == sum(row[0] for row in c['counters']) and len(c['records']['p']) > 0
    key = 2 * rec['pos'].astype(np.int64) + rec['strand']
    assert (np.diff(key) > 0).all()                                   # key order: ascending position, '+' before '-'
    counters2, hist2, rec2 = diffmod.host_routine(c['cov'], c['alpha'], *tabs)
    assert counters2.tolist() == c['counters'] and hist2.tolist() == c['hist']
    for k in ('pos', 'strand', 'cA', 'mA', 'cB', 'mB'):
        assert rec2[k].tolist() == c['records'][k], k
    for p, exact, cA, cB in zip(rec2['p'].tolist(), c['records']['p'], c['records']['cA'], c['records']['cB']):
        diffmod_synth.check_p(p, exact, cA + cB)
    # the engine accumulates until reset
    eng.run(*tabs)
    assert eng.counters.tolist() == (2 * np.array(c['counters'])).tolist() and eng.fetch_hist().tolist() == (2 * np.array(c['hist'])).tolist()
    eng.reset()
    assert not eng.counters.any() and not eng.fetch_hist().any()


def test_symmetries(hip_lib):
    keys, dropped = diffmod_synth.random_keys(17, 60, 120)
    assert dropped <= 1
    swapped = [(cB, mB, cA, mA) for cA, mA, cB, mB in keys]
    flipped = [(cA, cA - mA, cB, cB - mB) for cA, mA, cB, mB in keys]
    base, sw, fl = twin_p(keys), twin_p(swapped), twin_p(flipped)
    for i, key in enumerate(keys):
        exact = diffmod.exact_p(*key)
        assert diffmod.exact_p(*swapped[i]) == exact == diffmod.exact_p(*flipped[i]), key              # exactly, in the oracle
        for p in (base[i], sw[i], fl[i]):
            diffmod_synth.check_p(float(p), exact, key[0] + key[2], key)
    ones = [(7, 0, 9, 0), (7, 7, 9, 9), (300, 0, 5, 0), (1 << 19, 1 << 19, 1 << 19, 1 << 19), (6, 0, 1 << 19, 0)]         # M = 0 or M = N
    assert all(diffmod.exact_p(*k) == 1.0 for k in ones) and twin_p(ones).tolist() == [1.0] * len(ones)


def brute_q(p, m):
    order = sorted(range(len(p)), key=lambda i: p[i])                 # stable
    q = [0.0] * len(p)
    for j, i in enumerate(order):
        q[i] = min(1.0, min(p[order[k]] * m / (k + 1) for k in range(j, len(p))))
    return q


def test_bh_qvalues_equal_the_definition():
    rng = np.random.default_rng(4)
    p = np.round(rng.random(200) ** 3, 2)                              # many ties, zeros among them
    p[:5] = 1.0
    for m in (200, 1000):
        got = diffmod.bh_qvalues(p, m)
        assert np.allclose(got, brute_q(p.tolist(), m), rtol=1e-15, atol=0) and (got >= np.minimum(p, 1.0) - 1e-18).all()
    assert diffmod.bh_qvalues([], 10).shape == (0,)
    with pytest.raises(diffmod.DiffmodError, match='among'):
        diffmod.bh_qvalues([0.1, 0.2], 1)


def test_bh_qvalues_of_the_subset_below_alpha_are_those_of_the_full_run():
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.random(300), rng.random(60) * 1e-3, np.full(7, 0.01)])
    rng.shuffle(p)
    for alpha in (0.05, 0.2, 1.0):
        full = diffmod.bh_qvalues(p, len(p))
        sub = p <= alpha
        part = diffmod.bh_qvalues(p[sub], len(p))
        hit = full <= alpha
        assert hit.sum() > 20 and (sub | ~hit).all()
        assert np.array_equal(part[hit[sub]], full[hit])
        assert (part[~hit[sub]] > alpha).all()                         # and nothing else of the subset gets below alpha


@pytest.fixture(scope='module')
def synthetic(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('diffmod'))
    case = diffmod_synth.write_case(root)
    got = {'default': diffmod_synth.run_command(case, root, diffmod.HostEngine(COV, FDR), 'default'),
           'all': diffmod_synth.run_command(case, root, diffmod.HostEngine(COV, 1.0), 'all', all=1),
           'delta11': diffmod_synth.run_command(case, root, diffmod.HostEngine(COV, FDR), 'delta11', minDelta=11)}
    return root, case, got


def test_command_under_host_engine_equals_the_golden(synthetic):
    root, case, got = synthetic
    want = GOLDEN['command']
    want['json']['inputs']['FileID'] = 'default'
    assert got['default']['txt'] == want['txt'] and got['default']['json'] == want['json']
    doc = got['default']['json']
    rows = diffmod_synth.parse_report(got['default']['txt'])
    assert got['default']['txt'].splitlines()[0] == diffmod.HEADER and len(rows) == doc['listed'] == doc['hyper'] + doc['hypo'] and doc['hyper'] > 0 and doc['hypo'] > 0
    assert [r[:3] for r in rows] == sorted(r[:3] for r in rows)       # contig, position, strand
    listed = {r[:3] for r in rows}
    planted = 0
    for (name, p, strand), (runs, is_planted) in case['sites'].items():
        cA, mA, cB, mB = diffmod_synth.pooled(runs)
        if is_planted and cA >= COV and cB >= COV:
            planted += 1
            assert (name, p, strand) in listed, (name, p, strand, cA, mA, cB, mB)
    assert planted >= 30
    for r in rows:                                                     # the integer columns are those of the pooled files
        runs, _ = case['sites'][r[:3]]
        cA, mA, cB, mB = diffmod_synth.pooled(runs)
        assert r[3:9] == (cA, mA, 100 * mA // cA, cB, mB, 100 * mB // cB) and r[9] == '%.2f' % (100.0 * mA / cA - 100.0 * mB / cB)
        assert r[11] <= FDR and r[10] <= r[11] * (1 + 1e-6) and 100 * abs(mA * cB - mB * cA) >= 10 * cA * cB
    assert doc['m'] == sum(doc['contigs'][c][s]['tested'] for c in doc['contigs'] for s in '+-') == sum(doc['p_histogram'])
    assert all(sum(doc['contigs'][c][s][k] for s in '+-') > 0 for c in doc['contigs'] for k in ('tested', 'shallow_sample', 'shallow_control'))
    assert any('mod_pos.chrB-.C.bed: line 1 is outside the device grammar: the file is parsed on the host' in n for n in doc['notes'])
    assert sorted(doc['contigs']) == ['chrA', 'chrB'] and doc['inputs']['chr'] == ['chrA', 'chrB']           # found from the file names: no --Ref, no --chr


def test_command_all_lists_every_tested_key_and_min_delta_is_an_integer_rule(synthetic):
    root, case, got = synthetic
    every = diffmod_synth.parse_report(got['all']['txt'])
    m = got['all']['json']['m']
    assert len(every) == m == got['default']['json']['m'] and got['all']['json']['listed'] == m
    q_of = {r[:3]: r[11] for r in every}
    for r in diffmod_synth.parse_report(got['default']['txt']):
        assert q_of[r[:3]] == r[11]                                   # the subset below alpha gives the q of the full run
    assert min(abs(r[11] - FDR) / FDR for r in every) >= 1e-3        # the case keeps every q away from --fdr
    # q of the whole list against the definition, from the exact p of every tested key
    exact = [diffmod.exact_p(*r[3:5], *r[6:8]) for r in every]
    for r, q in zip(every, diffmod.bh_qvalues(exact, m).tolist()):
        assert abs(r[11] - q) <= 1e-6 * q
    # the site exactly on --minDelta 10: 30 % against 20 %
    name, p, strand = diffmod_synth.DELTA_SITE[:3]
    at10 = {r[:3] for r in diffmod_synth.parse_report(got['default']['txt'])}
    at11 = {r[:3] for r in diffmod_synth.parse_report(got['delta11']['txt'])}
    assert (name, p, strand) in at10 and (name, p, strand) not in at11 and at11 < at10
    assert [r for r in every if r[:3] == (name, p, strand)][0][9] == '10.00'


def test_engine_and_option_refusals(synthetic):
    root, case, _ = synthetic
    for kw, words in (({'cov': 0}, '--cov'), ({'alpha': 0.0}, '--fdr'), ({'alpha': 1.5}, '--fdr'), ({'alpha': float('nan')}, '--fdr')):
        with pytest.raises(diffmod.DiffmodError, match=words):
            diffmod.HostEngine(**kw)
    z = (np.zeros(4, np.int64), np.zeros(4, np.int64))
    with pytest.raises(diffmod.DiffmodError, match='controls are missing'):
        diffmod.HostEngine().run(z, z, None, None)
    mo = {'predFolder': case['predFolder'], 'control': case['control'], 'Base': 'C', 'outFolder': os.path.join(root, 'never'), 'FileID': 'x'}
    with pytest.raises(diffmod.DiffmodError, match='the engine was made for cov 5 alpha 0.05'):
        diffmod.diffmod(dict(mo, fdr=0.1), engine=diffmod.HostEngine(5, 0.05))
    with pytest.raises(diffmod.DiffmodError, match='--minDelta'):
        diffmod.diffmod(dict(mo, minDelta=101), engine=diffmod.HostEngine(5, 0.05))
    bad = os.path.join(root, 'bad', 'run1')
    os.makedirs(bad)
    with open(os.path.join(bad, 'mod_pos.chrA+.C.bed'), 'w') as fh:
        fh.write('chrA 5 6 C 9 + 5 6 0,0,0 9 11 1\nchrA 7 8 C 9 + 7 8 0,0,0 9 200 x\n')
    with pytest.raises(diffmod.DiffmodError, match=r'mod_pos\.chrA\+\.C\.bed:2: '):                     # file:line: reason, from the host parse
        diffmod.diffmod(dict(mo, control=[os.path.join(root, 'bad')]), engine=diffmod.HostEngine(5, 0.05))
    assert not os.path.exists(os.path.join(root, 'never'))


def _diffmod(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'diffmod'] + args, capture_output=True, text=True, timeout=300)


def test_command_line_refusals(synthetic, tmp_path):
    """One line each, naming the option, before a BED file is read or a GPU asked for."""
    root, case, _ = synthetic
    out = tmp_path / 'out'
    empty = tmp_path / 'empty'
    (empty / 'run1').mkdir(parents=True)
    common = ['--predFolder', case['predFolder'], '--outFolder', str(out)]
    ctrl = ['--control', ','.join(case['control'])]
    for args, words in ((common, ('--control', 'are needed')),
                        (common + ['--control', str(empty)], ('--control', 'no *.<chr>+.C.bed')),
                        (common + ['--control', str(tmp_path / 'nowhere')], ('--control', 'no folder')),
                        (common + ctrl + ['--fdr', '0'], ('--fdr', 'above 0 and at most 1')),
                        (common + ctrl + ['--fdr', '1.5'], ('--fdr', 'above 0 and at most 1')),
                        (common + ctrl + ['--cov', '0'], ('--cov', '1 or more')),
                        (common + ctrl + ['--minDelta', '-1'], ('--minDelta', '0 to 100')),
                        (common + ctrl + ['--all', '2'], ('--all', '0 or 1')),
                        (common + ctrl + ['--Ref', str(tmp_path / 'no.fa')], ('--Ref', 'does not exist')),
                        (['--predFolder', str(tmp_path / 'nowhere'), '--outFolder', str(out)] + ctrl, ('--predFolder', 'does not exist'))):
        res = _diffmod(args)
        last = res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ''
        assert res.returncode != 0 and last.startswith('Error: diffmod: ') and all(w in last for w in words), (args, res.stderr[-2000:])
    assert not out.exists()
    helptext = _diffmod(['--help']).stdout
    assert 'mod_pos' in helptext and 'ignores' in helptext and 'replicates' in helptext


def test_host_twin_under_address_sanitizer(tmp_path):
    """tests/diffmod_driver.cpp: csrc/diffmod.inc built as a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in statically -
    every table and record array in a heap block of exactly its size; the edge lengths of the GPU sweep, empty tables, a key at MAX_TOTAL."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'diffmod_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'diffmod_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'DIFFMOD-DRIVER-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
