"""CPU: `diffmod --replicates 1` without a GPU.  diffmod.RepHostEngine (integers and 50-digit decimals) against tests/golden/diffrep_case.json
(tests/golden/make_golden_diffrep.py: scipy.stats.f.sf and mpmath recorded as second witnesses), the compiled host twin dm_diffrep_test_host against
the oracle within the derived interval of DESIGN.md 22 (diffrep_synth.bounds: D within 18 * 2^-53 * C, phi and the incomplete beta within 2.5e-11),
every fate on both strands, --minReps below the default, the command under RepHostEngine on the synthetic case of tests/diffrep_synth.py, the point
of the feature (where one replicate disagrees, the replicate test's p exceeds the pooled Fisher p), the refusals of the command line, --replicates 0
and --replicates 1 against the bytes of the parent's commands, and the host twin under the address sanitizer (tests/diffrep_driver.cpp)."""
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
import diffrep_synth as synth  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'diffrep_case.json')))
COV, FDR = synth.COV, synth.FDR
INT_FIELDS = ('pos', 'strand', 'cA', 'mA', 'cB', 'mB', 'nA', 'nB')


def test_oracle_equals_the_golden_keys_and_their_witnesses():
    rows = GOLDEN['keys']
    assert len(rows) >= 280 and GOLDEN['cov'] == COV and {tuple(r['shape']) for r in rows} == set(synth.SHAPES)
    equal = over = 0
    for r in rows:
        KA, (a, b) = r['shape'][0], r['minReps']
        f, ua, ub = synth.used_of((tuple(r['c']), tuple(r['m'])), KA, COV, a, b)
        assert f == 0, r
        e = diffmod.rep_exact(tuple(ua), tuple(ub))
        assert (e['nu'], e['equal']) == (r['nu'], r['equal']) and float(e['p']) == r['p'] and float(e['phi']) == r['phi'], r          # the oracle has not moved
        assert diffmod.rep_exact_p(ua, ub) == r['p']
        if r['equal']:
            assert r['p'] == 1.0 and r['phi'] == 1.0
            equal += 1
            continue
        for witness in ('scipy', 'mpmath'):
            assert abs(r[witness] - r['p']) <= 1e-12 * r['p'], (witness, r)
        assert abs(r['D_mpmath'] - r['D']) <= 1e-12 * r['D'], r
        over += r['phi'] > 1.0
    assert equal >= 20 and over >= 50 and min(r['p'] for r in rows) < 1e-9 and {r['nu'] for r in rows} >= {1, 2, 6, 14}


@pytest.mark.parametrize('shape', synth.SHAPES)
def test_host_twin_within_the_interval_on_the_generator_keys(hip_lib, shape):
    KA, KB = shape
    assert diffmod.max_replicates() == diffmod.MAX_REPS == 8
    shallow_at_default = tested_below = 0
    for a, b in sorted({(KA, KB), synth.low_min_reps(KA, KB)}):
        keys = synth.sweep_keys(KA, KB, a, b)
        sample, control = synth.keys_on_a_line(keys, KA)
        counters, hist, got = diffmod.rep_host_routine(COV, 1.0, a, b, sample, control)
        host = diffmod.RepHostEngine(COV, 1.0, a, b)
        want_counters, want = host.run(sample, control)
        fates = [synth.used_of(k, KA, COV, a, b)[0] for k in keys]
        assert counters.tolist() == want_counters.tolist() == [[fates.count(j) for j in range(4)], [0] * 4]
        assert all(counters[0] > 0) and fates.count(-1) >= 1                                   # every fate, and an ignored key
        for k in INT_FIELDS:
            assert got[k].tolist() == want[k].tolist(), k
        assert got['pos'].tolist() == [i for i, f in enumerate(fates) if f == 0]
        synth.check_records(got, sample + control, KA, COV, a, b, (shape, a, b))
        synth.check_records(want, sample + control, KA, COV, a, b, (shape, a, b))             # (the oracle lies in its own interval)
        ones = want['p'] == 1.0
        assert ones.sum() >= 2 and (got['p'][ones] == 1.0).all() and (got['phi'][ones] == 1.0).all()          # the integer rule: exactly 1
        assert got['phi'].min() == 1.0 and got['phi'].max() > 50.0                             # X2 / nu below 1 and far above it
        assert (got['cA'].astype(np.int64) + got['cB']).max() == synth.MAX_TOTAL               # a key exactly at MAX_TOTAL was tested
        assert hist.sum() == counters[0, 0] and hist.tolist() == np.bincount(np.minimum(19, (20 * got['p']).astype(np.int64)), minlength=20).tolist()
        if (a, b) == (KA, KB):
            shallow_at_default = int(counters[0, 1] + counters[0, 2])
            assert (got['nA'] == KA).all() and (got['nB'] == KB).all()
        else:
            tested_below = int(((got['nA'] < KA) | (got['nB'] < KB)).sum())                   # a dropped replicate: nu changes
            assert tested_below >= 2
        # alpha 0.05: the records of alpha 1 with p <= alpha, bit for bit
        _, hist2, part = diffmod.rep_host_routine(COV, FDR, a, b, sample, control)
        keep = got['p'] <= FDR
        assert 0 < keep.sum() < len(keep) and hist2.tolist() == hist.tolist()
        for k in INT_FIELDS + ('phi', 'p'):
            assert part[k].tobytes() == got[k][keep].tobytes(), k
    assert shallow_at_default >= 4


@pytest.mark.parametrize('shape', ((2, 1), (3, 5)))
def test_every_fate_on_both_strands_at_the_tile_edges(hip_lib, shape):
    KA, KB = shape
    a, b = synth.low_min_reps(KA, KB)
    tile = diffmod.tile_positions()
    keys = synth.sweep_keys(KA, KB, a, b)
    for n, phase in ((tile + 1, 0), (3 * tile + 5, 1)):
        tables = [synth.host_tables(rec, n) for rec in synth.layout(keys, KA + KB, n, tile, phase)]
        counters, hist, got = diffmod.rep_host_routine(COV, 1.0, a, b, tables[:KA], tables[KA:])
        want_counters, want = diffmod.RepHostEngine(COV, 1.0, a, b).run(tables[:KA], tables[KA:])
        assert counters.tolist() == want_counters.tolist() and (counters > 0).all()
        for k in INT_FIELDS:
            assert got[k].tolist() == want[k].tolist(), k
        assert (np.diff(2 * got['pos'].astype(np.int64) + got['strand']) > 0).all()           # key order
        assert {0, tile - 1, tile, n - 1} <= set(got['pos'].tolist())
        synth.check_records(got, tables, KA, COV, a, b, (shape, n))


def test_engine_refusals():
    for kw, words in (({'cov': 0}, '--cov'), ({'alpha': 0.0}, '--fdr'), ({'min_a': 0, 'min_b': 3}, '--minReps'), ({'min_a': 1, 'min_b': 1}, '--minReps'),
                      ({'min_a': 9, 'min_b': 1}, '--minReps')):
        with pytest.raises(diffmod.DiffmodError, match=words):
            diffmod.RepHostEngine(**kw)
    z = ((np.zeros(3, np.int64), np.zeros(3, np.int64)),) * 2
    eng = diffmod.RepHostEngine(5, 0.05, 2, 2)
    for sample, control, words in (([z], [z], '3 or more'), ([z] * 9, [z], '1 to 8'), ([z], [z, z], '--minReps')):
        with pytest.raises(diffmod.DiffmodError, match=words):
            eng.run(sample, control)


@pytest.fixture(scope='module')
def synthetic(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('diffrep'))
    case = synth.write_case(root)
    got = {'default': synth.run_command(case, root, diffmod.RepHostEngine(COV, FDR, 3, 2), 'default'),
           'all': synth.run_command(case, root, diffmod.RepHostEngine(COV, 1.0, 3, 2), 'all', all=1),
           'delta11': synth.run_command(case, root, diffmod.RepHostEngine(COV, FDR, 3, 2), 'delta11', minDelta=11),
           'low': synth.run_command(case, root, diffmod.RepHostEngine(COV, 1.0, 2, 2), 'low', all=1, minReps='2,2')}
    return root, case, got


def test_command_under_rep_host_engine(synthetic):
    root, case, got = synthetic
    doc, txt = got['default']['json'], got['default']['txt']
    rows = synth.parse_report(txt)
    assert txt.splitlines()[0] == diffmod.REP_HEADER == 'chr\tpos\tstrand\tcovA\tmodA\tpctA\tcovB\tmodB\tpctB\tdelta\trepA\trepB\tphi\tp\tq'
    assert doc['test'] == 'quasibinomial-F' and doc['minReps'] == [3, 2]
    assert doc['replicates'] == {'sample': ['<root>/s1', '<root>/s2', '<root>/s3'], 'control': ['<root>/c1', '<root>/c2']}
    assert len(rows) == doc['listed'] == doc['hyper'] + doc['hypo'] and doc['hyper'] > 0 and doc['hypo'] > 0
    assert [r[:3] for r in rows] == sorted(r[:3] for r in rows)       # contig, position, strand
    assert sorted(doc['contigs']) == ['chrA', 'chrB'] and doc['inputs']['chr'] == ['chrA', 'chrB']
    a = doc['contigs']['chrA']
    assert a['files'] == [2, 4, 2] and a['control_files'] == [2, 2] and len(a['lines_read']) == 3 and len(a['control_lines_read']) == 2      # s2: two runs
    lines = {f: 0 for f in synth.FOLDERS}
    for (name, p, strand), (sample, control, _) in case['sites'].items():
        for f, (c, _) in zip(synth.FOLDERS, sample + control):
            lines[f] += (name == 'chrA') and c > 0
    assert a['lines_read'] == [lines[f] for f in synth.FOLDERS[:3]] and a['control_lines_read'] == [lines[f] for f in synth.FOLDERS[3:]]
    listed = {r[:3]: r for r in rows}
    planted = 0
    for key, site in case['sites'].items():
        if site[2] == 'planted':
            planted += 1
            assert key in listed, (key, site)
    assert planted == 40
    for r in rows:                                                     # the integer columns are the sums over the replicates, all of them used
        cA, mA, cB, mB = synth.pooled(case['sites'][r[:3]])
        assert r[3:9] == (cA, mA, 100 * mA // cA, cB, mB, 100 * mB // cB) and r[9] == '%.2f' % (100.0 * mA / cA - 100.0 * mB / cB) and r[10:12] == (3, 2)
        assert r[14] <= FDR and r[13] <= r[14] * (1 + 1e-6) and 100 * abs(mA * cB - mB * cA) >= 10 * cA * cB and r[12] >= 1.0
    assert doc['m'] == sum(doc['contigs'][c][s]['tested'] for c in doc['contigs'] for s in '+-') == sum(doc['p_histogram'])
    assert all(sum(doc['contigs'][c][s][k] for s in '+-') > 0 for c in doc['contigs'] for k in ('tested', 'shallow_sample', 'shallow_control'))
    assert any('mod_pos.chrB-.C.bed: line 1 is outside the device grammar: the file is parsed on the host' in n for n in doc['notes'])


def test_bh_over_the_contigs_all_and_min_delta(synthetic):
    root, case, got = synthetic
    every = synth.parse_report(got['all']['txt'])
    m = got['all']['json']['m']
    assert len(every) == m == got['default']['json']['m'] and got['all']['json']['listed'] == m and len({r[0] for r in every}) == 2
    q_of = {r[:3]: r[14] for r in every}
    for r in synth.parse_report(got['default']['txt']):
        assert q_of[r[:3]] == r[14]                                   # the subset below alpha gives the q of the full run
    assert min(abs(r[14] - FDR) / FDR for r in every) >= 1e-3         # the case keeps every q away from --fdr
    exact = []
    for r in every:                                                   # q of the whole list against the definition, from the oracle's p of every key
        sample, control, _ = case['sites'][r[:3]]
        exact.append(diffmod.rep_exact_p([s for s in sample if s[0] >= COV], [c for c in control if c[0] >= COV]))
    for r, p, q in zip(every, exact, diffmod.bh_qvalues(exact, m).tolist()):
        assert abs(r[13] - p) <= 1e-6 * p and abs(r[14] - q) <= 1e-6 * q and r[12] == float('%.4f' % r[12])
    # the site exactly on --minDelta 10: 30 % against 20 %
    name, p, strand = synth.DELTA_SITE[:3]
    at10 = {r[:3] for r in synth.parse_report(got['default']['txt'])}
    at11 = {r[:3] for r in synth.parse_report(got['delta11']['txt'])}
    assert (name, p, strand) in at10 and (name, p, strand) not in at11 and at11 < at10
    assert [r for r in every if r[:3] == (name, p, strand)][0][9] == '10.00'


def test_where_a_replicate_disagrees_the_p_exceeds_the_pooled_fisher_p(synthetic):
    """The point of the feature."""
    root, case, got = synthetic
    every = {r[:3]: r for r in synth.parse_report(got['all']['txt'])}
    listed = {r[:3] for r in synth.parse_report(got['default']['txt'])}
    seen = fisher_calls = held_back = 0
    for key, site in case['sites'].items():
        if site[2] != 'disagree':
            continue
        seen += 1
        fisher = diffmod.exact_p(*synth.pooled(site))
        r = every[key]
        assert r[13] > fisher and r[12] > 1.0, (key, site, r, fisher)
        fisher_calls += fisher <= 0.01
        held_back += fisher <= 0.01 and r[13] > 0.05 and key not in listed
    assert seen == 30 and fisher_calls >= 20 and held_back >= 20


def test_min_reps_below_the_default(synthetic):
    root, case, got = synthetic
    low, full = got['low']['json'], got['all']['json']
    assert low['minReps'] == [2, 2] and low['inputs']['minReps'] == [2, 2] and low['m'] > full['m']
    rows = synth.parse_report(got['low']['txt'])
    two = [r for r in rows if r[10] == 2]
    assert len(two) == low['m'] - full['m'] > 5 and all(r[11] == 2 for r in rows)
    for r in two:                                                      # the sums are over the used replicates alone
        sample, control, _ = case['sites'][r[:3]]
        used = [s for s in sample if s[0] >= COV]
        assert len(used) == 2 and r[3:5] == (sum(c for c, _ in used), sum(m for _, m in used))
        assert abs(r[13] - diffmod.rep_exact_p(used, control)) <= 1e-6 * r[13]
    for c in low['contigs']:
        for s in '+-':
            assert low['contigs'][c][s]['shallow_sample'] <= full['contigs'][c][s]['shallow_sample']


def test_option_refusals_before_a_file_is_read(synthetic):
    root, case, _ = synthetic
    mo = {'predFolder': case['predFolder'], 'control': case['control'], 'Base': 'C', 'outFolder': os.path.join(root, 'never'), 'FileID': 'x', 'replicates': 1}
    eng = diffmod.RepHostEngine(5, 0.05, 3, 2)
    for change, words in (({'fdr': 0.1}, 'the engine was made for cov 5 alpha 0.05 minReps 3,2'), ({'minReps': '2,2'}, 'the engine was made for'),
                          ({'minReps': '4,2'}, '--minReps'), ({'minReps': '3'}, '--minReps'), ({'minReps': 'x,2'}, '--minReps'), ({'replicates': 2}, '--replicates'),
                          ({'predFolder': case['predFolder'][:1], 'control': case['control'][:1]}, '3 or more replicates'),
                          ({'predFolder': case['predFolder'] + [case['predFolder'][0]]}, 'named twice'),
                          ({'control': case['control'] + [case['predFolder'][1] + os.sep]}, 'named twice'),
                          ({'predFolder': [case['predFolder'][0]] * 9}, '1 to 8 folders'),
                          ({'control': [os.path.join(root, 'nowhere'), case['control'][0]]}, 'no folder'),
                          ({'replicates': 0, 'minReps': '1,2'}, 'only with --replicates 1')):
        with pytest.raises(diffmod.DiffmodError, match=words):
            diffmod.diffmod(dict(mo, **change), engine=eng)
    assert not os.path.exists(os.path.join(root, 'never'))


def _diffmod(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'diffmod'] + args, capture_output=True, text=True, timeout=300)


def test_command_line_refusals(synthetic, tmp_path):
    """One line each, naming the option, before a BED file is read or a GPU asked for."""
    root, case, _ = synthetic
    out = tmp_path / 'out'
    empty = tmp_path / 'empty'
    (empty / 'run1').mkdir(parents=True)
    pred, ctrl = ','.join(case['predFolder']), ','.join(case['control'])
    rep = ['--replicates', '1', '--outFolder', str(out)]
    for args, words in ((rep + ['--predFolder', pred], ('--control', 'are needed')),
                        (rep + ['--predFolder', case['predFolder'][0], '--control', case['control'][0]], ('--replicates 1', '3 or more replicates')),
                        (rep + ['--predFolder', pred, '--control', ctrl, '--minReps', '4,2'], ('--minReps', '1 <= a <= 3')),
                        (rep + ['--predFolder', pred, '--control', ctrl, '--minReps', '1,1'], ('--minReps', 'a + b >= 3')),
                        (rep + ['--predFolder', pred, '--control', ctrl, '--minReps', 'two'], ('--minReps', 'two integers')),
                        (rep + ['--predFolder', pred + ',' + case['predFolder'][2], '--control', ctrl], ('--predFolder', 'named twice')),
                        (rep + ['--predFolder', pred, '--control', ctrl + ',' + case['predFolder'][0]], ('--control', 'named twice')),
                        (rep + ['--predFolder', pred, '--control', ctrl + ',' + str(empty)], ('--control', 'no *.<chr>+.C.bed')),
                        (rep + ['--predFolder', pred + ',' + str(tmp_path / 'nowhere'), '--control', ctrl], ('--predFolder', 'no folder')),
                        (rep + ['--predFolder', pred, '--control', ctrl, '--fdr', '0'], ('--fdr', 'above 0 and at most 1')),
                        (['--replicates', '2', '--outFolder', str(out), '--predFolder', pred, '--control', ctrl], ('--replicates', '0 or 1')),
                        (['--outFolder', str(out), '--predFolder', case['predFolder'][0], '--control', ctrl, '--minReps', '1,2'], ('--minReps', 'only with --replicates 1'))):
        res = _diffmod(args)
        last = res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ''
        assert res.returncode != 0 and last.startswith('Error: diffmod: ') and all(w in last for w in words), (args, res.stderr[-2000:])
    assert not out.exists()
    helptext = _diffmod(['--help']).stdout
    assert '--replicates' in helptext and '--minReps' in helptext and 'quasi-binomial' in helptext


def test_replicates_0_writes_the_bytes_of_the_parent(tmp_path):
    """tests/golden/diffmod_case.json holds the report and the document the command wrote before --replicates existed."""
    parent = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'diffmod_case.json')))['command']
    root = str(tmp_path)
    case = diffmod_synth.write_case(root)
    for fileid, options in (('unset', {}), ('zero', {'replicates': 0}), ('none', {'replicates': None, 'minReps': None})):
        got = diffmod_synth.run_command(case, root, diffmod.HostEngine(diffmod_synth.COV, diffmod_synth.FDR), fileid, **options)
        parent['json']['inputs']['FileID'] = fileid
        assert got['txt'] == parent['txt'] and got['json'] == parent['json'], fileid
        with open(os.path.join(root, 'out', fileid + '_diffmod.json')) as fh:
            assert list(json.load(fh)) == ['inputs', 'contigs', 'm', 'listed', 'hyper', 'hypo', 'p_histogram', 'notes', 'times']


def test_replicates_1_writes_the_bytes_of_the_parent(synthetic):
    """tests/golden/diffrep_case.json['command'] holds the reports and the documents the command wrote when --replicates 1 had a driver of its own,
    for three option sets of the synthetic case (make_golden_diffrep.command_case)."""
    root, case, got = synthetic
    parents = GOLDEN['command']
    assert sorted(parents) == ['all', 'default', 'low']
    for fileid, parent in parents.items():
        parent['json']['inputs']['FileID'] = fileid
        assert got[fileid]['txt'] == parent['txt'] and got[fileid]['json'] == parent['json'], fileid
        assert json.dumps(got[fileid]['json']) == json.dumps(parent['json']), fileid          # and every key in the parent's order
        with open(os.path.join(root, 'out', fileid + '_diffmod.json')) as fh:
            assert list(json.load(fh)) == ['test', 'inputs', 'replicates', 'minReps', 'contigs', 'm', 'listed', 'hyper', 'hypo', 'p_histogram', 'notes', 'times']


def test_host_twin_under_address_sanitizer(tmp_path):
    """tests/diffrep_driver.cpp: csrc/diffrep.inc built as a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in statically -
    every table, pointer list and record array in a heap block of exactly its size; the edge lengths of the GPU sweep, empty tables, a key at
    MAX_TOTAL, coverages whose sum needs 64 bits."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'diffrep_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'diffrep_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'DIFFREP-DRIVER-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
