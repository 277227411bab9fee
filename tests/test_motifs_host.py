"""CPU: the search of `motifs` (pattern_counts against brute force, find_motifs on constructed histograms: the order, every tie-break, the trimming),
motifs.HostEngine and the compiled host twin dm_motifs_count_host against tests/golden/motifs_case.json (plain dicts and loops:
tests/golden/make_golden_motifs.py), the count of an emitted motif against siteperf.site_codes, the command under HostEngine on the synthetic case
of tests/motifs_synth.py against tests/golden/motifs_command.json, the refusals of the command line, and the host twin under the address sanitizer
(tests/motifs_asan_driver.cpp)."""
import itertools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import merge, motifs, siteperf

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import motifs_synth  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
LET = 'ACGTN'


def ctx_index(word):
    v = 0
    for ch in word:
        v = v * 4 + 'ACGT'.index(ch)
    return v


def hist_of(L, background, entries):
    """[4^L][2]: `background` (n, m) in every context, then {pattern of A, C, G, T, N over the L flank offsets: (n, m)} set in each context it matches."""
    h = np.zeros((4 ** L, 2), np.int64)
    h[:] = background
    for pat, value in entries.items():
        for word in itertools.product(*[('ACGT' if c == 'N' else c) for c in pat]):
            h[ctx_index(word)] = value
    return h


def found(h, up, down, **kw):
    return [(m['motif'], m['ModinMotif'], m['sites'], m['modified']) for m in motifs.find_motifs(h, up, down, **kw)]


@pytest.mark.parametrize('up,down', [(1, 1), (2, 1), (0, 3), (0, 0)])
def test_pattern_counts_equal_brute_force(up, down):
    L = up + down
    rng = np.random.default_rng(100 * up + down)
    hist = rng.integers(0, 1000, (4 ** L, 2))
    got = motifs.pattern_counts(hist, up, down)
    assert got.shape == (5 ** L, 2) and got.dtype == np.int64
    for index, pat in enumerate(itertools.product(LET, repeat=L)):                  # the pattern index: digits A < C < G < T < N, the first the most significant
        want = np.zeros(2, np.int64)
        for c, word in enumerate(itertools.product('ACGT', repeat=L)):
            if all(p == 'N' or p == w for p, w in zip(pat, word)):
                want += hist[c]
        assert got[index].tolist() == want.tolist(), (pat, index)
        assert motifs.pattern_digits(index, L) == [LET.index(p) for p in pat]
    if L == 0:
        assert got.tolist() == [hist[0].tolist()]                                   # the single, empty pattern


def test_find_motifs_planted_gatc():
    h = hist_of(6, (10, 0), {'NNGTCN': (10, 10)})
    got = motifs.find_motifs(h, 3, 3, 20, 50, 8, 'A')
    assert [(m['motif'], m['ModinMotif'], m['label'], m['sites'], m['modified'], m['pass']) for m in got] == [('GATC', 1, 'gAtc', 640, 640, 1)]
    # a sub-pattern of the emitted motif (GATCG, 160 modified sites of its own) is gone with the motif's contexts: nothing is emitted twice
    assert (h[:, 1] > 0).sum() == 64                                               # (find_motifs works on a copy)


def test_find_motifs_two_motifs_in_the_stated_order():
    h = hist_of(5, (10, 0), {'NGTCN': (10, 10), 'GATTC': (10, 10)})                # flank (2,3): GATC, and GAATTC with its modified base at index 2
    assert found(h, 2, 3, min_sites=5, min_frac=50, max_motifs=8) == [('GATC', 1, 160, 160), ('GAATTC', 2, 10, 10)]
    assert found(h, 2, 3, min_sites=5, min_frac=50, max_motifs=1) == [('GATC', 1, 160, 160)]             # max_motifs cuts the list
    assert found(h, 2, 3, min_sites=11, min_frac=50, max_motifs=8) == [('GATC', 1, 160, 160)]            # GAATTC below min_sites


def test_find_motifs_tie_breaks():
    kw = dict(min_sites=5, min_frac=50, max_motifs=2)
    # fewer fixed letters first, although GAT has more modified sites than CA
    h = hist_of(2, (10, 0), {'CN': (10, 10), 'GT': (100, 100), 'GA': (100, 0), 'GC': (100, 0), 'GG': (100, 0), 'AT': (100, 0), 'TT': (100, 0)})
    assert found(h, 1, 1, **kw) == [('CA', 1, 40, 40), ('GAT', 1, 100, 100)]
    # as many fixed letters: the larger modified count
    quiet = {a + b: (100, 0) for a in 'AG' for b in 'ACGT'}
    h = hist_of(2, (0, 0), dict(quiet, CN=(10, 10), TN=(20, 20)))
    assert found(h, 1, 1, **kw) == [('TA', 1, 80, 80), ('CA', 1, 40, 40)]
    # as many modified: the larger tested count
    h = hist_of(2, (0, 0), dict(quiet, CN=(10, 10), TN=(10, 10), TA=(20, 10)))
    assert found(h, 1, 1, **kw) == [('TA', 1, 50, 40), ('CA', 1, 40, 40)]
    # all equal: the smaller pattern index (C before T at the most significant offset)
    h = hist_of(2, (0, 0), dict(quiet, CN=(10, 10), TN=(10, 10)))
    assert found(h, 1, 1, **kw) == [('CA', 1, 40, 40), ('TA', 1, 40, 40)]
    h = hist_of(2, (0, 0), dict({b + a: (100, 0) for a in 'AG' for b in 'ACGT'}, NC=(10, 10), NT=(10, 10)))           # the same downstream
    assert found(h, 1, 1, **kw) == [('AC', 0, 40, 40), ('AT', 0, 40, 40)]


def test_find_motifs_all_n_nothing_and_trimming():
    h = hist_of(2, (10, 9), {})
    got = motifs.find_motifs(h, 1, 1, 20, 50, 8, 'C')
    assert [(m['motif'], m['ModinMotif'], m['label'], m['sites'], m['modified']) for m in got] == [('C', 0, 'C', 160, 144)]      # the base alone
    assert motifs.find_motifs(hist_of(2, (10, 4), {}), 1, 1, 20, 50, 8) == []                          # 40 % everywhere: nothing
    assert motifs.find_motifs(hist_of(2, (1, 1), {}), 1, 1, 20, 50, 8) == []                           # 16 modified sites: below min_sites
    assert motifs.find_motifs(np.zeros((1, 2), np.int64), 0, 0, 1, 50, 8) == []
    assert found(np.array([[30, 20]]), 0, 0, min_sites=20, min_frac=50, max_motifs=8, base='T') == [('T', 0, 30, 20)]
    # an interior N is kept, the outer ones are trimmed, and ModinMotif counts from the first letter kept
    h = hist_of(6, (10, 0), {'NNGNTC': (10, 10)})
    got = motifs.find_motifs(h, 3, 3, 20, 50, 8, 'A')
    assert [(m['motif'], m['ModinMotif'], m['label']) for m in got] == [('GANTC', 1, 'gAntc')]
    assert motifs.report_text(got).splitlines()[1].split('\t') == ['1', 'GANTC', '1', 'gAntc', '640', '640', '100', '-']
    h = hist_of(6, (10, 0), {'CNTNNN': (10, 10)})
    got = motifs.find_motifs(h, 3, 3, 20, 50, 8, 'A')
    assert [(m['motif'], m['ModinMotif'], m['label']) for m in got] == [('CNTA', 3, 'cntA')]
    assert motifs.context_string(ctx_index('GATTCG'), 3, 3, 'A') == 'gatAtcg'


def golden_tables(g, which, name):
    seq = g['reference'][name]
    out = []
    for strand in '+-':
        cov, mod = np.zeros(len(seq), np.int64), np.zeros(len(seq), np.int64)
        for p, (c, m) in g[which][name][strand].items():
            cov[int(p)], mod[int(p)] = c, m
        out.append((cov, mod))
    return out


def test_host_engine_and_host_twin_equal_the_golden_case(hip_lib):
    g = json.load(open(os.path.join(GOLDEN, 'motifs_case.json')))
    o = g['options']
    assert sorted(g['reference']) == ['chrA', 'chrB'] and len(g['cases']) == 4
    for case in g['cases']:
        up, down = case['flank']
        eng = motifs.HostEngine(up, down, o['Base'], o['cov'], o['min_pct'], o['max_ctrl_pct'])
        twin = np.zeros((4 ** (up + down), 2), np.int64)
        for name in sorted(g['reference']):
            seq = g['reference'][name].encode()
            tabs = golden_tables(g, 'sample', name) + (golden_tables(g, 'control', name) if case['controls'] else [])
            counters, off_base = eng.count(seq, *tabs)
            h2, c2, o2 = motifs.count_host_routine(up, down, o['Base'], o['cov'], o['min_pct'], o['max_ctrl_pct'], seq, *tabs)
            twin += h2
            for s, strand in enumerate('+-'):
                want = case['contigs'][name][strand]
                assert dict(zip(motifs.COUNT_KEYS, counters[s].tolist()), off_base=int(off_base[s])) == want, (case['flank'], case['controls'], name, strand)
                assert dict(zip(motifs.COUNT_KEYS, c2[s].tolist()), off_base=int(o2[s])) == want
        hist = eng.fetch()
        got = {motifs.context_string(int(i), up, down, o['Base']): hist[i].tolist() for i in np.nonzero(hist.any(axis=1))[0]}
        assert got == case['contexts'], (case['flank'], case['controls'])
        assert np.array_equal(twin, hist)
        want_total = {k: sum(case['contigs'][n][s][k] for n in case['contigs'] for s in '+-') for k in motifs.COUNT_KEYS}
        assert dict(zip(motifs.COUNT_KEYS, eng.counters.sum(axis=0).tolist())) == want_total                 # accumulated over the contigs
        # every skip rule is hit on both strands of chrA (no_control: where there are controls)
        assert all(case['contigs']['chrA'][s][k] > 0 for s in '+-' for k in motifs.COUNT_KEYS + ('off_base',) if k != 'no_control' or case['controls'])
        eng.reset()
        assert not eng.fetch().any() and not eng.counters.any() and not eng.off_base.any()


def test_host_engine_refusals():
    for kw, words in (({'up': 5, 'down': 4}, '--flank'), ({'up': 9, 'down': 0}, '--flank'), ({'up': -1}, '--flank'), ({'base': 'N'}, '--Base'), ({'base': 'a'}, '--Base'),
                      ({'cov': 0}, '--cov'), ({'min_pct': 101}, '--minPct'), ({'min_pct': -1}, '--minPct'), ({'max_ctrl_pct': 101}, '--maxCtrlPct')):
        with pytest.raises(motifs.MotifsError, match=words):
            motifs.HostEngine(**kw)
    eng = motifs.HostEngine(1, 1, 'A')
    z = (np.zeros(4, np.int64), np.zeros(4, np.int64))
    with pytest.raises(motifs.MotifsError, match='both of their tables'):
        eng.count(b'ACGT', z, z, z, None)
    with pytest.raises(motifs.MotifsError, match='a table of 4 positions'):
        eng.count(b'ACGTA', z, z)


@pytest.fixture(scope='module')
def synthetic(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('motifs'))
    case = motifs_synth.write_case(root)
    got = {key: motifs_synth.run_command(case, root, ctrl, motifs.HostEngine(3, 3, 'A'), key) for key, ctrl in (('with_control', True), ('without_control', False))}
    return root, case, got


def test_command_under_host_engine_equals_the_golden(synthetic):
    root, case, got = synthetic
    want = json.load(open(os.path.join(GOLDEN, 'motifs_command.json')))
    with_c, without = got['with_control']['json'], got['without_control']['json']
    assert [(m['motif'], m['ModinMotif']) for m in with_c['motifs']] == [('GATC', 1)]                 # TGCAG is as high in the control: absent
    assert [(m['motif'], m['ModinMotif']) for m in without['motifs']] == [('GATC', 1), ('TGCAG', 3)]
    assert '--motif gAtc --ModinMotif 1' in got['with_control']['txt'] and '--motif tgcAg --ModinMotif 3' in got['without_control']['txt']
    for key in ('with_control', 'without_control'):
        assert got[key]['txt'] == want[key]['txt'], key
        assert got[key]['json'] == want[key]['json'], key
        notes = got[key]['json']['notes']
        assert any('mod_pos.chr2-.A.bed: line 1 is outside the device grammar' in n for n in notes)    # the file with \r: parsed on the host
        assert any(n.startswith('chr1 +: ') and 'not A in --Ref' in n for n in notes)                  # off_base > 0
    assert all(v['no_control'] == 0 for c in without['contigs'].values() for v in (c['+'], c['-'])) and with_c['contigs']['chr1']['+']['no_control'] > 0


def bed_tables(folder, name, length):
    tabs = [(np.zeros(length, np.int64), np.zeros(length, np.int64)) for _ in range(2)]
    for path in merge.find_bed_files(folder, name, 'A'):
        _, pos, strand, cov, mod = merge.readbed2(path)
        for s, sign in enumerate('+-'):
            sel = strand == sign
            np.add.at(tabs[s][0], pos[sel], cov[sel])
            np.add.at(tabs[s][1], pos[sel], mod[sel])
    return tabs


def test_sites_of_a_motif_equal_the_site_codes_of_siteperf(synthetic):
    """For an emitted motif without an interior N, on contigs with no site within the flank of an end: `sites` is the number of keys
    siteperf.site_codes marks whose coverage is >= cov in the sample, and in the control where there is one."""
    root, case, got = synthetic
    for key, with_control in (('with_control', True), ('without_control', False)):
        for mt in got[key]['json']['motifs']:
            total = 0
            for name, seq in case['reference'].items():
                code = siteperf.site_codes(seq.encode(), mt['motif'], mt['ModinMotif'])
                assert not code[:3].any() and not code[-3:].any()
                sample, control = bed_tables(case['predFolder'], name, len(seq)), bed_tables(case['control'], name, len(seq))
                for s in range(2):
                    keep = (((code >> s) & 1) != 0) & (sample[s][0] >= 5)
                    if with_control:
                        keep &= control[s][0] >= 5
                    total += int(keep.sum())
            assert mt['sites'] == total, (key, mt)


def test_command_notes_when_nothing_qualifies(synthetic, capsys):
    root, case, _ = synthetic
    mo = {'predFolder': case['predFolder'], 'control': [], 'Ref': case['Ref'], 'Base': 'A', 'outFolder': os.path.join(root, 'none'), 'FileID': 'none', 'minSites': 100000}
    doc = motifs.motifs(mo, engine=motifs.HostEngine(3, 3, 'A'))
    assert doc['motifs'] == [] and 'no pattern reached --minSites 100000 / --minFrac 50' in doc['notes']
    assert open(os.path.join(root, 'none', 'none_motifs.txt')).read().count('\n') == 1                # the header alone
    with pytest.raises(motifs.MotifsError, match='the engine was made for flank 2,3'):
        motifs.motifs(mo, engine=motifs.HostEngine(2, 3, 'A'))


def _motifs(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'motifs'] + args, capture_output=True, text=True, timeout=300)


def test_command_line_refusals(synthetic, tmp_path):
    """One line each, naming the option, before a BED file is read or a GPU asked for."""
    root, case, _ = synthetic
    out = tmp_path / 'out'
    other = tmp_path / 'other.fa'
    other.write_text('>chr1\n' + case['reference']['chr1'] + '\n')                  # chr2 is in the files and not in this reference
    common = ['--predFolder', case['predFolder'], '--Ref', case['Ref'], '--outFolder', str(out)]
    for args, words in ((['--predFolder', case['predFolder'], '--outFolder', str(out)], ('--Ref', 'is needed')),
                        (['--predFolder', case['predFolder'], '--Ref', str(tmp_path / 'no.fa'), '--outFolder', str(out)], ('--Ref', 'does not exist')),
                        (['--predFolder', case['predFolder'], '--Ref', str(other), '--outFolder', str(out)], ('--Ref', 'mod_pos.chr2', 'does not hold')),
                        (common + ['--chr', 'chr1,chr9'], ('--chr', 'holds no contig chr9')),
                        (common + ['--flank', '5,4'], ('--flank', '8 in all')),
                        (common + ['--flank', '3'], ('--flank', 'two numbers')),
                        (common + ['--minPct', '101'], ('--minPct', '0 to 100')),
                        (common + ['--maxCtrlPct', '-1'], ('--maxCtrlPct', '0 to 100')),
                        (common + ['--cov', '0'], ('--cov', '1 or more')),
                        (common + ['--minFrac', '101'], ('--minFrac', '0 to 100')),
                        (common + ['--control', str(tmp_path / 'nowhere')], ('--control', 'no folder')),
                        (['--predFolder', str(tmp_path / 'nowhere'), '--Ref', case['Ref'], '--outFolder', str(out)], ('--predFolder', 'does not exist'))):
        res = _motifs(args)
        last = res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ''
        assert res.returncode != 0 and last.startswith('Error: motifs: ') and all(w in last for w in words), (args, res.stderr[-2000:])
    assert not out.exists()


def test_host_twin_under_address_sanitizer(tmp_path):
    """tests/motifs_asan_driver.cpp: csrc/motifs.inc built as a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in statically -
    the contig and every table in a heap block of exactly its size, contigs of 0, 1, U + D and U + D + 1 bases, the flanks at their limits."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'motifs_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'motifs_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'MOTIFS-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
