"""CPU: the line routine of `bsperf` compiled for the host (dm_bsperf_parse_host: the code the kernel of csrc/bsperf.hip.inc runs) against the Python
statement of readBed's rules, bsperf.HostEngine and bsperf.measures against tests/golden/bsperf_case.json (plain dicts, sklearn.metrics and
numpy.corrcoef: tests/golden/make_golden_bsperf.py), the refusals of the command line, and the routine under the address sanitizer
(tests/bsperf_asan_driver.cpp)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from deepmod_amd import bsperf, merge
from test_cluster import REAL

NAMES = ['chr1', 'chr10', 'chrX']
HEADER = 'chrom start end name score strand thickStart thickEnd rgb coverage percentage\n'
TABS = 'chr1\t1005\t1006\t.\t33\t+\t1005\t1006\t0,0,0\t33\t91\n'                  # ENCODE bedMethyl: tabs
BLANKS = 'chr1 7 8 . 5 - 7 8 0,0,0 5 0 \n'                                        # the detect dialect: single spaces, one before the newline
MIXED = ' \tchr10\t0  1 .\t\t1 - 0 1 0,0,0 \t2147483647 100\t \n'

VIOLATIONS = {
    '10 fields': 'chr1 5 6 . 7 + 5 6 0,0,0 42',
    '12 fields': 'chr1 5 6 . 7 + 5 6 0,0,0 7 42 3',
    'carriage return': 'chr1 5 6 . 7 + 5 6 0,0,0 7 42\r',
    'sign': 'chr1 +5 6 . 7 + 5 6 0,0,0 7 42',
    'sign on the coverage': 'chr1 5 6 . 7 + 5 6 0,0,0 -7 42',
    '11 digits': 'chr1 5 6 . 7 + 5 6 0,0,0 00000000007 42',
    'above int32': 'chr1 5 6 . 7 + 5 6 0,0,0 2147483648 42',
    'percentage 101': 'chr1 5 6 . 7 + 5 6 0,0,0 7 101',
    'beyond the contig': 'chr10 2000 2001 . 7 + 5 6 0,0,0 7 42',
}


def python_statement(text, names, first_chunk=True):
    """split(), int(), the first-line skip and the <= 20 skip -> ([(contig index, strand, position, coverage, percentage)], the six line counters)."""
    recs, lines = [], dict.fromkeys(bsperf.LINE_KEYS, 0)
    rows = text.split('\n')
    if rows[-1] == '':
        rows.pop()
    for no, line in enumerate(rows):
        if first_chunk and no == 0:
            lines['first_lines'] += 1
            continue
        line = line.strip()
        if len(line) <= 20:
            lines['short'] += 1
            continue
        f = line.split()
        assert len(f) == 11
        pos, cov, pct = int(f[1]), int(f[9]), int(f[10])
        if f[5] not in ('+', '-'):
            lines['other_strand'] += 1
        elif f[0] not in names:
            lines['other_contig'] += 1
        elif cov == 0:
            lines['zero_coverage'] += 1
        else:
            lines['records'] += 1
            recs.append((names.index(f[0]), '+-'.index(f[5]), pos, min(cov, 65535), pct))
    return recs, lines


def _as_rows(pos, meta):
    contig, strand, cov, pct = bsperf.unpack_meta(meta)
    return list(zip(contig.tolist(), strand.tolist(), np.asarray(pos).tolist(), cov.tolist(), pct.tolist()))


def _crafted_text():
    rng = np.random.default_rng(4)
    rows = []
    for i in range(600):
        name = ['chr1', 'chr10', 'chrX', 'chr', 'chr11', 'chr1_random'][int(rng.integers(0, 6))]
        pos = int(rng.integers(0, 2000))
        cov = int(rng.choice([0, 1, 4, 5, 9, 10, 65535, 65536, 2 ** 31 - 1]))
        strand = '+-.'[int(rng.integers(0, 3)) if i % 9 == 0 else int(rng.integers(0, 2))]
        f = [name, str(pos), str(pos + 1), '.', str(min(cov, 1000)), strand, str(pos), str(pos + 1), '0,0,0', str(cov), str(int(rng.integers(0, 101)))]
        kind = i % 4
        rows.append('\t'.join(f) + '\n' if kind == 0 else ' '.join(f) + ' \n' if kind == 1 else '  '.join(f) + '\n' if kind == 2 else ' \t' + ' \t '.join(f) + '\t\n')
    rows[50:50] = ['\n', '   \n', 'chr1 1 2 . 1 +\n', 'x' * 20 + '\n', ' ' + 'y' * 20 + '\t\n', 'chr1 9 10 . 1 + 9 10 0 1 5\n']      # short lines (20 bytes after the strip are short); a line of 26 bytes is kept
    return HEADER + TABS + BLANKS + MIXED + ''.join(rows)


def test_parser_equals_the_python_statement(hip_lib):
    text = _crafted_text()
    for t in (text, text[:-1]):                                                  # with and without the final newline
        for first in (True, False):
            tt = t if first else t[len(HEADER):]
            (pos, meta), lines, flag, bad = bsperf.parse_device_grammar(tt.encode(), NAMES, None, first)
            want, want_lines = python_statement(tt, NAMES, first)
            assert (flag, bad) == (0, -1)
            assert _as_rows(pos, meta) == want and len(want) > 150
            assert dict(zip(bsperf.LINE_KEYS, lines.tolist())) == want_lines and all(v > 0 for k, v in want_lines.items() if k != 'first_lines')
            hpos, hmeta, hlines = bsperf.host_rows(tt.encode(), NAMES, None, first)
            assert np.array_equal(hpos, pos) and np.array_equal(hmeta, meta) and np.array_equal(hlines, lines)
    names = {r[0] for r in python_statement(text, NAMES)[0]}
    assert names == {0, 1, 2}                                                    # chr1 beside chr10; chr, chr11, chr1_random are other contigs
    assert bsperf.parse_device_grammar(b'', NAMES)[2:] == (0, -1)
    # a first line outside the grammar is skipped unread only as the first line of a file
    odd = 'chr1 5 6 . 7 + 5 6 0,0,0 7 101\r\n' + TABS
    assert bsperf.parse_device_grammar(odd.encode(), NAMES, None, True)[2:] == (0, -1)
    assert bsperf.parse_device_grammar(odd.encode(), NAMES, None, False)[2:] == (1, 1)


@pytest.mark.parametrize("what", sorted(VIOLATIONS))
def test_every_violation_is_flagged_with_its_line(hip_lib, what):
    line = VIOLATIONS[what]
    lengths = [3000, 2000, None]
    for before in (0, 1, 7):
        text = HEADER + TABS * before + line + '\n' + BLANKS
        _, _, flag, bad = bsperf.parse_device_grammar(text.encode(), NAMES, lengths)
        assert (flag, bad) == (1, before + 2)
        _, _, flag, bad = bsperf.parse_device_grammar((TABS * before + line).encode(), NAMES, lengths, False)      # the last line, without its newline
        assert (flag, bad) == (1, before + 1)
    assert bsperf.parse_device_grammar((HEADER + TABS + BLANKS).encode(), NAMES, lengths)[2:] == (0, -1)
    if what == 'beyond the contig':                                              # inside when the length is not known, or one longer
        assert bsperf.parse_device_grammar((HEADER + line + '\n').encode(), NAMES, None)[2:] == (0, -1)
        assert bsperf.parse_device_grammar((HEADER + line + '\n').encode(), NAMES, [3000, 2001, None])[2:] == (0, -1)


def test_host_statement_hands_over_or_stops_with_file_and_line():
    text = (HEADER + 'chr1 5 6 . 7 + 5 6 0,0,0 7 42\r\n' + '\r\n' + 'chr1 9 10 . 7 - 9 10 0,0,0 +8 42 \r\n').encode()
    pos, meta, lines = bsperf.host_rows(text, NAMES, [100, 100, 100], True, 'rep1.bed')
    assert _as_rows(pos, meta) == [(0, 0, 5, 7, 42), (0, 1, 9, 8, 42)] and lines.tolist() == [2, 1, 1, 0, 0, 0]
    for body, line, why in (('chr1 5 6 . 7 + 5 6 0,0,0 7\n', 2, '10 fields'), ('chr1 5 6 . 7 + 5 6 0,0,0 7 42 3\n', 2, '12 fields'),
                            (TABS + 'chr1 5 6 . 7 + 5 6 0,0,0 x 42\n', 3, 'invalid literal'), ('chr1 5 6 . 7 + 5 6 0,0,0 7 101\n', 2, 'percentage 101'),
                            ('chr1 5 6 . 7 + 5 6 0,0,0 -7 42\n', 2, 'coverage -7'), (TABS * 3 + 'chr10 100 6 . 7 + 5 6 0,0,0 7 42\n', 5, 'position 100 is not on chr10')):
        with pytest.raises(bsperf.BsPerfError, match=r'rep1\.bed:%d: .*%s' % (line + 10, why)):
            bsperf.host_rows((HEADER + body).encode(), NAMES, [3000, 100, 100], True, 'rep1.bed', 11)


def load_golden():
    """tests/golden/bsperf_case.json, its histogram [label][bucket][percentage] made dense."""
    g = json.load(open(os.path.join(GOLDEN, 'bsperf_case.json')))
    hist = np.zeros((3, len(g['options']['cov']), bsperf.NPCT), np.int64)
    for label, bucket, pct, count in g['hist_nonzero']:
        hist[label, bucket, pct] = count
    g['hist'] = hist.tolist()
    return g


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _host_run(g, tmp_path):
    """The golden inputs through host_rows, merge.merge_beds and HostEngine -> (fetch(), options)."""
    o = g['options']
    names, R = o['chr'], len(g['truth'])
    eng = bsperf.HostEngine(names, o['cov'], R, o['methylated'], o['unmethylated'], o['predCov'])
    recs = []
    for text in g['truth']:
        pos, meta, lines = bsperf.host_rows(text.encode(), names)
        eng.add_lines(lines)
        recs.append((pos, meta, lines))
    for rel, text in g['pred'].items():
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    for c, ck in enumerate(names):
        _, pos, strand, cov, mod = merge.merge_beds(merge.find_bed_files(str(tmp_path), ck, o['Base']))
        sel = [bsperf.unpack_meta(m)[0] == c for _, m, _ in recs]
        length = int(max([int(pos.max()) + 1 if len(pos) else 1] + [int(p[s].max()) + 1 for (p, _, _), s in zip(recs, sel) if s.any()]))
        tabs = np.zeros((2, 2, length), np.int64)                                 # [strand][cov | mod]
        st = (strand == '-').astype(np.int64)
        tabs[st, 0, pos], tabs[st, 1, pos] = cov, mod
        eng.open(c, (tabs[0, 0], tabs[0, 1]), (tabs[1, 0], tabs[1, 1]))
        for r, ((p, m, _), s) in enumerate(zip(recs, sel)):
            eng.fill(r, p[s], m[s])
        eng.count()
    return eng.fetch(), [r[2] for r in recs]


def test_host_engine_equals_the_golden_case(golden, tmp_path):
    g = golden
    got, lines = _host_run(g, tmp_path)
    R = len(g['truth'])
    assert np.array_equal(got['hist'][0], np.array(g['hist'])) and got['hist'][0].sum() > 100 and got['hist'][1].sum() == 0
    assert np.array_equal(got['unpredicted'][0], np.array(g['unpredicted']))
    assert got['below_threshold'].tolist() == [g['below_threshold'], 0] and got['untruthed'].tolist() == [g['untruthed'], 0]
    for ln, want in zip(lines, g['line_counts']):
        assert dict(zip(bsperf.LINE_KEYS, ln.tolist())) == {k: want[k] for k in bsperf.LINE_KEYS} and int(ln.sum()) == want['seen']
    assert got['lines'].tolist() == np.sum(lines, axis=0).tolist()
    meas = bsperf.measures(got, g['options']['cov'], R)['raw']
    for t, want in g['measures'].items():
        m = meas[int(t)]
        for key in ('methylated', 'unmethylated', 'methylated_unpredicted', 'unmethylated_unpredicted', 'n'):
            assert m[key] == want[key], (t, key)
        assert m['methylated'] > 0 and m['unmethylated'] > 0
        for key in ('auc', 'ap', 'r', 'rmse'):
            print('threshold %s %s: %.17g, recorded %.17g' % (t, key, m[key], want[key]))
            assert abs(m[key] - want[key]) <= 1e-12 * abs(want[key]), (t, key, m[key], want[key])
    assert bsperf.report_lines({'raw': meas}) == g['report']


def test_measures_edges():
    r, rmse = bsperf.correlation([1, 5, 7, 35, 25, 49], 2)
    assert np.isnan(r) and np.isnan(rmse)                                        # n < 2
    r, rmse = bsperf.correlation([2, 10, 14, 70, 50, 100], 1)                    # x = 5, 5: no variance of x
    assert np.isnan(r) and rmse == pytest.approx(np.sqrt(((5 - 6) ** 2 + (5 - 8) ** 2) / 2), rel=1e-15)
    x, y = np.array([0, 50, 100, 30]), np.array([10, 120, 200, 40])              # y: the sum of two replicates
    r, rmse = bsperf.correlation([4, x.sum(), y.sum(), (x * y).sum(), (x * x).sum(), (y * y).sum()], 2)
    assert r == pytest.approx(np.corrcoef(x, y / 2)[0, 1], rel=1e-14) and rmse == pytest.approx(np.sqrt(np.mean((x - y / 2) ** 2)), rel=1e-14)
    big = 2 ** 33                                                                # sums of 2^33 sites stay exact in Python integers
    r, rmse = bsperf.correlation([2 * big, 100 * big, 100 * big, 10000 * big, 10000 * big, 10000 * big], 1)
    assert (r, rmse) == (1.0, 0.0)


def test_host_engine_refusals():
    eng = bsperf.HostEngine(['chr1'], (1, 5), 2)
    eng.open(0, (np.zeros(10), np.zeros(10)), (np.zeros(10), np.zeros(10)))
    meta = bsperf.pack_meta([0, 0], [0, 1], [5, 5], [90, 90])
    eng.fill(0, [3, 3], meta)                                                    # one position on both strands: two keys
    eng.fill(1, [3], meta[:1])                                                   # the same key in another replicate is no duplicate
    with pytest.raises(bsperf.BsPerfError, match='replicate 1 holds position 3 of strand \\+ twice'):
        eng.fill(1, [3], meta[:1])
    with pytest.raises(bsperf.BsPerfError, match='refused'):
        eng.count()
    eng.open(0, (np.zeros(10), np.zeros(10)), (np.zeros(10), np.zeros(10)))
    with pytest.raises(bsperf.BsPerfError, match='replicate 0 holds position 4 of strand - twice'):
        eng.fill(0, [7, 4, 7, 4], bsperf.pack_meta([0] * 4, [1] * 4, [5] * 4, [0] * 4))
    with pytest.raises(bsperf.BsPerfError, match='outside the open contig'):
        eng.fill(0, [10], meta[:1])
    for kw, words in (({'thresholds': ()}, '1 to 8'), ({'thresholds': (5, 5)}, 'ascending'), ({'thresholds': (0, 5)}, 'positive'), ({'replicates': 5}, '1 to 4'),
                      ({'methylated': 0}, 'unmethylated < methylated'), ({'pred_cov': 0}, '1 or more')):
        with pytest.raises(bsperf.BsPerfError, match=words):
            bsperf.HostEngine(['chr1'], **kw)
    for names in ([], ['c%d' % i for i in range(65)], ['k' * 64], ['a b'], ['chr1', 'chr1']):
        with pytest.raises(bsperf.BsPerfError, match='--chr'):
            bsperf.HostEngine(names)


def _bsperf(args, env=None):
    e = dict(os.environ)
    e.pop('DEEPMOD_CLUSTER_MODEL', None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'bsperf'] + args, capture_output=True, text=True, timeout=300, env=e)


def test_command_line_refusals(tmp_path):
    """One line each, before any file is read or a GPU asked for."""
    runs = tmp_path / 'runs'
    runs.mkdir()
    out = tmp_path / 'out'
    fasta = tmp_path / 'genome.fa'
    fasta.write_text('>chr1 test\nACGCGT\n')
    rep = tmp_path / 'rep1.bed'
    rep.write_text(HEADER + TABS)
    reps = ','.join([str(rep)] * 5)
    common = ['--predFolder', str(runs), '--truth', str(rep), '--outFolder', str(out)]
    for args, words in (([], ('--predFolder',)),
                        (['--predFolder', str(runs)], ('--truth', 'are needed')),
                        (['--predFolder', str(runs), '--truth', str(tmp_path / 'no.bed')], ('--truth', 'does not exist')),
                        (['--predFolder', str(runs), '--truth', reps], ('--truth', '1 to 4')),
                        (['--predFolder', str(tmp_path / 'nothing'), '--truth', str(rep)], ('--predFolder', 'does not exist')),
                        (common + ['--cov', '1,x'], ('--cov', 'integers')),
                        (common + ['--cov', '5,1'], ('--cov', 'ascending')),
                        (common + ['--cov', '0,1'], ('--cov', 'positive')),
                        (common + ['--cov', '1,2,3,4,5,6,7,8,9'], ('--cov', '1 to 8')),
                        (common + ['--predCov', '0'], ('--predCov', '1 or more')),
                        (common + ['--methylated', '101'], ('--methylated', '<= 100')),
                        (common + ['--methylated', '10', '--unmethylated', '10'], ('--unmethylated', 'unmethylated < methylated')),
                        (common + ['--chr', ','.join('c%d' % i for i in range(65))], ('--chr', '1 to 64')),
                        (common + ['--chr', 'k' * 64], ('--chr', '1 to 63 printable')),
                        (common + ['--Ref', str(tmp_path / 'no.fa')], ('--Ref', 'does not exist')),
                        (common + ['--clusterCpG', REAL], ('--clusterCpG', 'needs --Ref')),
                        (common + ['--Ref', str(fasta), '--clusterCpG'], ('--clusterCpG', 'no cluster-model checkpoint')),
                        (common + ['--Ref', str(fasta), '--clusterCpG', REAL, '--Base', 'A'], ('--clusterCpG', '--Base C only')),
                        (common + ['--Ref', str(fasta), '--clusterCpG', REAL, '--chr', 'chr1,chr9'], ('--clusterCpG', 'holds no contig chr9'))):
        res = _bsperf(args)
        last = res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ''
        assert res.returncode != 0 and last.startswith('Error: bsperf: ') and all(w in last for w in words), (args, res.stderr[-2000:])
    assert os.listdir(runs) == [] and not out.exists()


def test_line_routine_under_address_sanitizer(tmp_path):
    """tests/bsperf_asan_driver.cpp: csrc/bsperf.inc built as a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in statically -
    every text and record array in a heap block of exactly its size; texts cut at every byte, record capacities one short."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'bsperf_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'bsperf_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'BSPERF-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
