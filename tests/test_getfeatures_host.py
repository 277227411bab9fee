"""CPU: `getfeatures` against the reference's own results (tests/golden/getfeatures/, written by make_golden_getfeatures.py from
myGetFeatureBasedPos.handle_record / get_Feature / readFA / readMotifMod).  The compiled walk (dm_xy_read), the numpy statement of the device stage
(getfeatures.xy_rows_np) and the writer together give the golden bytes; the compiled host form of the device stage (dm_xy_rows_host), the text
definition (dm_xy_format_host) and the kernels' formatting rule are held to Python's '%.3f'; the command line refuses what is not built."""
import glob
import gzip
import json
import os
import shutil
import subprocess
import sys
from collections import defaultdict

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from deepmod_amd import _lib, getfeatures as gf, rawreads, readmap, train

SCENARIOS = ['cg_neg', 'three_files', 'cg_pos', 'cg_pos_share', 'gatc_pos', 'gatc_neg', 'ccagg_pos', 'lists_neg', 'lists_pos']
CLI = os.path.join(ROOT, 'bin', 'DeepMod.py')


def load_golden(name):
    with gzip.open(os.path.join(GOLDEN, 'getfeatures', name + '.json.gz')) as fh:
        return json.loads(fh.read().decode())


def as_lists(sites_per_contig):
    """{contig: {'+': arr, '-': arr}} -> {contig: sorted [strand, pos] pairs}, the golden's form (contigs without a position left out)"""
    out = {}
    for c, per in sites_per_contig.items():
        pairs = sorted([s, int(p)] for s, arr in per.items() for p in arr)
        if pairs:
            out[c] = pairs
    return out


def setup_scenario(g, tmp_path, hip_lib):
    """-> (moptions, f5data, f5align) of a golden scenario, the position lists built by this project's own readFA / readMotifMod / readPosFiles"""
    fasta = tmp_path / 'genome.fa'
    fasta.write_text(g['fasta'])
    fadict = gf.readFA(str(fasta))
    mo = {'Ref': str(fasta), 'region': [None, None, None], 'fnum': 7, 'outLevel': 2, 'fadict': fadict, **g['options']}
    if g['options']['motifORPos'] == 1:
        mo['motif'] = g['motif']
        ful, _ = gf.readMotifMod(fadict, g['motif'][0], g['motif'][1])
        assert as_lists(ful) == {c: v for c, v in g['lists']['fulmodlist'].items() if v}, 'readMotifMod differs from the reference'
        mo['sites'] = gf.SiteLists(list(fadict), ful)
    else:
        lists = []
        for key in ('fulmodlist', 'anymodlist', 'nomodlist'):
            fn = tmp_path / (key + '.txt')
            fn.write_text(''.join('%s %s %d\n' % (c, s, p) for c, pairs in g['lists'][key].items() for s, p in pairs))
            lists.append(gf.readPosFiles(str(fn), fadict))
            assert as_lists(lists[-1]) == g['lists'][key]
        mo['sites'] = gf.SiteLists(list(fadict), *lists)
    f5data, f5align = {}, {}
    for r in g['reads']:
        ev = np.zeros(len(r['basecall']), dtype=rawreads.EVENT_DTYPE)
        ev['mean'], ev['stdv'], ev['length'] = r['ev_mean'], r['ev_stdv'], r['ev_length']
        ev['start'] = np.cumsum(np.r_[0, ev['length'][:-1]])
        ev['model_state'] = ['NN' + b + 'NN' for b in r['basecall']]
        f5data[r['name']] = (r['basecall'], ev, None, '/wrk/' + r['name'] + '.fast5', (0, 0))
        f5align[r['name']] = (60, r['flag'], r['rname'], r['pos'], r['cigar'], r['seq'])
    return mo, f5data, f5align


def written_files(folder):
    out = {}
    for fn in glob.glob(os.path.join(str(folder), '*.xy.gz')):
        k = os.path.basename(fn).split('.')[0]
        out[k] = {'xy': gzip.open(fn, 'rt').read(), 'ind': open(fn[:-3] + '.ind').read()}
    return out


@pytest.mark.parametrize('name', SCENARIOS)
def test_golden_bytes(name, tmp_path, hip_lib):
    """walk + numpy statement + writer = the reference's files, byte for byte after decompression, and its error channel; every file loads in train"""
    g = load_golden(name)
    mo, f5data, f5align = setup_scenario(g, tmp_path, hip_lib)
    out = tmp_path / 'out'
    out.mkdir()
    sp_options = {'ctfolder': str(out), 'Error': defaultdict(list)}
    gf.handle_record(mo, sp_options, {'f5data': f5data, 'ref_info': {}}, f5align, f5data)
    got = written_files(out)
    assert sorted(got) == sorted(g['files'])
    for k in g['files']:
        assert got[k]['ind'] == g['files'][k]['ind'], (name, k)
        assert got[k]['xy'] == g['files'][k]['xy'], (name, k)
    assert {k: list(v) for k, v in sp_options['Error'].items()} == g['errors']
    tmo = {'windowsize': 21, 'test': ['N', '100']}
    for fn in sorted(glob.glob(str(out / '*.xy.gz'))):
        x, y, _ = train.getDataFromFile_new(fn, tmo)
        table = np.loadtxt(fn, ndmin=2)
        assert len(x) == len(y) == int(((table[:, 1] > 0.5) | (table[:, 2] > 0.5)).sum()) and (len(x) == 0 or np.asarray(x).shape[1:] == (21, 7))
    mo['sites'].close()


def test_golden_cases_are_what_the_issue_names():
    """the fixtures hold the cases they were made for (a maker that drifts would leave the byte tests passing on less)"""
    g = load_golden('cg_neg')
    ind = g['files']['0']['ind']
    assert g['errors'] == {'Less(<500) events': ['/wrk/short_499.fast5']}
    for absent in ('short_499', 'no_site_contig', 'no_labelled_row'):
        assert absent not in ind
    assert 'aligned_500' in ind and 'rev_to_contig_end' in ind and 'fwd_from_contig_start' in ind
    assert any(c.islower() for c in g['fasta']) and 'N' * 12 in g['fasta'].replace('\n', '').upper()
    ful = g['lists']['fulmodlist']['chrS']
    assert ['+', 0] in ful and ['-', 8999] in ful and 'chrQ' not in {c for c, v in g['lists']['fulmodlist'].items() if v}
    assert len(load_golden('three_files')['files']) == 3
    # kept shares: 1,299 and 1,300 aligned events keep n + 50 rows of n + 200 (not above 0.9), 1,310 keep all 1,510
    rows = lambda gg, k, name: [int(ln.split()[0]) for ln in gg['files'][k]['ind'].splitlines()] + [gg['files'][k]['xy'].count('\n')]
    share = load_golden('cg_pos_share')
    first = rows(share, '0', None)
    assert first[1] - first[0] == 1350 and first[2] - first[1] == 1510
    pos = load_golden('cg_pos')
    first = rows(pos, '0', None)
    assert first[-1] - first[-2] == 1349
    assert any(float(ln.split()[2]) == 1.0 for ln in pos['files']['0']['xy'].splitlines()[:2000])      # positive labels exist


@pytest.mark.parametrize('name', ['cg_pos', 'lists_pos', 'gatc_neg'])
def test_rows_host_equals_the_numpy_statement(name, tmp_path, hip_lib):
    """dm_xy_rows_host (what dm_xy_rows falls back to) on a batch of all reads = xy_rows_np: text, keep, row and byte offsets"""
    g = load_golden(name)
    mo, f5data, f5align = setup_scenario(g, tmp_path, hip_lib)
    walked, ev3, ev0, row0 = [], [], 0, 0
    for readk, (mapq, flag, rname, pos, cigar, seq) in f5align.items():
        ev = f5data[readk][1]
        w = gf.walk_read(mo, mo['sites'], rname, flag, pos, cigar, seq, mo['fadict'][rname].encode(), len(ev), row0, ev0)
        if w['status'] != _lib.DM_XY_OK:
            continue
        walked.append(w)
        ev3.append(gf._event_block(ev))
        ev0 += len(ev)
        row0 += len(w['pos'])
    pos, lab, code = (np.concatenate([w[k] for w in walked]) for k in ('pos', 'lab', 'code'))
    rdesc, ev3 = np.stack([w['rdesc'] for w in walked]), np.concatenate(ev3)
    want = gf.xy_rows_np(pos, lab, code, rdesc, ev3)
    got = gf.rows_host(pos, lab, code, rdesc, ev3)
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(a, b)
    assert b''.join(v['xy'].encode() for v in g['files'].values()) == want[0]
    mo['sites'].close()


def test_get_feature_from_a_table_equals_the_walk(tmp_path, hip_lib):
    """get_Feature on dm_map_read's columns (the CpG swap applied, as with motif CG) = the rows dm_xy_read gives; isdif is False for matching events"""
    g = load_golden('cg_pos')
    mo, f5data, f5align = setup_scenario(g, tmp_path, hip_lib)
    for readk in ('swap_fwd', 'swap_rev', 'site_indels_rev', 'gappy_fwd'):
        mapq, flag, rname, pos, cigar, seq = f5align[readk]
        ref = mo['fadict'][rname]
        mp = readmap.map_read(flag, pos, cigar, seq, ref, len(f5data[readk][1]))
        m, isdif = gf.get_Feature(mo, {}, {'f5data': f5data}, f5align, f5data, readk, mp['leftclip'], mp['rightclip'], mp['base_map_info'], mp['strand'],
                                  rname, mp['first_match_pos'], mp['num_insertions'], mp['num_deletions'])
        w = gf.walk_read(mo, mo['sites'], rname, flag, pos, cigar, seq, ref.encode(), len(f5data[readk][1]))
        text = gf.xy_rows_np(w['pos'], w['lab'], w['code'], w['rdesc'], gf._event_block(f5data[readk][1]))[0]
        assert gf.xy_text_np(m) == text and not isdif
    mo['sites'].close()


def test_statuses_and_damaged_tables(tmp_path, hip_lib):
    g = load_golden('cg_neg')
    mo, f5data, f5align = setup_scenario(g, tmp_path, hip_lib)
    st = {}
    for readk, (mapq, flag, rname, pos, cigar, seq) in f5align.items():
        st[readk] = gf.walk_read(mo, mo['sites'], rname, flag, pos, cigar, seq, mo['fadict'][rname].encode(), len(f5data[readk][1]))['status']
    assert st['short_499'] == _lib.DM_XY_LESS_EVENT and st['no_site_contig'] == _lib.DM_XY_NO_SITE and st['aligned_500'] == _lib.DM_XY_OK
    mapq, flag, rname, pos, cigar, seq = f5align['aligned_500']
    wrong = ''.join({'A': 'C', 'C': 'A', 'G': 'T', 'T': 'G'}[b] for b in seq)
    assert gf.walk_read(mo, mo['sites'], rname, flag, pos, cigar, wrong, mo['fadict'][rname].encode(), len(seq))['status'] == _lib.DM_XY_NO_MATCH
    with pytest.raises(_lib.DeepModHipError):
        gf.walk_read(mo, mo['sites'], rname, flag, pos, '5000M', seq, mo['fadict'][rname].encode(), len(seq))
    # descriptors that do not fit their arrays are refused before anything is indexed
    w = gf.walk_read(mo, mo['sites'], rname, flag, pos, cigar, seq, mo['fadict'][rname].encode(), len(seq))
    ev3 = gf._event_block(f5data['aligned_500'][1])
    for col, value in ((0, 5), (2, -1), (3, len(ev3) + 1), (1, 1 << 50)):
        bad = w['rdesc'].copy()
        bad[col] = value
        with pytest.raises(_lib.DeepModHipError):
            gf.rows_host(w['pos'], w['lab'], w['code'], bad, ev3)
    two = np.stack([w['rdesc'], w['rdesc']])
    two[1, 0] = len(w['pos']) + 7                          # the second read starts behind the last row
    with pytest.raises(_lib.DeepModHipError):
        gf.rows_host(w['pos'], w['lab'], w['code'], two, ev3)
    mo['sites'].close()


def test_host_functions_under_address_sanitizer(tmp_path):
    """tests/xy_asan_driver.cpp: csrc/xyrows.inc behind tests/asan/host_shim.cpp, built as a PROGRAM with -fsanitize=address,undefined (the sanitizer's
    runtime linked in statically) - every array in a heap block of exactly its size; valid batches against a plain restatement, damaged descriptor
    tables, CIGARs past their sequences, outputs that are too small."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'xy_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'xy_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'XY-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]


# ------------------------------------------------------------------------------------------------ the text
F32 = np.float32
NAMED_VALUES = [0.0625, 0.1875, 1.0625, 2.6875, -2.6875, -0.0, -0.0004, 0.0005, 9.9995, 9.9996, 99999.9996, 16777216.0, 2.0 ** 30, 3.4e38,
                float('nan'), float('inf'), float('-inf')]


def sweep_values():
    """1.7e5 random fp32 bit patterns below 2^30 in magnitude, and every k / 2000 for |k| <= 20,000 with both fp32 neighbours"""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, 400000, dtype=np.uint64).astype(np.uint32)
    v = bits.view(np.float32)
    v = v[np.isfinite(v) & (np.abs(v) < 2.0 ** 30)][:170000]
    assert len(v) == 170000
    ties = (np.arange(-20000, 20001) / 2000.0).astype(np.float32)
    return np.concatenate([v, ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf))])


def test_format_host_equals_python_percent(hip_lib):
    vals = np.array(NAMED_VALUES + [float(F32(v)) for v in NAMED_VALUES], np.float64)
    rows = np.zeros((len(vals), 10))
    rows[:, 0], rows[:, 7], rows[:, 9] = vals, vals[::-1], vals
    want = ''.join(' '.join('%.3f' % v for v in row) + '\n' for row in rows).encode()
    assert gf.format_host(rows) == want
    assert b'nan' in want and b'-inf' in want and b'-0.000' in want and b'10.000' in want and b'1073741824.000' in want
    sweep = sweep_values().astype(np.float64)
    sweep = sweep[:len(sweep) // 10 * 10].reshape(-1, 10)
    assert gf.format_host(sweep) == ''.join(' '.join('%.3f' % v for v in row) + '\n' for row in sweep).encode()
    # sized first: a buffer that is too small is not written
    buf = np.full(8, 7, np.uint8)
    assert hip_lib.dm_xy_format_host(rows.ctypes.data, 1, buf.ctypes.data, 8) > 8 and (buf == 7).all()


def test_formatting_rule_of_the_kernels_equals_python_percent():
    for v in sweep_values():
        assert gf.format_value_rule(v) == '%.3f' % float(v), float(v)
    for v in NAMED_VALUES:
        v32 = F32(v)
        if np.isfinite(v32) and abs(v32) < 2.0 ** 30:
            assert gf.format_value_rule(v32) == '%.3f' % float(v32), v


def test_integer_form_of_the_keep_rule():
    """len(keepInd) > len(mfeatures) * 0.9 (double) is 10 kept > 9 n for every row count up to 4e7, at the counts where the two could part"""
    n = np.arange(1, 40_000_001, dtype=np.int64)
    edge = (9 * n) // 10
    for k in (edge - 1, edge, edge + 1):
        assert np.array_equal(k > n * 0.9, 10 * k > 9 * n)


def test_keep_statement_edges():
    """the numpy statement itself on hand-made reads: window of 25, the window cut at the read, 0.9 strictly, nothing kept"""
    def keep(labelled, sizes):
        lab = np.zeros(sum(sizes), np.uint8)
        lab[labelled] = 1
        rdesc = np.zeros((len(sizes), 4), np.int64)
        rdesc[:, 0] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        return gf.xy_keep_np(lab, rdesc)
    k, off = keep([100, 151, 300, 352], [700])
    assert k[75:177].all() and not k[74] and not k[177] and k[275:326].all() and not k[326] and k[327:378].all() and off.tolist() == [0, 102 + 51 + 51]
    k, off = keep([699, 700], [700, 700, 700])             # the last row of read 0 and the first of read 1
    assert k[674:700].all() and not k[673] and k[700:726].all() and not k[726] and off.tolist() == [0, 26, 52, 52]
    lab_rows = list(range(25, 867, 51)) + [874]            # rows 0 .. 899 kept: exactly 9/10 of 1,000 rows (not above), above for 999, below for 1,001
    for n, all_kept in ((999, True), (1000, False), (1001, False)):
        k, off = keep(lab_rows, [n])
        assert int(k[:900].sum()) == 900 and int(off[-1]) == (n if all_kept else 900), n
    k, off = keep([], [700])
    assert not k.any() and off.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ the command line
def run_cli(*args):
    p = subprocess.run([sys.executable, CLI, 'getfeatures', *args], capture_output=True, text=True)
    return p.returncode, [ln for ln in (p.stdout + p.stderr).splitlines() if ln.strip()]


def test_cli_refusals_print_one_line_each(tmp_path):
    wrk = tmp_path / 'wrk'
    wrk.mkdir()
    ref = tmp_path / 'ref.fa'
    ref.write_text('>c\nACGT\n')
    base = ['--wrkBase', str(wrk), '--Ref', str(ref), '--outFolder', str(tmp_path / 'out')]
    held = tmp_path / 'held' / '0'
    held.mkdir(parents=True)
    (held / '0.xy.gz').write_bytes(b'')
    cases = [(base + ['--fnum', '57'], '--fnum 7 only'),
             (base + ['--SignalGroup', 'rundif'], '--SignalGroup rundif'),
             (base + ['--region', 'c:10:200'], '--region takes a contig name only'),
             (base + ['--region', 'c:10'], '--region takes a contig name only'),
             (base + ['--motifORPos', '2', '--fulmod', 'a', '--nomod', 'b'], 'needs --fulmod, --anymod and --nomod (missing: --anymod)'),
             (base + ['--motifORPos', '3'], '--motifORPos 3 is not supported'),
             (base[:4] + ['--outFolder', str(tmp_path / 'held')], 'already holds */*.xy.gz'),
             (['--wrkBase', str(wrk), '--Ref', str(tmp_path / 'missing.fa')], 'reference file does not exist')]
    for args, text in cases:
        rc, lines = run_cli(*args)
        assert rc != 0 and len(lines) == 1 and lines[0].startswith('Error: getfeatures:') and text in lines[0], (args, lines)
    assert (held / '0.xy.gz').exists()                      # refused, not deleted
