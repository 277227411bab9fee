"""CPU: the line routines of `merge` compiled for the host (dm_bedmerge_parse_host, dm_bedmerge_format_host: the code the kernels of
csrc/bedmerge.hip.inc run) against merge.readbed2 and merge.save_mod, the refusals of the command line, and the routines under the address
sanitizer (tests/merge_asan_driver.cpp).  Reference: DeepMod_tools/sum_chr_mod.py through merge.py, which tests/golden/merge_case.json holds to it."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import merge
from test_cluster import REAL

DETECT = 'chr1 1005 1006 C 33 + 1005 1006 0,0,0 33 24 8 \n'                     # what detect writes: a space before the newline
MERGED = 'chr1 1005 1006 C 47 -  1005 1006 0,0,0 47 34 16\n'                    # sum_chr_mod.py: two spaces after the strand
CLUSTERED = 'chr1 7 8 C 1000 +  7 8 0,0,0 1500 46 700 61\n'                     # hm_cluster_predict.py: 13 fields
MIXED = ' \tchr1\t0  1 C\t\t1 - 0 1 0,0,0 \t2147483647 0 2147483647\t \n'

VIOLATIONS = {
    'carriage return': 'chr1 5 6 C 7 + 5 6 0,0,0 7 42 3\r',
    'blank line': '',
    'another contig': 'chr2 5 6 C 7 + 5 6 0,0,0 7 42 3',
    'sign': 'chr1 +5 6 C 7 + 5 6 0,0,0 7 42 3',
    '11 fields': 'chr1 5 6 C 7 + 5 6 0,0,0 7 42',
    '11 digits': 'chr1 5 6 C 7 + 5 6 0,0,0 7 42 00000000003',
    'above int32': 'chr1 5 6 C 7 + 5 6 0,0,0 2147483648 42 3',
    'strand': 'chr1 5 6 C 7 * 5 6 0,0,0 7 42 3',
    'modified above coverage': 'chr1 5 6 C 7 + 5 6 0,0,0 7 42 8',
    'beyond the table': 'chr1 2000 2001 C 7 + 5 6 0,0,0 7 42 3',
}


def _readbed2(tmp_path, text):
    p = tmp_path / 'x.bed'
    p.write_text(text)
    return merge.readbed2(str(p))


def test_parser_equals_readbed2_on_the_three_dialects(hip_lib, tmp_path):
    rng = np.random.default_rng(2)
    rows = []
    for i in range(400):
        cov = int(rng.integers(0, 3000))
        mod = int(rng.integers(0, cov + 1))
        pos = int(rng.integers(0, 2000))
        strand = '+-'[int(rng.integers(0, 2))]
        head = 'chr1 %d %d C %d %s' % (pos, pos + 1, min(cov, 1000), strand)
        tail = '%d %d 0,0,0 %d %d %d' % (pos, pos + 1, cov, mod * 100 // max(cov, 1), mod)
        kind = i % 4
        rows.append(head + ' ' + tail + ' \n' if kind == 0 else head + '  ' + tail + '\n' if kind == 1 else head + '  ' + tail + ' %d\n' % (i % 101) if kind == 2
                    else '\t' + (head + ' ' + tail).replace(' ', ' \t ') + '\n')
    text = DETECT + MERGED + CLUSTERED + MIXED + ''.join(rows)
    for t in (text, text[:-1]):                                                  # with and without the final newline
        (pos, strand, cov, mod), flag, bad = merge.parse_device_grammar(t.encode(), 'chr1', 2000)
        chrom, rpos, rstrand, rcov, rmod = _readbed2(tmp_path, t)
        assert (flag, bad) == (0, -1) and len(pos) == 404
        assert np.array_equal(pos, rpos) and np.array_equal(cov, rcov) and np.array_equal(mod, rmod) and np.array_equal(strand, (rstrand == '-').astype(np.uint8))
        assert set(chrom.tolist()) == {'chr1'}
    assert merge.parse_device_grammar(b'', 'chr1')[1:] == (0, -1)


@pytest.mark.parametrize("what", sorted(VIOLATIONS))
def test_every_violation_is_flagged_with_its_line(hip_lib, what):
    line = VIOLATIONS[what]
    for before in (0, 1, 7):
        text = DETECT * before + line + '\n' + MERGED
        (pos, _, _, _), flag, bad = merge.parse_device_grammar(text.encode(), 'chr1', 2000)
        assert flag == 1 and bad == before + 1 and len(pos) == before + 2
    inside = merge.parse_device_grammar((DETECT + MERGED).encode(), 'chr1', 2000)
    assert inside[1:] == (0, -1)


def _merged(chrom, rows):
    """rows [(pos, strand, cov, mod)] -> the tuple merge.save_mod takes, in its order."""
    rows = sorted(rows, key=lambda r: (r[0], r[1]))
    return (np.array([chrom] * len(rows), object), np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], object),
            np.array([r[2] for r in rows], np.int64), np.array([r[3] for r in rows], np.int64))


def _format_windows(chrom, base, rows):
    """The rows through dm_bedmerge_format_host: one call per window of two positions (the tables of positions p, p + 1)."""
    text, done = b'', set()
    for p in sorted({r[0] for r in rows}):
        if p in done:
            continue
        done.update((p, p + 1))
        tabs = np.zeros((4, 2), np.int32)
        for q, s, cv, md in rows:
            if q in (p, p + 1):
                tabs[2 * (s == '-'), q - p], tabs[2 * (s == '-') + 1, q - p] = cv, md
        length = 2 if p + 1 <= merge.MAX_LENGTH - 1 else 1
        text += merge.format_host(chrom, base, *[t[:length] for t in tabs], first_pos=p)
    return text


def _save_mod(tmp_path, chrom, base, rows):
    p = str(tmp_path / 'want.bed')
    merge.save_mod(p, _merged(chrom, rows), base)
    return open(p, 'rb').read()


@pytest.mark.parametrize("chrom,base", [('c', 'C'), ('chr1', 'A'), ('k' * 255, 'C')])
def test_formatter_equals_save_mod(hip_lib, tmp_path, chrom, base):
    rng = np.random.default_rng(5)
    rows = []
    p = 10
    while p <= 10 ** 9:                                                          # position and position + 1 at every digit-count step
        rows += [(p - 2, '+', 5, 1), (p - 1, '-', 5, 2), (p - 1, '+', 999, 999), (p, '+', 1000, 1), (p, '-', 1001, 1001), (p + 1, '-', 2 ** 31 - 1, 2 ** 31 - 1)]
        p *= 10
    rows += [(2 ** 31 - 2, '+', 7, 3), (2 ** 31 - 2, '-', 2 ** 31 - 1, 1), (2 ** 31 - 3, '-', 7, 7)]      # the largest position
    rows += [(20000 + 3 * m, '+', 100, m) for m in range(101)]                   # every pct; mod == 0 is dropped
    rows += [(30000 + 3 * m, '-', 2 ** 31 - 1, m * (2 ** 31 - 1) // 100) for m in range(1, 101)]
    rows += [(40000, '+', 200, 1), (40001, '-', 9, 0), (40001, '+', 0, 0)]       # pct 0 of a written row; rows that are dropped
    for i in range(300):                                                         # random sums up to the int32 range
        cov = int(rng.integers(1, 2 ** 31 if i % 2 else 5000))
        rows.append((50000 + 3 * i, '+-'[i % 2], cov, int(rng.integers(0, cov + 1))))
    got, want = _format_windows(chrom, base, rows), _save_mod(tmp_path, chrom, base, rows)
    assert got == want and want.count(b'\n') > 400
    # one table of many positions, both strands, against the same writer
    n = 5000
    cov = rng.integers(0, 1500, (2, n)).astype(np.int32)
    mod = (cov * rng.random((2, n)) ** 2).astype(np.int32)
    rows = [(700 + int(i), '+-'[s], int(cov[s, i]), int(mod[s, i])) for s in range(2) for i in range(n)]
    assert merge.format_host(chrom, base, cov[0], mod[0], cov[1], mod[1], first_pos=700) == _save_mod(tmp_path, chrom, base, rows)
    assert merge.format_host(chrom, base, None, None, cov[1], mod[1], first_pos=700) == _save_mod(tmp_path, chrom, base, [r for r in rows if r[1] == '-'])
    assert merge.format_host(chrom, base, cov[0, :0], mod[0, :0], None, None) == b''


def test_formatter_refusals(hip_lib):
    from deepmod_amd import _lib
    one = np.array([5], np.int32)
    text = merge.format_host('chr1', 'C', one, one, None, None)
    assert text == b'chr1 0 1 C 5 +  0 1 0,0,0 5 100 5\n'
    with pytest.raises(merge.MergeError, match='needs %d bytes' % len(text)):
        merge.format_host('chr1', 'C', one, one, None, None, cap=len(text) - 1)            # a capacity one byte short: nothing is written
    with pytest.raises(_lib.DeepModHipError, match='0 <= modified <= coverage'):
        merge.format_host('chr1', 'C', one, one + 1, None, None)
    with pytest.raises(_lib.DeepModHipError, match='2\\^31 - 2'):
        merge.format_host('chr1', 'C', one, one, None, None, first_pos=2 ** 31 - 1)
    for name in ('', 'k' * 256, 'a b'):
        with pytest.raises(_lib.DeepModHipError, match='contig name'):
            merge.format_host(name, 'C', one, one, None, None)
    assert merge.tile_positions() == 1024


def test_host_rows_hand_over_or_stop_with_file_and_line(tmp_path):
    p = tmp_path / 'mod_pos.chr1+.C.bed'
    p.write_text('chr1 5 6 C 7 + 5 6 0,0,0 7 42 3\r\n\nchr1 9 10 C 7 - 9 10 0,0,0 +8 42 3 \r\n')
    pos, strand, cov, mod = merge.host_rows(str(p), 'chr1', 100)
    assert pos.tolist() == [5, 9] and strand.tolist() == [0, 1] and cov.tolist() == [7, 8] and mod.tolist() == [3, 3]
    for body, line, why in (('chr1 5 6 C 7 + 5 6 0,0,0 7 42 3\nchr2 5 6 C 7 + 5 6 0,0,0 7 42 3\n', 2, 'a line of chr2 in a file named for chr1'),
                            ('\nchr1 5 6 C 7 + 5 6 0,0,0 7 42\n', 2, '11 fields'), ('chr1 5 6 C 7 + 5 6 0,0,0 7 42 x\n', 1, 'invalid literal'),
                            ('chr1 5 6 C 7 + 5 6 0,0,0 7 42 8\n', 1, 'outside 0 <= modified <= coverage'), ('chr1 5 6 C 7 . 5 6 0,0,0 7 42 3\n', 1, 'strand'),
                            ('chr1 5 6 C 7 + 5 6 0,0,0 7 42 3\n' * 3 + 'chr1 100 6 C 7 + 5 6 0,0,0 7 42 3\n', 4, 'position 100 is not on chr1')):
        p.write_text(body)
        with pytest.raises(merge.MergeError, match=r'mod_pos\.chr1\+\.C\.bed:%d: .*%s' % (line, why)):
            merge.host_rows(str(p), 'chr1', 100)


def _merge(args, env=None):
    e = dict(os.environ)
    e.pop('DEEPMOD_CLUSTER_MODEL', None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'merge'] + args, capture_output=True, text=True, timeout=300, env=e)


def test_command_line_refusals(tmp_path):
    """One line each, before any BED file is read or a GPU asked for."""
    runs = tmp_path / 'runs'
    runs.mkdir()
    fasta = tmp_path / 'genome.fa'
    fasta.write_text('>chr1 test\nACGCGT\n')
    common = ['--predFolder', str(runs), '--FileID', 'sum']
    for args, env, words in (([], None, ('--predFolder',)),
                             (['--predFolder', str(tmp_path / 'nothing')], None, ('--predFolder', 'does not exist')),
                             (common + ['--clusterCpG', REAL], None, ('--clusterCpG', 'needs --Ref')),
                             (common + ['--Ref', str(fasta), '--clusterCpG'], None, ('--clusterCpG', 'no cluster-model checkpoint')),
                             (common + ['--Ref', str(fasta), '--clusterCpG'], {'DEEPMOD_CLUSTER_MODEL': str(tmp_path / 'nothing')}, ('no cluster-model checkpoint at',)),
                             (common + ['--Ref', str(fasta), '--clusterCpG', REAL, '--Base', 'A'], None, ('--clusterCpG', '--Base C only')),
                             (common + ['--Ref', str(fasta), '--clusterCpG', REAL, '--chr', 'chr1,chr9'], None, ('--clusterCpG', 'holds no contig chr9')),
                             (common + ['--Ref', str(tmp_path / 'no.fa')], None, ('--Ref', 'does not exist'))):
        res = _merge(args, env)
        last = res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ''
        assert res.returncode != 0 and last.startswith('Error: ') and all(w in last for w in words), (args, res.stderr[-2000:])
    assert os.listdir(runs) == []


def test_line_routines_under_address_sanitizer(tmp_path):
    """tests/merge_asan_driver.cpp: csrc/bedmerge.inc built as a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in statically -
    every text, record array, table and output in a heap block of exactly its size; texts cut at every byte, a missing final newline, a capacity one
    byte short."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'merge_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'merge_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'MERGE-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
