"""CPU: bslabels.HostEngine and bslabels.format_lists_host against tests/golden/bslabels_case.json (plain dicts over readBed's rules:
tests/golden/make_golden_bslabels.py), the written files through getfeatures.readPosFiles, the line routine compiled for the host
(dm_bslabels_format_host: the code the kernels of csrc/bslabels.hip.inc run) at every digit count, the refusals of HostEngine and of the command line,
and the routine under the address sanitizer (tests/bslabels_asan_driver.cpp)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import bslabels, bsperf, getfeatures

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HEADER = 'chrom\tstart\tend\tname\tscore\tstrand\tthickStart\tthickEnd\tcolor\tcoverage\tpercentage\n'
TABS = 'chr1\t1005\t1006\t.\t33\t+\t1005\t1006\t0,0,0\t33\t91\n'


def golden():
    return json.load(open(os.path.join(GOLDEN, 'bslabels_case.json')))


def host_classes(g):
    """{contig: (counts [2][5], cls [2][length])} of the golden case through bsperf.host_rows and bslabels.HostEngine, and the summed line counters."""
    o = g['options']
    names = o['chr']
    lengths = [len(g['reference'][c]) for c in names]
    eng = bslabels.HostEngine(names, lengths, len(g['replicates']), o['cov'], o['methylated'], o['unmethylated'])
    recs = [bsperf.host_rows(text.encode(), names, lengths) for text in g['replicates']]
    out = {}
    for c, name in enumerate(names):
        eng.open(c, g['reference'][name].encode(), o['motif'], o['ModinMotif'], o['Base'])
        for r, (pos, meta, _) in enumerate(recs):
            sel = bsperf.unpack_meta(meta)[0] == c
            eng.fill(r, pos[sel], meta[sel])
        counts = eng.classify()
        out[name] = (counts, eng.fetch_classes())
        eng.close_contig()
    return out, [lines for _, _, lines in recs]


def test_host_engine_equals_the_golden_case():
    g = golden()
    got, lines = host_classes(g)
    assert sorted(got) == sorted(g['contigs']) and len(got) == 3
    for name, (counts, cls) in got.items():
        want = g['contigs'][name]
        for s, strand in enumerate('+-'):
            assert dict(zip(bslabels.COUNT_KEYS, counts[s].tolist())) == want['counts'][strand], (name, strand)
        texts = bslabels.format_lists_host(name, cls)
        assert {k: v.decode() for k, v in texts.items()} == want['texts'], name
    assert all(g['contigs']['chrA']['counts'][s][k] > 0 for s in '+-' for k in bslabels.COUNT_KEYS)             # every class is in the case
    assert all(v == '' for v in g['contigs']['chrE']['texts'].values())                                       # a contig without truth: three empty lists
    for ln, want in zip(lines, g['lines']):
        assert dict(zip(bsperf.LINE_KEYS, ln.tolist())) == {k: want[k] for k in bsperf.LINE_KEYS} and int(ln.sum()) == want['seen']


def test_written_lists_round_trip_through_getfeatures(tmp_path):
    """What makes the files usable: getfeatures.readPosFiles on them returns exactly the golden key sets."""
    g = golden()
    got, _ = host_classes(g)
    for name, (_, cls) in got.items():
        for which, text in bslabels.format_lists_host(name, cls).items():
            with open(bslabels.list_path(str(tmp_path), 'case', which, name), 'wb') as fh:
                fh.write(text)
    for which in bslabels.LISTS:
        read = getfeatures.readPosFiles(str(tmp_path / ('case.%s.*.txt' % which)), g['reference'])
        want = {}
        for name, entry in g['contigs'].items():
            for strand, pos in entry['keys'][which]:
                want.setdefault(name, {'+': [], '-': []})[strand].append(pos)
        assert sorted(read) == sorted(want), which
        for name in want:
            for strand in '+-':
                assert read[name][strand].tolist() == sorted(want[name][strand]), (which, name, strand)


def test_host_line_routine_at_every_digit_count(hip_lib):
    """dm_bslabels_format_host against the Python statement at positions 0, 9, 10, 99, 100, ... 999999999, 1000000000, 2147483646 and at names of 1 and
    63 bytes; a buffer one byte short is not written to and the size comes back."""
    plus, minus = np.array([1, 2, 3, 4, 0, 1], np.uint8), np.array([3, 2, 1, 0, 4, 1], np.uint8)
    edges = sorted({10 ** d - 1 for d in range(1, 10)} | {10 ** d for d in range(0, 10)} | {0, 2147483646})
    assert {0, 9, 10, 99, 100, 999999999, 1000000000, 2147483646} <= set(edges)
    for name in ('c', 'k' * 63):
        for edge in edges:
            first = min(edge, bslabels.MAX_LENGTH - len(plus))
            for p, m in ((plus, minus), (plus, None), (None, minus), (plus[:1], minus[5:])):
                if len(p if p is not None else m) == 1:
                    first = edge
                cls = np.stack([p if p is not None else np.zeros_like(m), m if m is not None else np.zeros_like(p)])
                for which, want in zip(bslabels.LISTS.values(), bslabels.format_lists_host(name, cls, first).values()):
                    size, raw = bslabels.format_host_routine(name, which, p, m, first)
                    assert size == len(want) and raw == want, (name, first, which)
                    if size:
                        size1, raw1 = bslabels.format_host_routine(name, which, p, m, first, cap=size - 1)
                        assert size1 == size and raw1 == b'\xa5' * (size - 1), (name, first, which)
    assert bslabels.format_host_routine('c', 1, plus[:1], minus[5:], 2147483646)[1] == b'c + 2147483646\nc - 2147483646\n'
    lib = hip_lib
    for args, words in ((('k' * 64, 1, 0, 1), b'1 to 63'), (('c', 0, 0, 1), b'list 0'), (('c', 4, 0, 1), b'list 4'), (('c', 1, 2147483646, 2), b'2^31 - 2'), (('c', 1, -1, 1), b'positions')):
        name, which, first, n = args
        assert lib.dm_bslabels_format_host(name.encode(), which, plus.ctypes.data, minus.ctypes.data, first, n, None, 0) == -1 and words in lib.dm_last_error()


def test_host_engine_refusals():
    for kw, words in (({'replicates': 5}, '--truth.*1 to 4'), ({'cov': 0}, '--cov'), ({'cov': 65536}, '--cov'), ({'methylated': 10, 'unmethylated': 10}, '--unmethylated'),
                      ({'methylated': 101}, '--methylated')):
        with pytest.raises(bslabels.BsLabelsError, match=words):
            bslabels.HostEngine(['chr1'], [10], **kw)
    for names in ([], ['c%d' % i for i in range(65)], ['k' * 64], ['a b'], ['chr1', 'chr1']):
        with pytest.raises(bslabels.BsLabelsError, match='--chr'):
            bslabels.HostEngine(names, [10] * len(names))
    with pytest.raises(bslabels.BsLabelsError, match='--Ref'):
        bslabels.HostEngine(['chr1'], [None])
    eng = bslabels.HostEngine(['chr1'], [10], 2)
    for motif, k, words in (('CNG', 0, '--motif'), ('CG', 2, '--ModinMotif'), ('CG', -1, '--ModinMotif'), ('CG', 1, '--ModinMotif.*--Base'), ('C' * 9, 0, '--motif'), ('', 0, '--motif')):
        with pytest.raises(bslabels.BsLabelsError, match=words):
            eng.open(0, b'ACGCGTACGT', motif, k, 'C')
    with pytest.raises(bslabels.BsLabelsError, match='reference bytes'):
        eng.open(0, b'ACG', 'CG', 0, 'C')
    with pytest.raises(bslabels.BsLabelsError, match='no contig'):
        eng.classify()
    eng.open(0, b'ACGCGTACGT', 'CG', 0, 'C')
    meta = bsperf.pack_meta([0, 0], [0, 1], [5, 5], [90, 90])
    eng.fill(0, [3, 3], meta)                                                    # one position on both strands: two keys
    eng.fill(1, [3], meta[:1])
    with pytest.raises(bslabels.BsLabelsError, match='bslabels: replicate 1 holds position 3 of strand \\+ twice'):
        eng.fill(1, [3], meta[:1])
    with pytest.raises(bslabels.BsLabelsError, match='refused'):
        eng.classify()
    eng.open(0, b'ACGCGTACGT', 'CG', 0, 'C')
    eng.classify()
    with pytest.raises(bslabels.BsLabelsError, match='classified'):
        eng.classify()
    with pytest.raises(bslabels.BsLabelsError, match='classified'):
        eng.fill(0, [3], meta[:1])


def _bslabels(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'bslabels'] + args, capture_output=True, text=True, timeout=300)


def test_command_line_refusals(tmp_path):
    """One line each, naming the option, before a replicate is read or a GPU asked for."""
    out = tmp_path / 'out'
    fasta = tmp_path / 'genome.fa'
    fasta.write_text('>chr1 test\nACGCGT\n>chr2\nACGT\n')
    rep = tmp_path / 'rep1.bed'
    rep.write_text(HEADER + TABS)
    common = ['--truth', str(rep), '--Ref', str(fasta), '--outFolder', str(out)]
    for args, words in ((['--Ref', str(fasta)], ('--truth', 'are needed')),
                        (['--truth', str(rep)], ('--Ref', 'is needed')),
                        (['--truth', str(tmp_path / 'no.bed'), '--Ref', str(fasta)], ('--truth', 'does not exist')),
                        (['--truth', str(rep), '--Ref', str(tmp_path / 'no.fa')], ('--Ref', 'does not exist')),
                        (['--truth', ','.join([str(rep)] * 5), '--Ref', str(fasta)], ('--truth', '1 to 4')),
                        (common + ['--cov', '0'], ('--cov', '1 to 65535')),
                        (common + ['--cov', '65536'], ('--cov', '1 to 65535')),
                        (common + ['--methylated', '10', '--unmethylated', '10'], ('--unmethylated', 'unmethylated < methylated')),
                        (common + ['--methylated', '20', '--unmethylated', '30'], ('--unmethylated', 'unmethylated < methylated')),
                        (common + ['--motif', 'CNG'], ('--motif', 'A, C, G, T')),
                        (common + ['--motif', 'CG', '--ModinMotif', '2'], ('--ModinMotif', 'no position')),
                        (common + ['--motif', 'CG', '--ModinMotif', '1'], ('--ModinMotif', '--Base C')),
                        (common + ['--motif', 'GATC', '--ModinMotif', '1'], ('--ModinMotif', '--Base C')),
                        (common + ['--chr', 'chr1,chr9'], ('--chr', 'holds no contig chr9')),
                        (common + ['--chr', ','.join('c%d' % i for i in range(65))], ('--chr', '1 to 64')),
                        (common + ['--chr', 'k' * 64], ('--chr', '1 to 63 printable'))):
        res = _bslabels(args)
        last = res.stderr.strip().splitlines()[-1] if res.stderr.strip() else ''
        assert res.returncode != 0 and last.startswith('Error: bslabels: ') and all(w in last for w in words), (args, res.stderr[-2000:])
    assert not out.exists()
    fasta.write_text('>contig1\nACGT\n')                                          # none of the default contigs
    res = _bslabels(['--truth', str(rep), '--Ref', str(fasta), '--outFolder', str(out)])
    assert res.returncode != 0 and res.stderr.strip().splitlines()[-1].startswith('Error: bslabels: --chr: ') and not out.exists()


def test_line_routine_under_address_sanitizer(tmp_path):
    """tests/bslabels_asan_driver.cpp: csrc/bslabels.inc built as a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in
    statically - every class array and text in a heap block of exactly its size, positions of 1 to 10 digits, capacities one short."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'bslabels_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'bslabels_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'BSLABELS-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
