"""GPU (-m gpu): `merge` on the device (csrc/bedmerge.hip.inc) against its host twins: the parser against merge.readbed2 and the host routine on
texts whose lines straddle the tile boundaries, the adds against numpy sums, the formatter against merge.save_mod for one buffer and for the smallest
buffer, the overflow guard, and the command against the reference tool's recorded bytes (tests/golden/merge_case.json) and against the chain of the
three tools on files (tests/cluster_fused_case.py), with the real and a synthetic cluster checkpoint."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_fused_case as cf
from conftest import GOLDEN, ROOT
from deepmod_amd import _lib, cluster, merge, summary, tfbundle
from test_cluster import REAL, _synthetic_cluster_weights
from test_merge_host import VIOLATIONS

pytestmark = pytest.mark.gpu

CONTIG_LEN = 2000


def _line(rng, i, contig='chr1', length=CONTIG_LEN):
    """A line in one of the three dialects or with mixed separators, 40 - 90 bytes."""
    cov = int(rng.integers(0, 3000))
    mod = int(rng.integers(0, cov + 1))
    pos = int(rng.integers(0, length))
    head = '%s %d %d C %d %s' % (contig, pos, pos + 1, min(cov, 1000), '+-'[int(rng.integers(0, 2))])
    tail = '%d %d 0,0,0 %d %d %d' % (pos, pos + 1, cov, mod * 100 // max(cov, 1), mod)
    kind = i % 4
    return (head + ' ' + tail + ' \n' if kind == 0 else head + '  ' + tail + '\n' if kind == 1 else head + '  ' + tail + ' %d\n' % (i % 101) if kind == 2
            else '\t' + (head + ' ' + tail).replace(' ', '\t', 3) + ' \t\n')


@pytest.fixture(scope="module")
def lines():
    """Lines for four tiles of text, no line starting on a tile boundary: every boundary lies inside a line."""
    tile = _lib.load().dm_xyload_tile_bytes()
    assert tile == 4096
    rng = np.random.default_rng(17)
    out, total = [], 0
    while total < 4 * tile + 40000:
        ln = _line(rng, len(out))
        if (total + len(ln)) % tile == 0:
            ln = ln[:-1] + ' \n'
        out.append(ln)
        total += len(ln)
    starts = np.cumsum([0] + [len(ln) for ln in out])
    assert not (starts[1:] % tile == 0).any()
    return out, starts, tile


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = merge.DeviceMerge(gpu_device)
    yield d
    d.close()


def _readbed2(tmp_path, text):
    p = tmp_path / 'x.bed'
    p.write_text(text)
    return merge.readbed2(str(p))


def _sums(length, recs):
    """numpy twin of the adds: recs [(pos, strand, cov, mod)] -> touch, cov, mod int64 [2][length]."""
    touch, cov, mod = (np.zeros((2, length), np.int64) for _ in range(3))
    for pos, strand, cv, md in recs:
        np.add.at(touch, (strand, pos), 1)
        np.add.at(cov, (strand, pos), cv)
        np.add.at(mod, (strand, pos), md)
    return touch, cov, mod


def _counters(d):
    return [np.stack(a) for a in zip(d.plus.fetch(), d.minus.fetch())]       # touch, cov, mod as [2][length]


def test_parser_on_lines_that_straddle_the_tile_boundaries(dev, lines, tmp_path):
    out, starts, tile = lines
    one_tile = int(np.searchsorted(starts, tile))                                # lines 0 .. one_tile - 1 reach into the second tile
    three = int(np.searchsorted(starts, 3 * tile))
    for n in (1, one_tile - 1, one_tile, one_tile + 1, three + 300):
        text = ''.join(out[:n])
        assert {1: len(text) < 100, one_tile - 1: len(text) < tile, one_tile: tile < len(text) < tile + 120, one_tile + 1: tile < len(text) < tile + 240}.get(n, len(text) > 3 * tile)
        for t in (text, text[:-1]):                                              # with and without the final newline
            dev.open('chr1', CONTIG_LEN)
            rows, flag, bad = dev.add_text(t.encode())
            assert (rows, flag, bad) == (n, 0, -1)
            got = dev.records()
            host, hflag, hbad = merge.parse_device_grammar(t.encode(), 'chr1', CONTIG_LEN)
            assert (hflag, hbad) == (0, -1) and all(np.array_equal(a, b) for a, b in zip(got, host))
            chrom, rpos, rstrand, rcov, rmod = _readbed2(tmp_path, t)
            assert np.array_equal(got[0], rpos) and np.array_equal(got[1], (rstrand == '-').astype(np.uint8)) and np.array_equal(got[2], rcov) and np.array_equal(got[3], rmod)
            touch, cov, mod = _sums(CONTIG_LEN, [(got[0], got[1], got[2], got[3])])
            ct, cc, cm = _counters(dev)
            assert np.array_equal(ct, touch) and np.array_equal(cc, cov) and np.array_equal(cm, mod) and touch.sum() == n
    assert three + 300 < len(out)


@pytest.mark.parametrize("what", sorted(VIOLATIONS))
def test_a_violation_in_the_second_tile_is_flagged_and_adds_nothing(dev, lines, what):
    out, starts, tile = lines
    k = int(np.searchsorted(starts, tile)) + 3                                   # line k + 1 (1-based) starts in the second tile
    assert tile < starts[k] < 2 * tile
    dev.open('chr1', CONTIG_LEN)
    first = ''.join(out[:5]).encode()
    dev.add_text(first)
    before = _counters(dev)
    text = ''.join(out[:k]) + VIOLATIONS[what] + '\n' + ''.join(out[k:k + 150])
    rows, flag, bad = dev.add_text(text.encode())
    assert (rows, flag, bad) == (k + 151, 1, k + 1)
    assert merge.parse_device_grammar(text.encode(), 'chr1', CONTIG_LEN)[1:] == (1, k + 1)
    assert all(np.array_equal(a, b) for a, b in zip(before, _counters(dev))) and before[0].sum() == 5
    assert len(dev.records()[0]) == 0


def _text_of(contig, pos, strand, cov, mod):
    """The records as a file in the detect dialect."""
    return ''.join('%s %d %d C %d %s %d %d 0,0,0 %d %d %d \n' % (contig, p, p + 1, min(c, 1000), '+-'[s], p, p + 1, c, 100 * m // max(c, 1), m)
                   for p, s, c, m in zip(pos.tolist(), strand.tolist(), cov.tolist(), mod.tolist())).encode()


def _merged_rows(contig, cov, mod):
    """The sums [2][length] -> the tuple merge.save_mod takes, sorted by (position, strand)."""
    pos, strand = np.nonzero(mod.T > 0)                                          # position-major: '+' before '-' at one position
    return (np.array([contig] * len(pos), object), pos.astype(np.int64), np.array(['+-'[s] for s in strand], object), cov[strand, pos], mod[strand, pos])


def _save_mod(tmp_path, contig, base, cov, mod):
    p = str(tmp_path / 'want.bed')
    merge.save_mod(p, _merged_rows(contig, cov, mod), base)
    return open(p, 'rb').read()


def _all_runs(d, base, cap):
    lines, nbytes, largest = d.format_begin(base)
    buf, parts, more = np.empty(max(cap(largest), 1), np.uint8), [], nbytes > 0
    while more:
        more, part = d.format_next(buf)
        assert 0 < len(part) <= len(buf)
        parts.append(part.tobytes())
    return b''.join(parts), len(parts), lines, nbytes, largest


TILE_POS = 1024


@pytest.mark.parametrize("length", [1, 2, TILE_POS - 1, TILE_POS, TILE_POS + 1, 3 * TILE_POS + 7, 1000003])
def test_adds_equal_numpy_sums_and_the_text_equals_save_mod(dev, tmp_path, length):
    assert merge.tile_positions() == TILE_POS
    rng = np.random.default_rng(length)
    contig, base = ('chr1', 'C') if length % 2 else ('k' * 255, 'A')
    dev.open(contig, length)
    empty, runs, lines, nbytes, largest = _all_runs(dev, base, lambda m: m)
    assert (empty, runs, lines, nbytes, largest) == (b'', 0, 0, 0, 0) and list(dev.format(base)) == []       # an empty table gives 0 bytes
    recs = []
    n_files = [int(rng.integers(1, 6)), int(rng.integers(1, 6))]
    for f in range(max(n_files)):
        n = min(4 * length, 20000)
        pos = rng.integers(0, length, n)
        strand = rng.integers(0, 2, n)
        cov = rng.integers(0, 3000, n)
        mod = np.where(rng.random(n) < 0.3, 0, (cov * rng.random(n) ** 2).astype(np.int64))
        keep = np.array(n_files)[strand] > f                                     # 1 - 5 files per strand
        pos, strand, cov, mod = pos[keep], strand[keep], cov[keep], mod[keep]
        if f == 0:                                                                # the edges and the value cases, both strands on one position
            steps = [p for k in range(1, 7) for p in (10 ** k - 2, 10 ** k - 1, 10 ** k) if p < length]
            fixed = [(p, s, 5 + s, 1 + s) for p in [0, length - 1] + steps for s in (0, 1)]
            fixed += [(length // 2, 0, 999, 999), (length // 2, 1, 1000, 1), (length // 3, 0, 1001, 1001), (length // 3, 1, 2 ** 30, 2 ** 30 - 1)]
            fixed += [(int(p), int(p) % 2, 100, m) for m, p in enumerate(rng.integers(0, length, 101))]              # every pct 0 .. 100
            fixed += [(length - 1, 0, 7, 0), (0, 1, 7, 7), (0, 1, 7, 7)]          # mod == 0; two records of one file on one key both count
            pos, strand, cov, mod = (np.r_[a, [r[j] for r in fixed]] for j, a in enumerate((pos, strand, cov, mod)))
        recs.append((pos, strand, cov, mod))
        if f % 2 == 0:
            rows, flag, bad = dev.add_text(_text_of(contig, pos, strand, cov, mod))
            assert (rows, flag, bad) == (len(pos), 0, -1)
        else:
            dev.add_records(pos, strand, cov, mod)
    touch, cov, mod = _sums(length, recs)
    ct, cc, cm = _counters(dev)
    assert np.array_equal(ct, touch) and np.array_equal(cc, cov) and np.array_equal(cm, mod) and cov.max() >= 2 ** 30
    want = _save_mod(tmp_path, contig, base, cov, mod)
    whole, runs, lines, nbytes, largest = _all_runs(dev, base, lambda m: 64 << 20)
    assert whole == want and runs == 1 and lines == want.count(b'\n') and nbytes == len(want) and 0 < largest <= nbytes
    assert b''.join(p.tobytes() for p in dev.format(base)) == want
    small, runs, _, _, _ = _all_runs(dev, base, lambda m: m)                     # the smallest allowed buffer: many runs, concatenated
    assert small == want and runs >= min((length + TILE_POS - 1) // TILE_POS, 2)
    if length > 3 * TILE_POS:
        assert runs >= 3
    dev.format_begin(base)
    buf = np.empty(largest, np.uint8)
    with pytest.raises(_lib.DeepModHipError, match='%d bytes are needed' % largest) as exc:
        for _ in range((length + TILE_POS - 1) // TILE_POS):                    # one byte below the largest tile: refused when that tile is next
            dev.format_next(buf, largest - 1)
    assert exc.value.code == _lib.DM_EINVAL
    assert merge.format_host(contig, base, cov[0], mod[0], cov[1], mod[1]) == want


def test_one_add_of_more_records_than_the_grid_has_threads(dev, tmp_path):
    """300,000 records in one add: bm_add_kernel's grid is capped, every thread takes a second record and some none (the adds above carry 20,000 records
    a call at most).  Three tiles and seven positions take them, so the second pass adds to sums the first pass made."""
    grid = 1024 * 256                                                 # bmk::MAX_BLOCKS x bmk::THREADS
    length, n = 3 * TILE_POS + 7, 300000
    assert grid < n < 2 * grid
    rng = np.random.default_rng(9)
    pos, strand, cov = rng.integers(0, length, n), rng.integers(0, 2, n), rng.integers(0, 30, n)
    mod = (cov * rng.random(n)).astype(np.int64)
    pos[[0, grid - 1, grid, n - 1]] = [0, length - 1, 0, length - 1]               # the ends of both passes on the ends of the tables
    dev.open('chr1', length)
    dev.add_records(pos, strand, cov, mod)
    touch, cov, mod = _sums(length, [(pos, strand, cov, mod)])
    ct, cc, cm = _counters(dev)
    assert np.array_equal(ct, touch) and np.array_equal(cc, cov) and np.array_equal(cm, mod) and touch.sum() == n and touch.min() > 0
    assert b''.join(p.tobytes() for p in dev.format('C')) == _save_mod(tmp_path, 'chr1', 'C', cov, mod)


def test_single_file_with_the_largest_coverage_and_growing_tables(dev, tmp_path):
    """coverage 2^31 - 1 fits one file alone; without a length the tables grow to the largest position + 1 of each file, sums kept."""
    dev.open('chr1')
    assert dev.plus.length == 1
    pos, strand = np.array([0, 0, 3, 5000, 5000]), np.array([0, 1, 1, 0, 1])
    cov, mod = np.array([2 ** 31 - 1, 1001, 1000, 2 ** 31 - 1, 999]), np.array([2 ** 31 - 1, 1001, 0, 1, 999])
    dev.add_records(pos, strand, cov, mod)
    assert dev.plus.length == dev.minus.length == 5001
    touch, cov_s, mod_s = _sums(5001, [(pos, strand, cov, mod)])
    assert all(np.array_equal(a, b) for a, b in zip(_counters(dev), (touch, cov_s, mod_s)))
    assert b''.join(p.tobytes() for p in dev.format('C')) == _save_mod(tmp_path, 'chr1', 'C', cov_s, mod_s)
    with pytest.raises(_lib.DeepModHipError, match='2\\^31 or more'):
        dev.add_records([7], [0], [1], [1])
    dev.open('chr1')
    dev.add_text(b'chr1 9 10 C 5 + 9 10 0,0,0 5 20 1 \n')
    assert dev.plus.length == 10
    dev.add_text(b'chr1 4099 4100 C 5 - 4099 4100 0,0,0 5 20 1 \nchr1 9 10 C 5 + 9 10 0,0,0 5 40 2 \n')
    assert dev.plus.length == dev.minus.length == 4100
    assert b''.join(p.tobytes() for p in dev.format('C')) == b'chr1 9 10 C 10 +  9 10 0,0,0 10 30 3\nchr1 4099 4100 C 5 -  4099 4100 0,0,0 5 20 1\n'
    rows, flag, bad = dev.add_text(b'chr1 2147483647 4100 C 5 - 4099 4100 0,0,0 5 20 1 \n')               # position + 1 is no int32
    assert (flag, bad) == (1, 1) and dev.plus.length == 4100


def test_overflow_guard_refuses_the_second_file_and_keeps_the_first(dev):
    dev.open('chr1', 100)
    one = b'chr1 7 8 C 1000 + 7 8 0,0,0 1073741824 50 536870912 \n'
    assert dev.add_text(one) == (1, 0, -1)
    before = _counters(dev)
    assert before[1][0, 7] == 2 ** 30 and before[2][0, 7] == 2 ** 29 and before[0].sum() == 1
    with pytest.raises(_lib.DeepModHipError, match=r"the largest coverages of this contig's files sum to 2147483648 \(2\^31 or more\): the int32 tables cannot hold them") as exc:
        dev.add_text(one.replace(b' 7 8 ', b' 9 10 '))
    assert exc.value.code == _lib.DM_EINVAL
    with pytest.raises(_lib.DeepModHipError, match='2\\^31 or more'):
        dev.add_records([9], [1], [2 ** 30], [0])
    assert all(np.array_equal(a, b) for a, b in zip(before, _counters(dev)))
    dev.add_records([9], [1], [2 ** 30 - 1], [5])                               # one below: taken
    assert _counters(dev)[1][1, 9] == 2 ** 30 - 1


# ---- the command ----
def _merge(folder, more, timeout=600):
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'merge', '--predFolder', str(folder), '--threads', '3'] + more,
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    return res


@pytest.mark.parametrize("variant", ["as recorded", "detect dialect", "carriage returns in one file"])
def test_command_writes_the_reference_tools_bytes(gpu_device, tmp_path, variant):
    g = json.load(open(os.path.join(GOLDEN, 'merge_case.json')))
    crlf = 'runB/sub/mod_pos.chr1-.C.bed'
    for rel, text in g['inputs'].items():
        if variant == "detect dialect":
            text = text.replace('\n', ' \n')
        elif variant.startswith("carriage") and rel == crlf:
            text = text.replace('\n', '\r\n')
        p = tmp_path / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(text.encode())
    base, fileid, chrs = g['argv']
    res = _merge(tmp_path, ['--Base', base, '--FileID', fileid, '--chr', chrs])
    for fn, text in g['outputs'].items():
        assert (tmp_path / fn).read_bytes() == text.encode(), fn
    assert (tmp_path / 'merged.chr7.C.bed').read_bytes() == b''                  # a contig without files: an empty file
    doc = json.load(open(tmp_path / 'merged_merge.json'))
    notes = [n for c in doc['contigs'].values() for n in c['notes']]
    if variant.startswith("carriage"):
        assert len(notes) == 1 and crlf in notes[0] and 'line 1 ' in notes[0]
    else:
        assert notes == []
    c1 = doc['contigs']['chr1']
    assert len(c1['files']) == 5 and c1['lines_read'] == sum(g['inputs'][f].count('\n') for f in g['inputs'] if '.chr1' in f)
    assert c1['lines_written'] == g['outputs']['merged.chr1.C.bed'].count('\n') and set(c1['kernel_ms']) == {'parse', 'add', 'format'}
    assert doc['contigs']['chr7']['files'] == [] and len([ln for ln in res.stdout.splitlines() if ' -+ C: ' in ln]) == 3
    assert glob.glob(str(tmp_path / '*clusterCpG*')) == []


def test_command_stops_at_a_line_of_another_contig(gpu_device, tmp_path):
    (tmp_path / 'runA').mkdir()
    (tmp_path / 'runA' / 'mod_pos.chr1+.C.bed').write_text('chr1 5 6 C 7 + 5 6 0,0,0 7 42 3 \nchr2 5 6 C 7 + 5 6 0,0,0 7 42 3 \n')
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'merge', '--predFolder', str(tmp_path), '--chr', 'chr1'], capture_output=True, text=True,
                         timeout=600)
    last = res.stderr.strip().splitlines()[-1]
    assert res.returncode != 0 and last.startswith('Error: ') and 'mod_pos.chr1+.C.bed:2: a line of chr2 in a file named for chr1' in last


@pytest.fixture(scope="module")
def synthetic_checkpoint(tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp('merge_cluster_model') / 'synthetic')
    tfbundle.write_bundle(prefix, _synthetic_cluster_weights())
    return prefix


def _split_runs(folder, n):
    """The chain's counters of every position split at random over three runs (mod_i <= cov_i), written as detect writes them (with rows that were
    touched only) into runA/, runB/sub/ and runC/x/y/."""
    seq, cov_p, mod_p, cov_m, mod_m = cf.chain(n)['case']
    rng = np.random.default_rng(n)
    for strand, cov, mod in (('+', cov_p, mod_p), ('-', cov_m, mod_m)):
        cov, mod = cov.astype(np.int64), mod.astype(np.int64)
        c1 = rng.integers(0, cov + 1)
        c2 = rng.integers(0, cov - c1 + 1)
        c3 = cov - c1 - c2
        m1 = rng.integers(np.maximum(0, mod - c2 - c3), np.minimum(c1, mod) + 1)
        m2 = rng.integers(np.maximum(0, mod - m1 - c3), np.minimum(c2, mod - m1) + 1)
        m3 = mod - m1 - m2
        assert (m3 >= 0).all() and (m3 <= c3).all() and (m1 <= c1).all() and (m2 <= c2).all()
        for sub, c, m in (('runA', c1, m1), ('runB/sub', c2, m2), ('runC/x/y', c3, m3)):
            text = summary.bed_lines_py(cf.CHROM, strand, 'C', cf.touch_of(c, m), c, m)
            os.makedirs(os.path.join(folder, sub), exist_ok=True)
            if text:
                with open(os.path.join(folder, sub, 'mod_pos.%s%s.C.bed' % (cf.CHROM, strand)), 'wb') as fh:
                    fh.write(text)


@pytest.mark.parametrize("model", ["real", "synthetic"])
@pytest.mark.parametrize("n", [1, 2, 26, 257, 70001])
def test_command_with_the_cluster_stage_equals_the_three_tools(gpu_device, tmp_path, synthetic_checkpoint, n, model):
    ch = cf.chain(n)
    if n == 70001:
        cf.assert_run_is_no_empty_comparison(ch)
    prefix = REAL if model == 'real' else synthetic_checkpoint
    _split_runs(str(tmp_path), n)
    _merge(tmp_path, ['--Base', 'C', '--FileID', 'run', '--chr', cf.CHROM, '--Ref', ch['fasta'], '--clusterCpG', prefix])
    assert (tmp_path / ('run.%s.C.bed' % cf.CHROM)).read_bytes() == ch['pred_text'].encode()
    written = cluster.hm_cluster_predict(os.path.join(ch['folder'], 'run'), os.path.join(ch['folder'], 'motif'), prefix, chrkeys=[cf.CHROM], device=gpu_device)
    mine = tmp_path / ('run_clusterCpG.%s.C.bed' % cf.CHROM)
    doc = json.load(open(tmp_path / 'run_merge.json'))['contigs'][cf.CHROM]
    assert doc['notes'] == [] and doc['sites'] == len(ch['lines'])
    if len(ch['lines']) == 0:
        assert written == [] and not mine.exists()                                # the chain writes no file: neither does the command
    else:
        assert mine.read_bytes() == open(written[0], 'rb').read()
        os.remove(written[0])


def test_two_runs_of_the_command_write_identical_files(gpu_device, tmp_path):
    ch = cf.chain(70001)
    _split_runs(str(tmp_path), 70001)
    got = []
    for _ in range(2):
        _merge(tmp_path, ['--Base', 'C', '--FileID', 'run', '--chr', cf.CHROM, '--Ref', ch['fasta'], '--clusterCpG', REAL])
        got.append([(tmp_path / f).read_bytes() for f in ('run.%s.C.bed' % cf.CHROM, 'run_clusterCpG.%s.C.bed' % cf.CHROM)])
    assert got[0] == got[1] and all(len(b) > 10000 for b in got[0])
