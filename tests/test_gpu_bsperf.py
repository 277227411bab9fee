"""GPU (-m gpu): `bsperf` on the device (csrc/bsperf.hip.inc) against its host twins: the parser against dm_bsperf_parse_host on a text whose lines
straddle the tile boundaries, whole and cut at every line end; duplicates and ranges; the counters against bsperf.HostEngine, exactly, at the wave and
block edges and at every edge of the semantics; and the command against tests/golden/bsperf_case.json (tests/golden/make_golden_bsperf.py: plain
dicts, sklearn, numpy.corrcoef) and, with --clusterCpG, against HostEngine fed with the file `merge --clusterCpG` writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_fused_case as cf
import long_cases
from conftest import ROOT
from deepmod_amd import _lib, bsperf, merge
from test_bsperf_host import BLANKS, HEADER, NAMES, TABS, VIOLATIONS, load_golden
from test_cluster import REAL
from test_gpu_merge import _split_runs

pytestmark = pytest.mark.gpu

LENGTHS = [3000, 2000, None]                                                     # of NAMES


def _truth_line(rng, i):
    name = ['chr1', 'chr10', 'chrX', 'chr', 'chr11'][int(rng.integers(0, 5))]
    pos = int(rng.integers(0, 2000))
    cov = int(rng.choice([0, 1, 4, 5, 9, 10, 65535, 65536, 2 ** 31 - 1]))
    strand = '+-.'[int(rng.integers(0, 3)) if i % 9 == 0 else int(rng.integers(0, 2))]
    f = [name, str(pos), str(pos + 1), '.', str(min(cov, 1000)), strand, str(pos), str(pos + 1), '0,0,0', str(cov), str(int(rng.integers(0, 101)))]
    kind = i % 5
    return ('\t'.join(f) + '\n' if kind == 0 else ' '.join(f) + ' \n' if kind == 1 else '  '.join(f) + '\n' if kind == 2 else ' \t' + ' \t '.join(f) + '\t\n' if kind == 3
            else 'chr1 1 2 . 1 +\n')


@pytest.fixture(scope="module")
def lines():
    """Lines for a little more than three tiles of text, no line starting on a tile boundary: every boundary lies inside a line."""
    tile = bsperf.tile_bytes()
    assert tile == 4096 == _lib.load().dm_xyload_tile_bytes()
    rng = np.random.default_rng(23)
    out, total = [HEADER], len(HEADER)
    while total < 3 * tile + 600:
        ln = _truth_line(rng, len(out))
        if (total + len(ln)) % tile == 0:
            ln = ln[:-1] + ' \n'
        out.append(ln)
        total += len(ln)
    starts = np.cumsum([0] + [len(ln) for ln in out])
    assert not (starts[1:] % tile == 0).any()
    return out, starts, tile


@pytest.fixture(scope="module")
def eng(gpu_device):
    e = bsperf.DeviceEngine(NAMES, (1, 5, 10), 2, lengths=LENGTHS, device=gpu_device)
    yield e
    e.close()


def _device_parse(eng, text, first):
    got, n, flag, bad = eng.add_truth_text(0, text.encode(), first)
    pos, meta = eng.records()
    assert len(pos) == n
    return pos, meta, got, flag, bad


def test_parser_equals_the_host_parser_whole_and_cut_at_every_line_end(eng, lines):
    out, starts, tile = lines
    whole = ''.join(out)
    for first in (True, False):
        for t in (whole, whole[:-1]):                                            # with and without the final newline
            t = t if first else t[len(HEADER):]
            (hpos, hmeta), hlines, hflag, hbad = bsperf.parse_device_grammar(t.encode(), NAMES, LENGTHS, first)
            assert (hflag, hbad) == (0, -1) and len(hpos) > 60 and (hlines[1:] > 0).sum() >= 4
            pos, meta, got, flag, bad = _device_parse(eng, t, first)
            assert (flag, bad) == (0, -1) and np.array_equal(pos, hpos) and np.array_equal(meta, hmeta) and np.array_equal(got, hlines)
    (hpos, hmeta), hlines, _, _ = bsperf.parse_device_grammar(whole.encode(), NAMES, LENGTHS, True)
    before = eng.fetch()['lines']
    for k in range(1, len(out)):                                                 # two chunks, cut behind line k
        a, b = ''.join(out[:k]), ''.join(out[k:])
        pa, ma, la, fa, _ = _device_parse(eng, a, True)
        pb, mb, lb, fb, _ = _device_parse(eng, b, False)
        assert fa == 0 and fb == 0
        assert np.array_equal(np.r_[pa, pb], hpos) and np.array_equal(np.r_[ma, mb], hmeta) and np.array_equal(la + lb, hlines), k
    assert np.array_equal(eng.fetch()['lines'] - before, hlines * (len(out) - 1))  # the handle sums the chunks it took
    assert len(out) > 150 and starts[-1] > 3 * tile


def test_first_line_is_skipped_only_in_the_first_chunk_of_a_file(eng):
    """HEADER has no digits in field 1: as a file's first line it is skipped unread, as a later chunk's first line it is outside the grammar."""
    pos, meta, got, flag, bad = _device_parse(eng, HEADER + TABS + BLANKS, True)
    assert (flag, bad) == (0, -1) and pos.tolist() == [1005, 7] and got.tolist() == [2, 1, 0, 0, 0, 0]
    pos, meta, got, flag, bad = _device_parse(eng, HEADER + TABS + BLANKS, False)
    assert (flag, bad) == (1, 1) and len(pos) == 0 and got.sum() == 0
    pos, meta, got, flag, bad = _device_parse(eng, TABS + BLANKS, False)
    assert (flag, bad) == (0, -1) and pos.tolist() == [1005, 7] and got.tolist() == [2, 0, 0, 0, 0, 0]
    assert eng.add_truth_text(0, b'', True)[1:] == (0, 0, -1)


@pytest.mark.parametrize("what", sorted(VIOLATIONS))
def test_a_violation_in_the_second_tile_is_flagged_and_adds_nothing(eng, lines, what):
    out, starts, tile = lines
    k = int(np.searchsorted(starts, tile)) + 3                                   # line k + 1 (1-based) starts in the second tile
    assert tile < starts[k] < 2 * tile
    before = eng.fetch()['lines']
    text = ''.join(out[:k]) + VIOLATIONS[what] + '\n' + ''.join(out[k:k + 100])
    got, n, flag, bad = eng.add_truth_text(1, text.encode(), True)
    assert (n, flag, bad) == (0, 1, k + 1) and got.sum() == 0
    assert bsperf.parse_device_grammar(text.encode(), NAMES, LENGTHS, True)[2:] == (1, k + 1)
    assert np.array_equal(eng.fetch()['lines'], before) and len(eng.records()[0]) == 0
    # the host statement takes the chunk: its records take the place of the parser's
    if what in ('carriage return', 'sign', '11 digits'):                         # what split() and int() read
        pos, meta, hl = bsperf.host_rows(text.encode(), NAMES, LENGTHS, True)
        eng.add_truth_records(1, pos, meta, hl)
        dpos, dmeta = eng.records()
        assert np.array_equal(dpos, pos) and np.array_equal(dmeta, meta) and np.array_equal(eng.fetch()['lines'] - before, hl)
    else:
        with pytest.raises(bsperf.BsPerfError, match=r'<text>:%d: ' % (k + 1)):
            bsperf.host_rows(text.encode(), NAMES, LENGTHS, True)


# ---- the tables and the count ----
def _tables(dm, name, length, cov, mod):
    """cov, mod int [2][length] -> the two summary tables of a DeviceMerge."""
    dm.open(name, length)
    strand, pos = np.nonzero(cov > 0)
    dm.add_records(pos, strand, cov[strand, pos], mod[strand, pos])


def _both(gpu_device, names, thresholds, R, methylated=90, unmethylated=0, pred_cov=1):
    return (bsperf.DeviceEngine(names, thresholds, R, methylated, unmethylated, pred_cov, device=gpu_device),
            bsperf.HostEngine(names, thresholds, R, methylated, unmethylated, pred_cov))


def _run_both(gpu_device, dm, length, cov, mod, recs, thresholds, methylated=90, unmethylated=0, pred_cov=1, scores=None):
    """recs: per replicate (pos, strand, coverage, percentage).  -> (device fetch, host fetch)."""
    dev, host = _both(gpu_device, ['chr1'], thresholds, len(recs), methylated, unmethylated, pred_cov)
    try:
        _tables(dm, 'chr1', length, cov, mod)
        dev.open(0, dm.plus, dm.minus)
        host.open(0, (cov[0], mod[0]), (cov[1], mod[1]))
        for r, (pos, strand, cv, pct) in enumerate(recs):
            meta = bsperf.pack_meta(np.zeros(len(pos), np.int64), strand, cv, pct)
            for e in (dev, host):
                e.fill(r, pos, meta)
        for e in (dev, host):
            e.count()
            if scores is not None:
                e.add_scores(*scores)
        return dev.fetch(), host.fetch()
    finally:
        dev.close()
        dm.close_contig()


def _assert_equal(got, want):
    for key in want:
        assert np.array_equal(got[key], want[key]), key


@pytest.fixture(scope="module")
def dm(gpu_device):
    d = merge.DeviceMerge(gpu_device)
    yield d
    d.close()


def _random_case(rng, length, R, thresholds, methylated, unmethylated, pred_cov, n_keys):
    cov, mod = np.zeros((2, length), np.int64), np.zeros((2, length), np.int64)
    keys = rng.choice(2 * length, min(n_keys, 2 * length), replace=False)
    s, p = keys // length, keys % length
    pk = rng.random(len(keys)) < 0.8                                              # predicted at all
    cov[s[pk], p[pk]] = rng.choice([pred_cov - 1, pred_cov, pred_cov + 1, 7, 100, 3000], int(pk.sum()))
    mod[s[pk], p[pk]] = (cov[s[pk], p[pk]] * rng.choice([0.0, 1.0, 0.5, 0.899, 0.9, 0.33], int(pk.sum()))).astype(np.int64)
    edges = sorted({1, 65535, 70000} | {c + d for c in thresholds for d in (-1, 0, 1) if c + d >= 1})
    pcts = sorted({0, 100, unmethylated, unmethylated + 1, methylated - 1, methylated, 50})
    recs = []
    for r in range(R):
        tk = rng.random(len(keys)) < 0.85                                         # a site is in most replicates
        n = int(tk.sum())
        recs.append((p[tk], s[tk], rng.choice(edges, n), np.where(rng.random(n) < 0.6, rng.choice([0, 100], n), rng.choice(pcts, n))))
    return cov, mod, recs


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("length", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_count_equals_the_host_engine_at_wave_and_block_edges(gpu_device, dm, length, R):
    rng = np.random.default_rng(length * 10 + R)
    thresholds, methylated, unmethylated, pred_cov = (2, 5, 10), 90, 5, 3
    cov, mod, recs = _random_case(rng, length, R, thresholds, methylated, unmethylated, pred_cov, 2 * length)
    n = max(length // 3, 1)
    keys = rng.choice(2 * length, min(n, 2 * length), replace=False)
    scores = (keys % length, keys // length, rng.integers(0, 101, len(keys)))
    got, want = _run_both(gpu_device, dm, length, cov, mod, recs, thresholds, methylated, unmethylated, pred_cov, scores)
    _assert_equal(got, want)
    if length >= 1023:
        assert (want['hist'].sum(axis=(1, 2, 3)) > 0).all() and (want['unpredicted'].sum(axis=(1, 2)) > 0).all() and (want['untruthed'] > 0).all()
        assert (want['below_threshold'] > 0).all() and (want['moments'][0, :, 0] > 0).all() and (want['moments'][1, :2, 0] > 0).all()


def test_every_percentage_at_every_threshold_and_label_edge(gpu_device, dm):
    thresholds, methylated, unmethylated, pred_cov = (1, 5, 10), 90, 3, 4
    rows = []                                                                    # (truth coverage of replicate 0, of 1, pct 0, pct 1, pred cov, pred mod)
    for x in range(101):
        for c in thresholds:
            for m in (c - 1, c):
                if m >= 1:
                    rows.append((m, m + 7, 100, 95, 100, x))                     # methylated; the smaller coverage decides the bucket
                    rows.append((m + 3, m, 0, 0, 100, x))                        # unmethylated
    for p0 in (methylated - 1, methylated, unmethylated, unmethylated + 1, 0, 100):
        for p1 in (methylated - 1, methylated, unmethylated, unmethylated + 1, 0, 100):
            for pc in (pred_cov - 1, pred_cov):                                  # the prediction-coverage edge
                rows.append((6, 6, p0, p1, pc, pc // 2))
    a = np.array(rows, np.int64)
    n = len(a)
    length = n + 5
    pos = np.arange(n) + 2
    cov, mod = np.zeros((2, length), np.int64), np.zeros((2, length), np.int64)
    strand = (pos % 2).astype(np.int64)
    cov[strand, pos], mod[strand, pos] = a[:, 4], a[:, 5]
    recs = [(pos, strand, a[:, 0], a[:, 2]), (pos[:-3], strand[:-3], a[:-3, 1], a[:-3, 3])]      # the last three sites are in one replicate only
    cov[0, 0], mod[0, 0] = 9, 9                                                  # a prediction without truth
    got, want = _run_both(gpu_device, dm, length, cov, mod, recs, thresholds, methylated, unmethylated, pred_cov)
    _assert_equal(got, want)
    h = want['hist'][0]
    assert (h[1].sum(axis=0) > 0).all() and (h[0].sum(axis=0) > 0).all() and h[2].sum() > 0      # every percentage, in both classes
    assert want['untruthed'][0] == 3 and want['unpredicted'][0].sum() == 35                     # position 0 and two of the three sites; pred_cov - 1 is no prediction
    # one replicate: the same sites, every one with truth
    got, want = _run_both(gpu_device, dm, length, cov, mod, recs[:1], thresholds, methylated, unmethylated, pred_cov)
    _assert_equal(got, want)
    assert want['untruthed'][0] == 1


def test_random_sites_and_one_contended_bin(gpu_device, dm):
    rng = np.random.default_rng(8)
    length = 130001
    cov, mod, recs = _random_case(rng, length, 2, (1, 5, 10), 90, 0, 1, 100000)
    keys = rng.choice(2 * length, 30000, replace=False)
    got, want = _run_both(gpu_device, dm, length, cov, mod, recs, (1, 5, 10), 90, 0, 1, (keys % length, keys // length, rng.integers(0, 101, len(keys))))
    _assert_equal(got, want)
    assert want['hist'][0].sum() > 40000
    # 2 x 10^5 sites that all fall in one bin
    length = 100000
    cov, mod = np.full((2, length), 8, np.int64), np.full((2, length), 4, np.int64)
    pos, strand = np.tile(np.arange(length), 2), np.repeat(np.arange(2), length)
    recs = [(pos, strand, np.full(2 * length, 7), np.full(2 * length, 100))] * 2
    got, want = _run_both(gpu_device, dm, length, cov, mod, recs, (1, 5, 10), 90, 0, 1, (pos, strand, np.full(2 * length, 77)))
    _assert_equal(got, want)
    assert want['hist'][0, 1, 1, 50] == 200000 == want['hist'][1, 1, 1, 77] and want['moments'][0, 1].tolist() == [200000, 10 ** 7, 4 * 10 ** 7, 2 * 10 ** 9, 5 * 10 ** 8, 8 * 10 ** 9]


def test_every_capped_grid_takes_a_second_pass(gpu_device, dm):
    """300,001 positions (long_cases.bsperf_case): bs_count_kernel<0/1> walks 2 x length elements in three passes of its grid, every replicate's one
    fill call and the one score call carry more records than bs_fill_kernel's and bs_score_kernel's grids have threads."""
    grid = 1024 * 256                                                 # bsk::MAX_BLOCKS x bsk::THREADS
    cov, mod, recs, scores = long_cases.bsperf_case()
    length = cov.shape[1]
    assert 2 * length > 2 * grid and all(len(r[0]) > grid for r in recs) and len(scores[0]) > grid
    assert len(np.unique(scores[1] * length + scores[0])) == len(scores[0])
    e = long_cases.bsperf_joined_elements()
    assert all(((e >= lo) & (e < hi)).any() for lo, hi in ((0, grid), (grid, 2 * grid), (2 * grid, 2 * length)))      # truth and a prediction in every pass
    thresholds, methylated, unmethylated, pred_cov = long_cases.BSPERF_RULE
    got, want = _run_both(gpu_device, dm, length, cov, mod, recs, thresholds, methylated, unmethylated, pred_cov, scores)
    _assert_equal(got, want)                                          # both kinds: tables and scores
    assert (want['hist'].sum(axis=(1, 2, 3)) > 100000).all() and (want['unpredicted'].sum(axis=(1, 2)) > 0).all() and (want['untruthed'] > 0).all()


def test_duplicates_and_range(gpu_device, dm):
    dev = bsperf.DeviceEngine(['chr1', 'chr2'], (1, 5), 2, device=gpu_device)
    try:
        cov = np.zeros((2, 5000), np.int64)
        cov[0, 7] = 3
        _tables(dm, 'chr1', 5000, cov, cov)
        before = dev.fetch()
        dev.open(0, dm.plus, dm.minus)
        pos = np.arange(0, 5000, 2)
        meta = bsperf.pack_meta(np.zeros(len(pos), np.int64), np.zeros(len(pos), np.int64), np.full(len(pos), 9), np.full(len(pos), 100))
        dev.fill(0, pos, meta)
        dev.fill(1, pos, meta)                                                   # the same keys in another replicate are no duplicates
        dev.fill(0, pos + 1, meta)                                               # other keys in a second call
        minus = bsperf.pack_meta([0], [1], [9], [100])
        dev.fill(0, [7], minus)                                                  # the other strand of a position is another key
        for bad_pos, bad_meta, words in (([5000], meta[:1], 'position 5000 of 5000'), ([-1], meta[:1], 'position -1'),
                                         ([5], bsperf.pack_meta([1], [0], [9], [100]), 'contig 1, the open one is 0'),
                                         ([5], bsperf.pack_meta([0], [0], [0], [100]), 'coverage 0'), ([5], bsperf.pack_meta([0], [0], [9], [101]), 'percentage 101')):
            with pytest.raises(_lib.DeepModHipError, match=words) as exc:        # refused before a launch
                dev.fill(1, bad_pos, bad_meta)
            assert exc.value.code == _lib.DM_EINVAL
        with pytest.raises(bsperf.BsPerfError, match=r'replicate 1 holds position 44 of strand \+ twice'):
            dev.fill(1, [4000, 44, 3001, 3001], meta[:4])                        # 44 is there already, 3001 twice in one call: the smallest is named
        with pytest.raises(_lib.DeepModHipError, match='refused'):
            dev.count()
        _assert_equal(dev.fetch(), before)                                       # nothing was counted
        dev.open(0, dm.plus, dm.minus)                                           # opened again, the contig starts clean
        dev.fill(1, [44], meta[:1])
        dev.fill(0, [44], meta[:1])
        with pytest.raises(_lib.DeepModHipError, match='after dm_bsperf_count'):
            dev.add_scores([1], [0], [5])
        dev.count()
        with pytest.raises(_lib.DeepModHipError, match='has been counted'):
            dev.count()
        for args, words in ((([5000], [0], [5]), 'position 5000'), (([5], [2], [5]), 'strand 2'), (([5], [0], [101]), 'percentage 101'),
                            (([5, 9, 5], [0, 0, 0], [5, 5, 5]), 'position 5 of strand \\+ occurs twice')):
            with pytest.raises(_lib.DeepModHipError, match=words):
                dev.add_scores(*args)
        got = dev.fetch()
        assert got['hist'].sum() == 0 and got['unpredicted'][0].sum() == 1 and got['untruthed'].tolist() == [1, 0]
    finally:
        dev.close()
        dm.close_contig()


def test_slot_indices_past_2_31(gpu_device, dm):
    """4 replicates of 2^28 + 5 positions: the last slots lie past element 2^31 of the truth table, and (strand, position) runs past 2^29.  The
    counters do not depend on where a site lies: HostEngine on the same sites moved to a contig of 100 positions is the expectation."""
    length, small = 2 ** 28 + 5, 100
    assert 4 * 2 * length > 2 ** 31
    off = length - small
    pos = np.array([0, 1, 50, 97, 98, 99, 99], np.int64)                         # in the small contig; the last five move to the end of the large one
    strand = np.array([0, 1, 0, 1, 0, 0, 1], np.int64)
    pcov, pmod = np.array([10, 4, 0, 7, 100, 3, 10]), np.array([9, 0, 0, 7, 50, 1, 9])
    recs = [(pos[r % 2:], strand[r % 2:], np.array([7, 12, 5, 1, 30, 9, 7])[r % 2:], np.array([100, 0, 95, 100, 40, 0, 100])[r % 2:]) for r in range(4)]
    scores = (pos[[0, 3, 6]], strand[[0, 3, 6]], np.array([0, 55, 100]))
    host = bsperf.HostEngine(['chr1'], (1, 5, 10), 4)
    cov, mod = np.zeros((2, small), np.int64), np.zeros((2, small), np.int64)
    cov[strand, pos], mod[strand, pos] = pcov, pmod
    host.open(0, (cov[0], mod[0]), (cov[1], mod[1]))
    for r, (p, s, cv, pct) in enumerate(recs):
        host.fill(r, p, bsperf.pack_meta(np.zeros(len(p), np.int64), s, cv, pct))
    host.count()
    host.add_scores(*scores)
    want = host.fetch()
    assert want['hist'][0].sum() == 5 and want['hist'][1].sum() == 2 and want['untruthed'].tolist() == [1, 1] and want['unpredicted'].sum(axis=(1, 2)).tolist() == [1, 4]
    move = lambda p: np.where(p >= 50, p + off, p)
    dev = bsperf.DeviceEngine(['chr1'], (1, 5, 10), 4, device=gpu_device)
    try:
        dm.open('chr1', length)
        dm.add_records(move(pos), strand, pcov, pmod)
        dev.open(0, dm.plus, dm.minus)
        for r, (p, s, cv, pct) in enumerate(recs):
            dev.fill(r, move(p), bsperf.pack_meta(np.zeros(len(p), np.int64), s, cv, pct))
        with pytest.raises(_lib.DeepModHipError, match='position %d of %d' % (length, length)):
            dev.fill(3, [length], bsperf.pack_meta([0], [1], [7], [100]))
        dev.count()
        dev.add_scores(move(scores[0]), scores[1], scores[2])
        _assert_equal(dev.fetch(), want)
    finally:
        dev.close()
        dm.close_contig()


# ---- the command ----
def _command(args, timeout=600):
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'bsperf'] + args, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    return res


def _write_golden(g, folder, crlf=False):
    for rel, text in g['pred'].items():
        p = folder / 'runs' / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text(text)
    truth = []
    for r, text in enumerate(g['truth']):
        p = folder / ('rep%d.bed' % (r + 1))
        if crlf and r == 1:                                                      # carriage returns in the second half of the second replicate
            half = text.index('\n', len(text) // 2) + 1
            text = text[:half] + text[half:].replace('\n', '\r\n')
        p.write_bytes(text.encode())
        truth.append(str(p))
    return truth


def _options(g, folder, truth):
    o = g['options']
    return {'predFolder': str(folder / 'runs'), 'truth': truth, 'Base': o['Base'], 'outFolder': str(folder / 'out'), 'FileID': 'case', 'chr': o['chr'],
            'cov': o['cov'], 'predCov': o['predCov'], 'methylated': o['methylated'], 'unmethylated': o['unmethylated'], 'Ref': None, 'clusterCpG': None, 'threads': 2}


def _comparable(doc):
    return {k: doc[k] for k in ('lines', 'lines_seen', 'counters', 'measures')}, [dict(v) for v in doc['truth'].values()]


def test_command_on_the_golden_case_writes_the_recorded_lines_twice(gpu_device, tmp_path):
    g = load_golden()
    o = g['options']
    truth = _write_golden(g, tmp_path)
    args = ['--predFolder', str(tmp_path / 'runs'), '--truth', ','.join(truth), '--Base', o['Base'], '--FileID', 'case', '--chr', ','.join(o['chr']),
            '--cov', ','.join(str(c) for c in o['cov']), '--predCov', str(o['predCov']), '--methylated', str(o['methylated']), '--unmethylated', str(o['unmethylated'])]
    files = []
    for out in ('out1', 'out2'):
        res = _command(args + ['--outFolder', str(tmp_path / out)])
        text = (tmp_path / out / 'case_bsperf.txt').read_text()
        assert text.splitlines() == g['report'] and all(ln in res.stdout for ln in g['report'])
        doc = json.load(open(tmp_path / out / 'case_bsperf.json'))
        doc.pop('kernel_ms')
        files.append((text, json.dumps(doc)))
    assert files[0] == files[1]                                                  # two runs: the same bytes, apart from the kernel ms
    doc = json.loads(files[0][1])
    raw = doc['counters']['raw']
    assert raw['hist'] == g['hist'] and raw['unpredicted'] == g['unpredicted'] and raw['below_threshold'] == g['below_threshold'] and raw['untruthed'] == g['untruthed']
    assert doc['notes'] == [] and list(doc['counters']) == ['raw']
    for path, want in zip(truth, g['line_counts']):
        assert doc['truth'][path]['lines_seen'] == want['seen'] and all(doc['truth'][path][k] == want[k] for k in bsperf.LINE_KEYS)
    for t, want in g['measures'].items():
        for key in ('auc', 'ap', 'r', 'rmse'):
            assert abs(doc['measures']['raw'][t][key] - want[key]) <= 1e-12 * abs(want[key])
    assert doc['contigs']['chrA']['lines_read'] == sum(text.count('\n') for rel, text in g['pred'].items() if '.chrA' in rel)


def test_command_takes_the_host_path_for_a_chunk_outside_the_grammar_and_writes_the_same(gpu_device, tmp_path):
    g = load_golden()
    docs = []
    for name, crlf in (('plain', False), ('crlf', True)):
        folder = tmp_path / name
        folder.mkdir()
        truth = _write_golden(g, folder, crlf)
        docs.append(bsperf.bsperf(_options(g, folder, truth), gpu_device, chunk_bytes=1000))      # a dozen chunks per replicate
        docs[-1]['text'] = (folder / 'out' / 'case_bsperf.txt').read_bytes()
    plain, crlf = docs
    assert plain['notes'] == [] and len(crlf['notes']) >= 3 and all('rep2.bed: line ' in n and 'parsed on the host' in n for n in crlf['notes'])
    half = g['truth'][1].index('\n', len(g['truth'][1]) // 2) + 1
    assert ' line %d is outside' % (g['truth'][1][:half].count('\n') + 1) in crlf['notes'][0]
    assert _comparable(plain) == _comparable(crlf) and plain['text'] == crlf['text'] and plain['report'] == g['report']
    # a chunk the host statement refuses too stops the command with file and line
    folder = tmp_path / 'bad'
    folder.mkdir()
    truth = _write_golden(g, folder)
    text = g['truth'][0]
    cut = text.index('\n', len(text) // 3) + 1
    open(truth[0], 'w').write(text[:cut] + 'chrA 5 6 . 7 + 5 6 0,0,0 7 101\n' + text[cut:])
    with pytest.raises(bsperf.BsPerfError, match=r'rep1\.bed:%d: .*percentage 101' % (text[:cut].count('\n') + 1)):
        bsperf.bsperf(_options(g, folder, truth), gpu_device, chunk_bytes=1000)
    # and a key that occurs twice in a replicate, naming the file and the position
    dup = [ln for ln in text.split('\n')[1:] if ln.startswith('chrB') and len(ln) > 20 and ln.split('\t')[9] != '0' and ln.split('\t')[5] in '+-'][5]
    open(truth[0], 'w').write(text + dup + '\n')
    with pytest.raises(bsperf.BsPerfError, match=r'rep1\.bed: chrB: replicate 0 holds position %s of strand \%s twice' % (dup.split('\t')[1], dup.split('\t')[5])):
        bsperf.bsperf(_options(g, folder, truth), gpu_device)
    assert not (folder / 'out').exists()


def test_cluster_stage_equals_the_host_engine_fed_with_the_file_merge_writes(gpu_device, tmp_path):
    n = 70001
    ch = cf.chain(n)
    seq, cov_p, mod_p, cov_m, mod_m = ch['case']
    runs = tmp_path / 'runs'
    _split_runs(str(runs), n)
    rng = np.random.default_rng(3)
    up = np.frombuffer(seq.upper().encode(), np.uint8)
    plus_c = np.flatnonzero((up[:-1] == ord('C')) & (up[1:] == ord('G')))
    reps, cpg = [], set(plus_c.tolist())
    for r in range(2):                                                           # bisulfite truth on most CpGs of both strands, and on a few other positions
        rows = [HEADER]
        for strand, sites in (('+', plus_c), ('-', plus_c + 1)):
            for p in sites[rng.random(len(sites)) < 0.9]:
                rows.append('\t'.join([cf.CHROM, str(p), str(p + 1), '.', '9', strand, str(p), str(p + 1), '0,0,0', str(int(rng.choice([1, 4, 5, 12, 30]))),
                                       str(int(rng.choice([0, 0, 100, 95, 90, 89, 40])))]) + '\n')
        rows += ['\t'.join([cf.CHROM, str(p), str(p + 1), '.', '9', '+', str(p), str(p + 1), '0,0,0', '8', '100']) + '\n' for p in range(3, n, 997)
                 if p not in cpg]
        path = tmp_path / ('rep%d.bed' % (r + 1))
        path.write_text(''.join(rows))
        reps.append(str(path))
    subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'merge', '--predFolder', str(runs), '--Base', 'C', '--FileID', 'run', '--chr', cf.CHROM,
                    '--Ref', ch['fasta'], '--clusterCpG', REAL], capture_output=True, text=True, timeout=600, check=True)
    res = _command(['--predFolder', str(runs), '--truth', ','.join(reps), '--Base', 'C', '--FileID', 'run', '--chr', cf.CHROM, '--Ref', ch['fasta'], '--clusterCpG', REAL,
                    '--outFolder', str(tmp_path / 'out'), '--cov', '1,5,10'])
    doc = json.load(open(tmp_path / 'out' / 'run_bsperf.json'))
    fields = [ln.split() for ln in open(runs / ('run_clusterCpG.%s.C.bed' % cf.CHROM))]
    assert len(fields) == len(ch['lines']) > 1000 and all(len(f) == 13 for f in fields)
    host = bsperf.HostEngine([cf.CHROM], (1, 5, 10), 2, lengths=[n])
    host.open(0, (cov_p, mod_p), (cov_m, mod_m))
    for r, path in enumerate(reps):
        pos, meta, lines = bsperf.host_rows(open(path, 'rb').read(), [cf.CHROM], [n])
        host.add_lines(lines)
        host.fill(r, pos, meta)
    host.count()
    host.add_scores([int(f[1]) for f in fields], [int(f[5] == '-') for f in fields], [int(f[12]) for f in fields])
    want = host.fetch()
    for k, kind in enumerate(bsperf.KINDS):
        c = doc['counters'][kind]
        assert c['hist'] == want['hist'][k].tolist() and c['unpredicted'] == want['unpredicted'][k].tolist() and c['moments'] == want['moments'][k].tolist()
        assert c['untruthed'] == int(want['untruthed'][k]) and c['below_threshold'] == int(want['below_threshold'][k])
        assert want['hist'][k].sum() > 1000 and want['unpredicted'][k].sum() > 0 and want['untruthed'][k] > 0
    assert doc['contigs'][cf.CHROM]['sites'] == len(fields) and doc['lines'] == dict(zip(bsperf.LINE_KEYS, want['lines'].tolist()))
    report = bsperf.report_lines(bsperf.measures(want, (1, 5, 10), 2, (0, 1)))
    assert (tmp_path / 'out' / 'run_bsperf.txt').read_text().splitlines() == report and len(report) == 6
    assert [ln.split()[0] for ln in report] == ['raw'] * 3 + ['clustered'] * 3 and all(ln in res.stdout for ln in report)
