"""GPU (-m gpu): the tiled text writer merge and bslabels share (csrc/textout.hip.inc), on what sharing adds: the state one handle carries from a
format to the next.  One merge.DeviceMerge and one bslabels.DeviceEngine format contigs of 3 TILE + 7, then 1, then TILE + 1 positions - a longer
offset table, a shorter one, a longer one again - each in runs of exactly the largest tile's bytes and in one run, against merge.format_host and
bslabels.format_list_host byte for byte; a format cut off by an add is over; the format time grows with a text and not without one.  The texts at the
tile edges themselves are held by test_gpu_merge.py and test_gpu_bslabels.py.  The first test needs no GPU: the fills below give at least two runs
at the smallest buffer by the host formatters' own count."""
from collections import namedtuple

import numpy as np
import pytest

from deepmod_amd import _lib, bslabels, bsperf, merge
from test_gpu_bslabels import COV, HI, LO, make_contig, whole_text

TILE = 1024
LENGTHS = (3 * TILE + 7, 1, TILE + 1)
NAMES = ['r%d' % n for n in LENGTHS]
MOTIF, K, R, BASE = 'C', 0, 2, 'C'

MergeCase = namedtuple('MergeCase', 'records cov mod text tile_bytes')
ListsCase = namedtuple('ListsCase', 'seq recs cls text tile_bytes')


def _tiles(length):
    return [(a, min(a + TILE, length)) for a in range(0, length, TILE)]


def _merge_text(name, cov, mod, a=0, b=None):
    return merge.format_host(name, BASE, cov[0, a:b], mod[0, a:b], cov[1, a:b], mod[1, a:b], first_pos=a)


def _merge_case(name, length):
    """Four records per position on average, every one with modified > 0: lines in every tile, tiles of about the same size."""
    rng = np.random.default_rng(length)
    n = 4 * length
    pos, strand, cov = np.r_[0, length - 1, rng.integers(0, length, n)], np.r_[0, 1, rng.integers(0, 2, n)], rng.integers(1, 3000, n + 2)
    mod = 1 + (cov - 1) * rng.integers(0, 101, n + 2) // 100
    sums = np.zeros((2, 2, length), np.int64)
    np.add.at(sums[0], (strand, pos), cov)
    np.add.at(sums[1], (strand, pos), mod)
    return MergeCase((pos, strand, cov, mod), sums[0], sums[1], _merge_text(name, sums[0], sums[1]),
                     [len(_merge_text(name, sums[0], sums[1], a, b)) for a, b in _tiles(length)])


def _lists_case(c, name, length):
    seq, recs = make_contig(np.random.default_rng(1000 + length), length, MOTIF, K, R)
    host = bslabels.HostEngine(NAMES, LENGTHS, R, COV, HI, LO)
    host.open(c, seq, MOTIF, K)
    for r, (pos, strand, cov, pct) in enumerate(recs):
        host.fill(r, pos, bsperf.pack_meta(np.full(len(pos), c, np.int64), strand, cov, pct))
    host.classify()
    cls = host.fetch_classes()
    text = {w: bslabels.format_list_host(name, cls, w) for w in bslabels.LISTS.values()}
    return ListsCase(seq, recs, cls, text, {w: [len(bslabels.format_list_host(name, cls[:, a:b], w, a)) for a, b in _tiles(length)] for w in text})


@pytest.fixture(scope="module")
def want():
    """The fills and what the host formatters make of them, computed once (no GPU)."""
    return ([_merge_case(name, n) for name, n in zip(NAMES, LENGTHS)], [_lists_case(c, name, n) for c, (name, n) in enumerate(zip(NAMES, LENGTHS))])


def host_runs(tile_bytes, cap):
    """The runs of whole tiles the writer makes with buffers of cap bytes: tiles without text are skipped, a run takes every next tile that still fits."""
    runs, t = 0, 0
    while t < len(tile_bytes):
        if tile_bytes[t] == 0:
            t += 1
            continue
        assert tile_bytes[t] <= cap
        room = cap
        while t < len(tile_bytes) and tile_bytes[t] <= room:
            room -= tile_bytes[t]
            t += 1
        runs += 1
    return runs


def test_the_fills_need_two_runs_by_the_host_formatters_own_count(want):
    merges, lists = want
    for case in merges:
        assert sum(case.tile_bytes) == len(case.text) > 0
    assert host_runs(merges[0].tile_bytes, max(merges[0].tile_bytes)) >= 2
    for case in lists:
        assert all(sum(case.tile_bytes[w]) == len(case.text[w]) for w in case.text)
    assert all(host_runs(lists[0].tile_bytes[w], max(lists[0].tile_bytes[w])) >= 2 for w in bslabels.LISTS.values())
    assert [len(lists[1].text[w]) > 0 for w in (bslabels.C_FUL, bslabels.C_ANY, bslabels.C_NO)] == [True, False, False]     # the contig of one position: two empty lists
    assert merge.tile_positions() == bslabels.tile_positions() == TILE


def _merge_runs(d, cap):
    """-> (text, runs, lines, bytes, largest tile) with buffers of cap(largest tile, bytes) bytes."""
    lines, nbytes, largest = d.format_begin(BASE)
    buf, parts, more = np.empty(max(cap(largest, nbytes), 1), np.uint8), [], nbytes > 0
    while more:
        more, part = d.format_next(buf)
        assert 0 < len(part) <= len(buf)
        parts.append(part.tobytes())
    return b''.join(parts), len(parts), lines, nbytes, largest


@pytest.mark.gpu
def test_merge_formats_contig_after_contig_on_one_handle(gpu_device, want):
    d = merge.DeviceMerge(gpu_device)
    try:
        for name, length, case in zip(NAMES, LENGTHS, want[0]):
            d.open(name, length)
            before = d.times()
            assert d.format_begin(BASE) == (0, 0, 0) and d.times() == before       # an empty table: no text, no format time
            d.add_records(*case.records)
            text, runs, lines, nbytes, largest = _merge_runs(d, lambda tile, whole: tile)
            print('merge %s: %d bytes, largest tile %d, %d runs, format ms %r -> %r' % (name, nbytes, largest, runs, before[2], d.times()[2]))
            assert text == case.text and (lines, nbytes, largest) == (case.text.count(b'\n'), len(case.text), max(case.tile_bytes))
            assert runs == host_runs(case.tile_bytes, largest) >= (2 if length > 3 * TILE else 1)
            assert d.times()[2] > before[2]
            assert _merge_runs(d, lambda tile, whole: whole)[:2] == (case.text, 1)
        # a format cut off by an add is over; a fresh one gives the new sums
        d.format_begin(BASE)
        d.add_records([5], [0], [7], [3])
        with pytest.raises(_lib.DeepModHipError, match='dm_bedmerge_format_next: no format begun') as err:
            d.format_next(np.empty(1 << 20, np.uint8))
        assert err.value.code == _lib.DM_ESTATE
        cov, mod = case.cov.copy(), case.mod.copy()
        cov[0, 5] += 7
        mod[0, 5] += 3
        new = _merge_text(name, cov, mod)
        assert new != case.text and _merge_runs(d, lambda tile, whole: tile)[0] == new
    finally:
        d.close()


@pytest.mark.gpu
def test_bslabels_formats_contig_after_contig_on_one_handle(gpu_device, want):
    dev = bslabels.DeviceEngine(NAMES, LENGTHS, R, COV, HI, LO, gpu_device)
    try:
        for c, (name, length, case) in enumerate(zip(NAMES, LENGTHS, want[1])):
            dev.open(c, case.seq, MOTIF, K)
            for r, (pos, strand, cov, pct) in enumerate(case.recs):
                dev.fill(r, pos, bsperf.pack_meta(np.full(len(pos), c, np.int64), strand, cov, pct))
            dev.classify()
            assert np.array_equal(dev.fetch_classes(), case.cls)
            for which in bslabels.LISTS.values():                                  # all three lists of a contig, one after the other
                text, tile_bytes = case.text[which], case.tile_bytes[which]
                before = dev.times()
                n_lines, n_bytes, largest, runs = whole_text(dev, which, None)     # buffers of exactly the largest tile's bytes
                print('bslabels %s list %d: %d bytes, largest tile %d, %d runs, format ms %r -> %r' % (name, which, n_bytes, largest, len(runs), before[3], dev.times()[3]))
                assert b''.join(runs) == text and (n_lines, n_bytes, largest) == (text.count(b'\n'), len(text), max(tile_bytes))
                assert len(runs) == host_runs(tile_bytes, largest) >= (2 if length > 3 * TILE else 0)
                if text:
                    assert dev.times()[3] > before[3] and dev.times()[:3] == before[:3]
                else:
                    assert dev.times() == before                                   # a list without a line: no format time
                assert whole_text(dev, which, max(n_bytes, 1))[3] == ([text] if text else [])
            dev.close_contig()
    finally:
        dev.close()
