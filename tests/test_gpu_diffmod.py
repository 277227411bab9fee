"""GPU (-m gpu): `diffmod` on the device (csrc/diffmod.hip.inc) against diffmod.HostEngine, the oracle in exact rationals: counters and records
exact, p within the derived bound of DESIGN.md 21 (diffmod_synth.check_p: relative 1e-9 for cA + cB <= 4096, 1e-6 above, <= 1e-289 for an exact p
below 1e-290), at the tile edges of the select kernel, on both paths of the test kernel and at their split, at MAX_TOTAL and above it; the edges
of the two compactions; accumulation, reset, bit-identical repeats and the refusals of the C ABI; and the command on the device against the command
under HostEngine on the synthetic case of tests/diffmod_synth.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import _lib, diffmod, merge, summary

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import diffmod_synth  # noqa: E402
import long_cases  # noqa: E402

pytestmark = pytest.mark.gpu

COV, FDR = diffmod_synth.COV, diffmod_synth.FDR
INT_FIELDS = ('pos', 'strand', 'cA', 'mA', 'cB', 'mB')


class Tables:
    """The device tables of the sample and of the controls, filled through merge.DeviceMerge as the command fills them."""

    def __init__(self):
        self.dm = {'sample': merge.DeviceMerge(0), 'control': merge.DeviceMerge(0)}

    def fill(self, recs, n):
        out = []
        for role in ('sample', 'control'):
            self.dm[role].open('c', n)
            if len(recs[role][0]):
                self.dm[role].add_records(*recs[role])
            out += [self.dm[role].plus, self.dm[role].minus]
        return out

    def close(self):
        for dm in self.dm.values():
            dm.close()


def host_side(recs, n):
    return diffmod_synth.host_tables(recs['sample'], n) + diffmod_synth.host_tables(recs['control'], n)


def hist_of(p):
    return np.bincount(np.minimum(diffmod.HIST_BINS - 1, (diffmod.HIST_BINS * np.asarray(p, np.float64)).astype(np.int64)), minlength=diffmod.HIST_BINS)


def check_against_host(got, want, what):
    """Records of the device under alpha 1 against HostEngine's: the same keys in the same order, the integer columns equal, p within the bound."""
    for k in INT_FIELDS:
        assert got[k].tolist() == want[k].tolist(), (what, k)
    for i, (p, exact) in enumerate(zip(got['p'].tolist(), want['p'].tolist())):
        diffmod_synth.check_p(p, exact, int(want['cA'][i]) + int(want['cB'][i]), (what, i, [int(want[k][i]) for k in INT_FIELDS]))


@pytest.fixture(scope='module')
def sweep_lengths():
    t = diffmod.tile_positions()
    return [t - 1, t, t + 1, 3 * t + 5]


@pytest.mark.parametrize('which', range(4))
def test_sweep_equals_host_engine(hip_lib, sweep_lengths, which):
    n, tile, small = sweep_lengths[which], diffmod.tile_positions(), diffmod.small_support()
    assert small >= 65 and diffmod.max_total() == diffmod.MAX_TOTAL == 1 << 20
    keys = diffmod_synth.sweep_keys(small, diffmod.MAX_TOTAL)
    supports = {min(cA, mA + mB) - max(0, mA + mB - cB) + 1 for cA, mA, cB, mB in keys if cA >= COV and cB >= COV and cA + cB <= diffmod.MAX_TOTAL}
    assert set(diffmod_synth.SUPPORTS) | {small, small + 1, 5001} <= supports
    recs = diffmod_synth.layout(keys, n, tile, which)
    dev, low, host = diffmod.DeviceEngine(COV, 1.0), diffmod.DeviceEngine(COV, FDR), diffmod.HostEngine(COV, 1.0)
    tables = Tables()
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(*d)
        want_counters, want = host.run(*host_side(recs, n))
        assert counters.tolist() == want_counters.tolist(), (n, counters, want_counters)
        assert (want_counters > 0).all()                              # every fate, on both strands
        assert len(got['p']) == dev.n_records == want_counters[:, 0].sum()
        assert (np.diff(2 * got['pos'].astype(np.int64) + got['strand']) > 0).all()                  # key order
        check_against_host(got, want, n)
        assert (got['cA'].astype(np.int64) + got['cB']).max() == diffmod.MAX_TOTAL                   # a key exactly at MAX_TOTAL was tested
        assert dev.fetch_hist().tolist() == hist_of(got['p']).tolist()                              # the histogram of the device's own p
        # alpha 0.05: exactly the records of alpha 1 with p <= alpha, bit for bit; the histogram is of every tested key all the same
        counters2, part = low.run(*d)
        keep = got['p'] <= FDR
        assert counters2.tolist() == counters.tolist() and 0 < keep.sum() < len(keep)
        for k in INT_FIELDS + ('p',):
            assert part[k].tobytes() == got[k][keep].tobytes(), k
        assert low.fetch_hist().tolist() == dev.fetch_hist().tolist()
    finally:
        tables.close()
        dev.close(), low.close()


def test_sweep_wraps_the_grid_and_the_tile_scan_carries(hip_lib):
    """2,050 tiles (long_cases.diffmod_wrap): select_kernel's workgroup 0 takes tiles 0 and 2,048, workgroup 1 tile 1 and the ragged 2,049, and
    scan_kernel carries its total over nine groups of 256 tile counts.  The criterion of test_sweep_equals_host_engine."""
    tile, small = diffmod.tile_positions(), diffmod.small_support()
    n, recs = long_cases.diffmod_wrap(tile, small, diffmod.MAX_TOTAL)
    tiles = (n + tile - 1) // tile
    assert tiles > 2048 and tiles > 256                               # dfk::MAX_BLOCKS: the grid wraps; dfk::THREADS: the scan takes a second group
    want_counters, want = long_cases.diffmod_wrap_oracle(tile, small, diffmod.MAX_TOTAL)
    dev, low = diffmod.DeviceEngine(COV, 1.0), diffmod.DeviceEngine(COV, FDR)
    tables = Tables()
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(*d)
        assert counters.tolist() == want_counters.tolist(), (n, counters, want_counters)
        assert (want_counters > 0).all()                              # every fate, on both strands
        assert len(got['p']) == dev.n_records == want_counters[:, 0].sum()
        assert (np.diff(2 * got['pos'].astype(np.int64) + got['strand']) > 0).all()                  # key order
        check_against_host(got, want, n)
        assert (got['cA'].astype(np.int64) + got['cB']).max() == diffmod.MAX_TOTAL
        assert set(long_cases.WRAP_TILE_SET) | {tiles - 1} <= long_cases.tiles_holding(got['pos'], tile)      # tiles 0 | 2,048, 2,047 | 2,049, 255 | 256 | 257
        assert dev.fetch_hist().tolist() == hist_of(got['p']).tolist()                              # the histogram of the device's own p
        counters2, part = low.run(*d)
        keep = got['p'] <= FDR
        assert counters2.tolist() == counters.tolist() and 0 < keep.sum() < len(keep)
        for k in INT_FIELDS + ('p',):
            assert part[k].tobytes() == got[k][keep].tobytes(), k
        assert low.fetch_hist().tolist() == dev.fetch_hist().tolist()
    finally:
        tables.close()
        dev.close(), low.close()


def test_chunk_scan_carries_and_records_compact_across_groups(hip_lib):
    """More than 65,536 + 256 tested keys in one run (long_cases.diffmod_chunks): scan_kernel over more than 256 chunk counts, records_kernel reading
    chunk_off beyond the first group; records fetched in runs that straddle record 65,536."""
    tile = diffmod.tile_positions()
    n, recs, keys, dropped, tested = long_cases.diffmod_chunks(tile)
    group = 256 * 256                                                 # dfk::THREADS counts per group of the scan x dfk::CHUNK work items per chunk
    want_counters, want = long_cases.diffmod_chunks_oracle(tile)
    dev, low = diffmod.DeviceEngine(COV, 1.0), diffmod.DeviceEngine(COV, FDR)
    tables = Tables()
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(*d)
        assert counters.tolist() == want_counters.tolist()
        assert counters[:, 0].sum() == tested > group + 256 == 65792
        assert len(got['p']) == dev.n_records == tested               # alpha 1: every key is a record
        assert (np.diff(2 * got['pos'].astype(np.int64) + got['strand']) > 0).all()
        check_against_host(got, want, 'chunks')
        assert dev.fetch_hist().tolist() == hist_of(got['p']).tolist()
        counters2, part = low.run(*d)
        keep = got['p'] <= FDR
        assert counters2.tolist() == counters.tolist() and keep[:group].any() and keep[group:].any() and not keep.all()       # records of chunk groups 0 and 1
        for k in INT_FIELDS + ('p',):
            assert part[k].tobytes() == got[k][keep].tobytes(), k
        assert low.fetch_hist().tolist() == dev.fetch_hist().tolist()
        for first, count, run in ((group - 100, 300, 77), (group - 1, 2, 1), (0, dev.n_records, 50000)):
            piece = dev.fetch_records(first, count, fetch_run=run)
            for k in INT_FIELDS + ('p',):
                assert piece[k].tobytes() == got[k][first:first + count].tobytes(), (k, first)
    finally:
        tables.close()
        dev.close(), low.close()


def test_large_keys_wrap_their_grid(hip_lib):
    """1,200 keys above small_support() (long_cases.diffmod_large: three distinct ones, one of them underflowing) between small keys: fisher_kernel<true>
    loops over its list with barriers and wave_sum reused; the list is filled by an atomic in no particular order, and p must not depend on it."""
    n, recs, n_large = long_cases.diffmod_large()
    small = diffmod.small_support()
    assert all(long_cases.support_of(*k) > small for k in long_cases.LARGE_KEYS) and n_large > 1024          # dfk::LARGE_BLOCKS
    dev, host = diffmod.DeviceEngine(COV, 1.0), diffmod.HostEngine(COV, 1.0)
    tables = Tables()
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(*d)
        want_counters, want = host.run(*host_side(recs, n))
        assert counters.tolist() == want_counters.tolist() and counters[:, 0].sum() == 2 * n
        large = np.array([long_cases.support_of(*k) > small for k in zip(*(got[f].tolist() for f in ('cA', 'mA', 'cB', 'mB')))])
        assert large.sum() == n_large and large[0::2].all() and not large[1::2].any()                     # interleaved with small keys
        check_against_host(got, want, 'large')
        assert (want['p'][large] < 1e-290).any() and (want['p'][large] >= 1e-290).any()                 # the underflowing key and the others
        again = dev.run(*d)[1]
        for k in INT_FIELDS + ('p',):
            assert again[k].tobytes() == got[k].tobytes(), k        # two runs: the same bits
    finally:
        tables.close()
        dev.close()


def test_compaction_edges(hip_lib):
    """A tile where every key is tested, one where none is, a ragged last one; alpha so small that no record remains, and alpha 1; records fetched in
    runs smaller than a tile's worth."""
    tile = diffmod.tile_positions()
    n = 2 * tile + 300
    keys, _ = diffmod_synth.random_keys(23, 400, 40)
    keys = [k for k in keys if k[0] >= COV and k[2] >= COV]
    rng = np.random.default_rng(2)
    pick = rng.integers(0, len(keys), (n, 2))
    rows = {'sample': [], 'control': []}
    for p in range(n):
        for s in range(2):
            cA, mA, cB, mB = keys[pick[p, s]]
            if tile <= p < 2 * tile:
                cA, mA = (COV - 1, 0) if (p + s) % 2 else (0, 0)        # the middle tile: shallow in the sample or no sample record at all
            elif p >= 2 * tile and (p + s) % 3 == 0:
                continue
            if cA:
                rows['sample'].append((p, s, cA, mA))
            rows['control'].append((p, s, cB, mB))
    recs = {k: tuple(np.array([r[j] for r in v], np.int64) for j in range(4)) for k, v in rows.items()}
    dev, none, host = diffmod.DeviceEngine(COV, 1.0), diffmod.DeviceEngine(COV, 1e-300), diffmod.HostEngine(COV, 1.0)
    tables = Tables()
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(*d)
        want_counters, want = host.run(*host_side(recs, n))
        assert counters.tolist() == want_counters.tolist()
        first = got['pos'] < tile
        assert first.sum() == 2 * tile and not ((got['pos'] >= tile) & (got['pos'] < 2 * tile)).any() and (got['pos'] >= 2 * tile).sum() > 0
        check_against_host(got, want, 'edges')
        whole = dev.fetch_records(0, dev.n_records)
        pieces = dev.fetch_records(0, dev.n_records, fetch_run=100)
        middle = dev.fetch_records(37, 1000, fetch_run=333)
        for k in INT_FIELDS + ('p',):
            assert whole[k].tobytes() == pieces[k].tobytes() == got[k].tobytes() and middle[k].tobytes() == got[k][37:1037].tobytes(), k
        counters0, nothing = none.run(*d)
        assert counters0.tolist() == counters.tolist() and none.n_records == 0 and all(len(v) == 0 for v in nothing.values())
        assert none.fetch_hist().tolist() == dev.fetch_hist().tolist() == hist_of(got['p']).tolist()
        # tables without a tested key at all: no work list, no record, the histogram as it was
        empty = {k: tuple(np.zeros(0, np.int64) for _ in range(4)) for k in ('sample', 'control')}
        counters1, nothing = dev.run(*tables.fill(empty, tile + 1))
        assert not counters1.any() and dev.n_records == 0 and len(nothing['p']) == 0 and dev.fetch_hist().tolist() == hist_of(got['p']).tolist()
    finally:
        tables.close()
        dev.close(), none.close()


def test_accumulation_reset_and_identical_bits(hip_lib):
    tile = diffmod.tile_positions()
    keys = diffmod_synth.sweep_keys(diffmod.small_support(), diffmod.MAX_TOTAL)
    dev = diffmod.DeviceEngine(COV, 1.0)
    tables = Tables()
    try:
        total, hist, runs = np.zeros((2, 4), np.int64), np.zeros(diffmod.HIST_BINS, np.int64), []
        for n, phase in ((700, 0), (tile + 300, 1), (700, 0)):
            counters, got = dev.run(*tables.fill(diffmod_synth.layout(keys, n, tile, phase), n))
            total += counters
            hist += hist_of(got['p'])
            runs.append(got)
        assert dev.counters.tolist() == total.tolist() and dev.fetch_hist().tolist() == hist.tolist() and hist.sum() == total[:, 0].sum() > 0
        for k in INT_FIELDS + ('p',):
            assert runs[0][k].tobytes() == runs[2][k].tobytes(), k   # two identical runs: the same bits
        dev.reset()
        assert not dev.counters.any() and not dev.fetch_hist().any() and dev.n_records == 0
        counters, got = dev.run(*tables.fill(diffmod_synth.layout(keys, 700, tile, 0), 700))
        assert got['p'].tobytes() == runs[0]['p'].tobytes() and dev.fetch_hist().tolist() == hist_of(got['p']).tolist()
        assert all(v > 0 for v in dev.times())
    finally:
        tables.close()
        dev.close()


def test_abi_refusals(hip_lib):
    lib = hip_lib
    for args, words in (((0, 0.05), b'coverage'), ((-3, 0.05), b'coverage'), ((5, 0.0), b'alpha'), ((5, 1.5), b'alpha'), ((5, -0.1), b'alpha'), ((5, float('nan')), b'alpha')):
        assert not lib.dm_diffmod_create(0, *args) and words in lib.dm_last_error(), args
    assert not lib.dm_diffmod_create(99, 5, 0.05) and b'no device 99' in lib.dm_last_error()
    h = lib.dm_diffmod_create(0, 5, 1.0)
    assert h
    counters, got = np.full(8, -1, np.int64), ctypes.c_int64(-1)
    tabs = [summary.PositionSummary(8) for _ in range(4)]
    short = summary.PositionSummary(7)
    p = [t._h for t in tabs]
    out = (counters.ctypes.data, ctypes.byref(got))
    one = np.zeros(1, np.int64)
    arrays = [np.zeros(1, t) for _, t in diffmod.RECORD_FIELDS]
    rec = [a.ctypes.data for a in arrays]
    try:
        for call, words in ((lambda: lib.dm_diffmod_run(None, p[0], p[1], p[2], p[3], *out), b'null handle'),
                            (lambda: lib.dm_diffmod_run(h, None, p[1], p[2], p[3], *out), b'null handle'),
                            (lambda: lib.dm_diffmod_run(h, p[0], p[0], p[2], p[3], *out), b'one per strand'),
                            (lambda: lib.dm_diffmod_run(h, p[0], p[1], None, None, *out), b'the controls are missing'),
                            (lambda: lib.dm_diffmod_run(h, p[0], p[1], p[2], None, *out), b'the controls are missing'),
                            (lambda: lib.dm_diffmod_run(h, p[0], p[1], p[2], p[0], *out), b'of their own'),
                            (lambda: lib.dm_diffmod_run(h, p[0], short._h, p[2], p[3], *out), b'tables of different lengths: table 1 has 7 positions'),
                            (lambda: lib.dm_diffmod_run(h, p[0], p[1], p[2], short._h, *out), b'tables of different lengths: table 3 has 7 positions'),
                            (lambda: lib.dm_diffmod_run(h, p[0], p[1], p[2], p[3], None, ctypes.byref(got)), b'null argument'),
                            (lambda: lib.dm_diffmod_fetch_records(None, 0, 0, *rec), b'null handle'),
                            (lambda: lib.dm_diffmod_fetch_records(h, 0, 1, *rec), b'records 0 .. 1 of 0'),
                            (lambda: lib.dm_diffmod_fetch_records(h, -1, 0, *rec), b'records -1'),
                            (lambda: lib.dm_diffmod_fetch_hist(None, one.ctypes.data), b'null handle'),
                            (lambda: lib.dm_diffmod_fetch_hist(h, None), b'null argument'),
                            (lambda: lib.dm_diffmod_reset(None), b'null handle'),
                            (lambda: lib.dm_diffmod_times(None, None, None), b'null handle')):
            assert call() == _lib.DM_EINVAL and words in lib.dm_last_error(), lib.dm_last_error()
        assert (counters == -1).all() and got.value == -1              # nothing was run
        a, b = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        assert lib.dm_diffmod_times(h, ctypes.byref(a), ctypes.byref(b)) == 0 and a.value == 0.0 and b.value == 0.0          # and nothing was launched
        if lib.dm_device_count() > 1:                                  # a table on another device
            far = summary.PositionSummary(8, device=1)
            assert lib.dm_diffmod_run(h, p[0], far._h, p[2], p[3], *out) == _lib.DM_EINVAL and b'is on device 1' in lib.dm_last_error()
            far.close()
        # and the handle still works: empty tables, nothing to count
        assert lib.dm_diffmod_run(h, p[0], p[1], p[2], p[3], *out) == 0 and not counters.any() and got.value == 0
        assert lib.dm_diffmod_fetch_records(h, 0, 0, *rec) == 0
        lib.dm_diffmod_destroy(None)
    finally:
        lib.dm_diffmod_destroy(h)
        for t in tabs + [short]:
            t.close()


class Recording(diffmod.DeviceEngine):
    """The device engine, keeping the records it hands to the command."""

    def run(self, *tabs):
        counters, rec = super().run(*tabs)
        self.seen = getattr(self, 'seen', []) + [rec]
        return counters, rec


def test_command_on_the_device_equals_the_command_under_host_engine(hip_lib, tmp_path):
    root = str(tmp_path)
    case = diffmod_synth.write_case(root)
    recording = Recording(COV, 1.0)
    try:
        for key, options, alpha, engine in (('default', {}, FDR, None), ('all', {'all': 1}, 1.0, recording)):       # engine None: DeviceEngine on GPU 0
            want = diffmod_synth.run_command(case, root, diffmod.HostEngine(COV, alpha), 'host_' + key, **options)
            got = diffmod_synth.run_command(case, root, engine, 'dev_' + key, **options)
            rows, wrows = diffmod_synth.parse_report(got['txt']), diffmod_synth.parse_report(want['txt'])
            assert [r[:10] for r in rows] == [r[:10] for r in wrows] and len(rows) > 30, key              # the listed keys and every integer column
            for r, w in zip(rows, wrows):
                for j in (10, 11):                                     # p and q as printed: seven digits
                    assert abs(r[j] - w[j]) <= 1.1e-6 * w[j], (key, r, w)
            for doc in (got['json'], want['json']):
                doc['inputs'].pop('FileID')
            assert got['json'] == want['json'], key                   # counters, m, listed, hyper, hypo, the histogram, the notes
            assert any('mod_pos.chrB-.C.bed: line 1 is outside the device grammar: the file is parsed on the host' in n for n in got['json']['notes'])
        m = got['json']['m']
        assert got['json']['listed'] == m == len(rows)
        # p and q of every tested key, as the device handed them over, within the bound: every key of this case has cA + cB <= 4096
        rec = {k: np.concatenate([r[k] for r in recording.seen]) for k, _ in diffmod.RECORD_FIELDS}
        exact = np.array([diffmod.exact_p(*(int(rec[k][i]) for k in ('cA', 'mA', 'cB', 'mB'))) for i in range(m)])
        assert len(rec['p']) == m and (rec['cA'].astype(np.int64) + rec['cB']).max() <= 4096
        for i in range(m):
            diffmod_synth.check_p(float(rec['p'][i]), float(exact[i]), 4096, i)
        q, want_q = diffmod.bh_qvalues(rec['p'], m), diffmod.bh_qvalues(exact, m)
        assert (np.abs(q - want_q) <= 1e-9 * want_q).all()
    finally:
        recording.close()
