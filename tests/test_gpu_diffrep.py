"""GPU (-m gpu): `diffmod --replicates 1` on the device (csrc/diffrep.hip.inc) against diffmod.RepHostEngine, the oracle in integers and 50-digit
decimals: counters and the integer columns of the records exact, phi and p within the derived interval of DESIGN.md 22 (diffrep_synth.bounds), at
the tile edges of the sweep and over the replicate shapes (1, 2), (2, 1), (2, 2), (3, 5), (8, 8); the edges of the compaction; accumulation, reset,
bit-identical repeats and the refusals of the C ABI; and the command on the device against the command under RepHostEngine on the synthetic case of
tests/diffrep_synth.py.  The tables are filled through merge.DeviceMerge as the command fills them, which stores no count outside 0 <= m <= c: the
hold of such counts is the host twin's to show (tests/test_diffrep_host.py, the same routine)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import _lib, diffmod, merge, summary

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import diffrep_synth as synth  # noqa: E402
import long_cases  # noqa: E402

pytestmark = pytest.mark.gpu

COV, FDR = synth.COV, synth.FDR
INT_FIELDS = ('pos', 'strand', 'cA', 'mA', 'cB', 'mB', 'nA', 'nB')
ALL_FIELDS = INT_FIELDS + ('phi', 'p')


class Tables:
    """The device tables of K replicates, filled through merge.DeviceMerge as the command fills them."""

    def __init__(self, K):
        self.dm = [merge.DeviceMerge(0) for _ in range(K)]

    def fill(self, recs, n):
        out = []
        for dm, rec in zip(self.dm, recs):
            dm.open('c', n)
            if len(rec[0]):
                dm.add_records(*rec)
            out.append((dm.plus, dm.minus))
        return out

    def close(self):
        for dm in self.dm:
            dm.close()


def device_keys(keys):
    """The keys a table filled from files can hold: 0 <= m <= c, and no coverage near 2^31 (merge refuses sums past int32)."""
    return [synth.held(k) for k in keys if max(k[0]) < 2 ** 30]


def hist_of(p):
    return np.bincount(np.minimum(diffmod.HIST_BINS - 1, (diffmod.HIST_BINS * np.asarray(p, np.float64)).astype(np.int64)), minlength=diffmod.HIST_BINS)


@pytest.fixture(scope='module')
def sweep_lengths():
    t = diffmod.tile_positions()
    return [t - 1, t, t + 1, 3 * t + 5]


@pytest.mark.parametrize('shape', synth.SHAPES)
@pytest.mark.parametrize('which', range(4))
def test_sweep_equals_rep_host_engine(hip_lib, sweep_lengths, which, shape):
    KA, KB = shape
    n, tile = sweep_lengths[which], diffmod.tile_positions()
    a, b = synth.low_min_reps(KA, KB) if which % 2 else (KA, KB)      # the default least counts, and one below
    keys = device_keys(synth.sweep_keys(KA, KB, a, b))
    recs = synth.layout(keys, KA + KB, n, tile, which)
    host_tabs = [synth.host_tables(rec, n) for rec in recs]
    dev, low, host = diffmod.RepDeviceEngine(COV, 1.0, a, b), diffmod.RepDeviceEngine(COV, FDR, a, b), diffmod.RepHostEngine(COV, 1.0, a, b)
    tables = Tables(KA + KB)
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(d[:KA], d[KA:])
        want_counters, want = host.run(host_tabs[:KA], host_tabs[KA:])
        assert counters.tolist() == want_counters.tolist(), (n, counters, want_counters)
        assert (want_counters > 0).all()                              # every fate, on both strands
        assert len(got['p']) == dev.n_records == want_counters[:, 0].sum()
        assert (np.diff(2 * got['pos'].astype(np.int64) + got['strand']) > 0).all()                  # key order
        for k in INT_FIELDS:
            assert got[k].tolist() == want[k].tolist(), (n, k)
        synth.check_records(got, host_tabs, KA, COV, a, b, (shape, n))
        ones = want['p'] == 1.0
        assert ones.sum() >= 2 and (got['p'][ones] == 1.0).all() and (got['phi'][ones] == 1.0).all()          # the integer rule: exactly 1
        assert (got['cA'].astype(np.int64) + got['cB']).max() == synth.MAX_TOTAL                     # a key exactly at MAX_TOTAL was tested
        assert {0, n - 1} <= set(got['pos'].tolist()) and (n <= tile or {tile - 1, tile} <= set(got['pos'].tolist()))
        assert dev.fetch_hist().tolist() == hist_of(got['p']).tolist()                              # the histogram of the device's own p
        # alpha 0.05: exactly the records of alpha 1 with p <= alpha, bit for bit; the histogram is of every tested key all the same
        counters2, part = low.run(d[:KA], d[KA:])
        keep = got['p'] <= FDR
        assert counters2.tolist() == counters.tolist() and 0 < keep.sum() < len(keep)
        for k in ALL_FIELDS:
            assert part[k].tobytes() == got[k][keep].tobytes(), k
        assert low.fetch_hist().tolist() == dev.fetch_hist().tolist()
    finally:
        tables.close()
        dev.close(), low.close()


@pytest.mark.parametrize('shape,which,phase', long_cases.REP_CASES)
def test_sweep_wraps_the_grid_and_the_tile_scan_carries(hip_lib, shape, which, phase):
    """(2, 2) on 2,050 tiles: sweep_kernel's workgroup 0 takes tiles 0 and 2,048, workgroup 1 tile 1 and the ragged 2,049; (8, 8) on 258 tiles: the
    scan of the tile counts carries into a second group with sixteen replicates' tables.  The criterion of test_sweep_equals_rep_host_engine."""
    KA, KB = shape
    tile = diffmod.tile_positions()
    n, (a, b), recs = long_cases.diffrep_case(shape, which, phase, tile)
    tiles = (n + tile - 1) // tile
    assert tiles > 256 and (which != 'wrap' or tiles > 2048)          # dfk::THREADS: the scan takes a second group; dfk::MAX_BLOCKS: the grid wraps
    host_tabs = long_cases.diffrep_host_tables(shape, which, phase, tile)
    want_counters, want = long_cases.diffrep_oracle(shape, which, phase, tile)
    dev, low = diffmod.RepDeviceEngine(COV, 1.0, a, b), diffmod.RepDeviceEngine(COV, FDR, a, b)
    tables = Tables(KA + KB)
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(d[:KA], d[KA:])
        assert counters.tolist() == want_counters.tolist(), (n, counters, want_counters)
        assert (want_counters > 0).all()                              # every fate, on both strands
        assert len(got['p']) == dev.n_records == want_counters[:, 0].sum()
        assert (np.diff(2 * got['pos'].astype(np.int64) + got['strand']) > 0).all()                  # key order
        for k in INT_FIELDS:
            assert got[k].tolist() == want[k].tolist(), (n, k)
        synth.check_records(got, host_tabs, KA, COV, a, b, (shape, n))
        ones = want['p'] == 1.0
        assert ones.sum() >= 2 and (got['p'][ones] == 1.0).all() and (got['phi'][ones] == 1.0).all()          # the integer rule: exactly 1
        assert (got['cA'].astype(np.int64) + got['cB']).max() == synth.MAX_TOTAL                     # a key exactly at MAX_TOTAL was tested
        held = long_cases.tiles_holding(got['pos'], tile)
        assert {0, n - 1, tile - 1, tile} <= set(got['pos'].tolist()) and {0, 255, 256, 257, tiles - 1} <= held
        assert which != 'wrap' or set(long_cases.WRAP_TILE_SET) <= held                             # tiles 0 | 2,048 and 2,047 | 2,049 as well
        assert dev.fetch_hist().tolist() == hist_of(got['p']).tolist()                              # the histogram of the device's own p
        counters2, part = low.run(d[:KA], d[KA:])
        keep = got['p'] <= FDR
        assert counters2.tolist() == counters.tolist() and 0 < keep.sum() < len(keep)
        for k in ALL_FIELDS:
            assert part[k].tobytes() == got[k][keep].tobytes(), k
        assert low.fetch_hist().tolist() == dev.fetch_hist().tolist()
    finally:
        tables.close()
        dev.close(), low.close()


def test_compaction_edges(hip_lib):
    """A tile where every key is tested, one where none is, a ragged last one; an alpha that leaves no record, and alpha 1; records fetched in runs
    smaller than a tile's worth."""
    KA, KB = 2, 2
    tile = diffmod.tile_positions()
    n = 2 * tile + 300
    keys = [k for k in synth.random_keys(KA, KB, 23, 60, 40) if min(k[0]) >= COV]
    assert len(keys) > 30
    rng = np.random.default_rng(2)
    pick = rng.integers(0, len(keys), (n, 2))
    rows = [[] for _ in range(KA + KB)]
    for p in range(n):
        for s in range(2):
            c, m = keys[pick[p, s]]
            if p >= 2 * tile and (p + s) % 3 == 0:
                continue
            for j in range(KA + KB):
                if tile <= p < 2 * tile and j == 0:                   # the middle tile: the first sample replicate shallow or absent
                    if (p + s) % 2:
                        rows[j].append((p, s, COV - 1, 0))
                    continue
                rows[j].append((p, s, c[j], m[j]))
    recs = [tuple(np.array([r[f] for r in v], np.int64) for f in range(4)) for v in rows]
    host_tabs = [synth.host_tables(rec, n) for rec in recs]
    dev, none, host = diffmod.RepDeviceEngine(COV, 1.0, KA, KB), diffmod.RepDeviceEngine(COV, 1e-300, KA, KB), diffmod.RepHostEngine(COV, 1.0, KA, KB)
    tables = Tables(KA + KB)
    try:
        d = tables.fill(recs, n)
        counters, got = dev.run(d[:KA], d[KA:])
        want_counters, want = host.run(host_tabs[:KA], host_tabs[KA:])
        assert counters.tolist() == want_counters.tolist()
        first = got['pos'] < tile
        assert first.sum() == 2 * tile and not ((got['pos'] >= tile) & (got['pos'] < 2 * tile)).any() and (got['pos'] >= 2 * tile).sum() > 0
        for k in INT_FIELDS:
            assert got[k].tolist() == want[k].tolist(), k
        synth.check_records(got, host_tabs, KA, COV, KA, KB, 'edges')
        whole = dev.fetch_records(0, dev.n_records)
        pieces = dev.fetch_records(0, dev.n_records, fetch_run=100)
        middle = dev.fetch_records(37, 1000, fetch_run=333)
        for k in ALL_FIELDS:
            assert whole[k].tobytes() == pieces[k].tobytes() == got[k].tobytes() and middle[k].tobytes() == got[k][37:1037].tobytes(), k
        counters0, nothing = none.run(d[:KA], d[KA:])
        assert counters0.tolist() == counters.tolist() and none.n_records == 0 and all(len(v) == 0 for v in nothing.values())
        assert none.fetch_hist().tolist() == dev.fetch_hist().tolist() == hist_of(got['p']).tolist()
        # tables without a key at all: no record, the histogram as it was
        empty = [tuple(np.zeros(0, np.int64) for _ in range(4))] * (KA + KB)
        d = tables.fill(empty, tile + 1)
        counters1, nothing = dev.run(d[:KA], d[KA:])
        assert not counters1.any() and dev.n_records == 0 and len(nothing['p']) == 0 and dev.fetch_hist().tolist() == hist_of(got['p']).tolist()
    finally:
        tables.close()
        dev.close(), none.close()


def test_accumulation_reset_and_identical_bits(hip_lib):
    KA, KB = 3, 5
    a, b = synth.low_min_reps(KA, KB)
    tile = diffmod.tile_positions()
    keys = device_keys(synth.sweep_keys(KA, KB, a, b))
    dev = diffmod.RepDeviceEngine(COV, 1.0, a, b)
    tables = Tables(KA + KB)
    try:
        total, hist, runs = np.zeros((2, 4), np.int64), np.zeros(diffmod.HIST_BINS, np.int64), []
        for n, phase in ((700, 0), (tile + 300, 1), (700, 0)):
            d = tables.fill(synth.layout(keys, KA + KB, n, tile, phase), n)
            counters, got = dev.run(d[:KA], d[KA:])
            total += counters
            hist += hist_of(got['p'])
            runs.append(got)
        assert dev.counters.tolist() == total.tolist() and dev.fetch_hist().tolist() == hist.tolist() and hist.sum() == total[:, 0].sum() > 0
        for k in ALL_FIELDS:
            assert runs[0][k].tobytes() == runs[2][k].tobytes(), k   # two identical runs: the same bits
        dev.reset()
        assert not dev.counters.any() and not dev.fetch_hist().any() and dev.n_records == 0
        d = tables.fill(synth.layout(keys, KA + KB, 700, tile, 0), 700)
        counters, got = dev.run(d[:KA], d[KA:])
        assert got['p'].tobytes() == runs[0]['p'].tobytes() and dev.fetch_hist().tolist() == hist_of(got['p']).tolist()
        assert all(v > 0 for v in dev.times())
    finally:
        tables.close()
        dev.close()


def test_abi_refusals(hip_lib):
    lib = hip_lib
    assert lib.dm_diffrep_max_replicates() == 8
    for args, words in (((0, 0.05, 1, 2), b'coverage'), ((5, 0.0, 1, 2), b'alpha'), ((5, 1.5, 1, 2), b'alpha'), ((5, float('nan'), 1, 2), b'alpha'),
                        ((5, 0.05, 0, 3), b'1 to 8 each'), ((5, 0.05, 9, 1), b'1 to 8 each'), ((5, 0.05, 1, 1), b'3 or more together')):
        assert not lib.dm_diffrep_create(0, *args) and words in lib.dm_last_error(), args
    assert not lib.dm_diffrep_create(99, 5, 0.05, 1, 2) and b'no device 99' in lib.dm_last_error()
    h = lib.dm_diffrep_create(0, 5, 1.0, 2, 2)
    assert h
    counters, got = np.full(8, -1, np.int64), ctypes.c_int64(-1)
    tabs = [summary.PositionSummary(8) for _ in range(18)]
    short = summary.PositionSummary(7)
    p = [t._h for t in tabs]
    out = (counters.ctypes.data, ctypes.byref(got))

    def lists(plus, minus):
        return (ctypes.c_void_p * len(plus))(*plus), (ctypes.c_void_p * len(minus))(*minus)

    def run(n_a, n_b, plus, minus, handle=h):
        return lib.dm_diffrep_run(handle, n_a, n_b, *lists(plus, minus), *out)

    one = np.zeros(1, np.int64)
    arrays = [np.zeros(1, t) for _, t in diffmod.REP_RECORD_FIELDS]
    rec = [a.ctypes.data for a in arrays]
    try:
        for call, words in ((lambda: run(2, 2, p[0:4], p[4:8], None), b'null handle'),
                            (lambda: lib.dm_diffrep_run(h, 2, 2, None, lists(p[0:4], p[4:8])[1], *out), b'null argument'),
                            (lambda: lib.dm_diffrep_run(h, 2, 2, *lists(p[0:4], p[4:8]), None, ctypes.byref(got)), b'null argument'),
                            (lambda: run(2, 2, [p[0], None, p[2], p[3]], p[4:8]), b'replicate 1: two tables, one per strand (null handle)'),
                            (lambda: run(2, 2, p[0:4], [p[4], p[5], p[6], p[0]]), b'the same table twice (replicate 0 and replicate 3)'),
                            (lambda: run(2, 2, [p[0], p[1], p[1], p[3]], p[4:8]), b'the same table twice (replicate 1 and replicate 2)'),
                            (lambda: run(0, 2, p[0:2], p[4:6]), b'1 to 8 replicates'),
                            (lambda: run(9, 2, p[0:11], p[4:15]), b'1 to 8 replicates'),
                            (lambda: run(2, -1, p[0:2], p[4:6]), b'1 to 8 replicates'),
                            (lambda: run(2, 1, p[0:3], p[4:7]), b'at most the replicates of either group'),
                            (lambda: run(2, 2, [p[0], short._h, p[2], p[3]], p[4:8]), b'tables of different lengths: table 2 has 7 positions'),
                            (lambda: run(2, 2, p[0:4], [p[4], p[5], p[6], short._h]), b'tables of different lengths: table 7 has 7 positions'),
                            (lambda: lib.dm_diffrep_fetch_records(None, 0, 0, *rec), b'null handle'),
                            (lambda: lib.dm_diffrep_fetch_records(h, 0, 1, *rec), b'records 0 .. 1 of 0'),
                            (lambda: lib.dm_diffrep_fetch_records(h, -1, 0, *rec), b'records -1'),
                            (lambda: lib.dm_diffrep_fetch_hist(None, one.ctypes.data), b'null handle'),
                            (lambda: lib.dm_diffrep_fetch_hist(h, None), b'null argument'),
                            (lambda: lib.dm_diffrep_reset(None), b'null handle'),
                            (lambda: lib.dm_diffrep_times(None, None, None), b'null handle')):
            assert call() == _lib.DM_EINVAL and words in lib.dm_last_error(), lib.dm_last_error()
        h12 = lib.dm_diffrep_create(0, 5, 1.0, 1, 2)                  # two replicates in all: refused whatever the least counts
        assert run(1, 1, p[0:2], p[4:6], h12) == _lib.DM_EINVAL and b'3 or more replicates together' in lib.dm_last_error()
        lib.dm_diffrep_destroy(h12)
        assert (counters == -1).all() and got.value == -1              # nothing was run
        ta, tb = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        assert lib.dm_diffrep_times(h, ctypes.byref(ta), ctypes.byref(tb)) == 0 and ta.value == 0.0 and tb.value == 0.0          # and nothing was launched
        if lib.dm_device_count() > 1:                                  # a table on another device
            far = summary.PositionSummary(8, device=1)
            assert run(2, 2, [p[0], far._h, p[2], p[3]], p[4:8]) == _lib.DM_EINVAL and b'is on device 1' in lib.dm_last_error()
            far.close()
        # and the handle still works: empty tables, nothing to count; 8 and 8 replicates at once
        assert run(2, 2, p[0:4], p[4:8]) == 0 and not counters.any() and got.value == 0
        h88 = lib.dm_diffrep_create(0, 5, 1.0, 8, 8)
        more = [summary.PositionSummary(8) for _ in range(14)]
        q = p + [t._h for t in more]
        assert run(8, 8, q[0:16], q[16:32], h88) == 0 and not counters.any() and got.value == 0
        lib.dm_diffrep_destroy(h88)
        for t in more:
            t.close()
        assert lib.dm_diffrep_fetch_records(h, 0, 0, *rec) == 0
        lib.dm_diffrep_destroy(None)
    finally:
        lib.dm_diffrep_destroy(h)
        for t in tabs + [short]:
            t.close()


class Recording(diffmod.RepDeviceEngine):
    """The device engine, keeping the records it hands to the command."""

    def run(self, sample, control):
        counters, rec = super().run(sample, control)
        self.seen = getattr(self, 'seen', []) + [rec]
        return counters, rec


def test_command_on_the_device_equals_the_command_under_rep_host_engine(hip_lib, tmp_path):
    root = str(tmp_path)
    case = synth.write_case(root)
    recording = Recording(COV, 1.0, 3, 2)
    try:
        for key, options, alpha, engine in (('default', {}, FDR, None), ('all', {'all': 1}, 1.0, recording)):       # engine None: RepDeviceEngine on GPU 0
            want = synth.run_command(case, root, diffmod.RepHostEngine(COV, alpha, 3, 2), 'host_' + key, **options)
            got = synth.run_command(case, root, engine, 'dev_' + key, **options)
            rows, wrows = synth.parse_report(got['txt']), synth.parse_report(want['txt'])
            assert [r[:12] for r in rows] == [r[:12] for r in wrows] and len(rows) > 30, key              # the listed keys and every integer column
            for r, w in zip(rows, wrows):
                assert abs(r[12] - w[12]) <= 1.01e-4                   # phi as printed: four decimals
                for j in (13, 14):                                     # p and q as printed: seven digits
                    assert abs(r[j] - w[j]) <= 1.1e-6 * w[j], (key, r, w)
            for doc in (got['json'], want['json']):
                doc['inputs'].pop('FileID')
            assert got['json'] == want['json'], key                   # counters, m, listed, hyper, hypo, the histogram, the notes, the replicates
            assert any('mod_pos.chrB-.C.bed: line 1 is outside the device grammar: the file is parsed on the host' in n for n in got['json']['notes'])
        m = got['json']['m']
        assert got['json']['listed'] == m == len(rows)
        # phi and p of every tested key, as the device handed them over, within the interval; q within what p allows
        rec = {k: np.concatenate([r[k] for r in recording.seen]) for k, _ in diffmod.REP_RECORD_FIELDS}
        assert len(rec['p']) == m
        exact = []
        for i, r in enumerate(rows):
            sample, control, _ = case['sites'][r[:3]]
            ua, ub = [s for s in sample if s[0] >= COV], [c for c in control if c[0] >= COV]
            synth.check_key(float(rec['p'][i]), float(rec['phi'][i]), ua, ub, r[:3])
            exact.append(diffmod.rep_exact_p(ua, ub))
        q, want_q = diffmod.bh_qvalues(rec['p'], m), diffmod.bh_qvalues(exact, m)
        assert (np.abs(q - want_q) <= 1e-8 * want_q).all()            # (every key of this case has C < 50,000: E / D stays far below this)
    finally:
        recording.close()
