"""GPU (-m gpu): reads with basecaller move tables (detect --move).  The device segmentation (dm_signal_move_stats_device: move tables in, event
statistics resident on the device) against tests/golden/host_move.npz - the reference's own getFast5Info with moptions['move'] = True - bit for
bit, against the host-table form (dm_move_events + dm_signal_event_stats_device) on handles with stale tables, growing buffers, 4,096 reads,
tables that straddle the kernels' chunk and ordinary malformed tables; then `DeepMod.py detect --move` end to end against the twin event-table
run, the oracle chain and the command's other forms."""
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from deepmod_amd import _lib, rawreads, readmap, signal as dm_signal, synth, synth_reads
from deepmod_amd.model import DeviceArray
from oracle import detect_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'host_move.npz'))
    return {c: {k: z[c + '_' + k] for k in ('raw', 'move', 'first', 'fq_seq', 'start', 'length', 'mean', 'stdv')} for c in z['cases'].tolist()}


def _read(g):
    return (g['raw'], g['move'], int(g['first']), len(str(g['fq_seq'])))


def _random_read(rng, n_bases, first=None, p=0.25, tail=None):
    """a valid move read (raw, move, first, bases): boundary gaps 1 + geometric(p) strides, signal levels per event"""
    gaps = 1 + rng.geometric(p, n_bases - 1)
    idx = np.cumsum(gaps)
    tail = int(rng.integers(1, 6)) if tail is None else tail
    L = (int(idx[-1]) if n_bases > 1 else 0) + tail
    move = np.zeros(L, np.uint8)
    move[idx] = 1
    move[0] = rng.integers(0, 3)
    first = int(rng.integers(0, 90)) if first is None else first
    n_raw = first + 2 * L + int(rng.integers(0, 2))
    level = np.repeat(rng.normal(0, 1, n_bases), np.diff(np.concatenate([[first], first + 2 * idx, [n_raw]])))
    raw = np.round(500 + 70 * np.concatenate([rng.normal(0, 1, first), level + rng.normal(0, 0.3, n_raw - first)])).astype(np.int16)
    return raw, move, first, n_bases


def _batch(reads):
    """reads [(raw, move, first, bases)] -> the arrays of dm_signal_move_stats_device"""
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return {'raw': np.concatenate([r[0] for r in reads]), 'raw_off': off([r[0] for r in reads]),
            'move': np.concatenate([r[1] for r in reads]).astype(np.uint8), 'mv_off': off([r[1] for r in reads]),
            'first': np.array([r[2] for r in reads], np.int64), 'ev_off': np.concatenate([[0], np.cumsum([r[3] for r in reads])]).astype(np.int64)}


def _host_tables(b):
    """dm_move_events on the batch (bases do not matter here) -> (status, ev_off of the reads that passed, start, length)"""
    fq = np.full(int(b['ev_off'][-1]), ord('A'), np.uint8)
    mev_off, status, start, length, _ = dm_signal.move_events(b['move'], b['mv_off'], b['first'], b['raw_off'], fq, b['ev_off'])
    return status, mev_off, start, length


def _device_move(nz, b):
    blk = DeviceArray((max(int(b['ev_off'][-1]), 1), 3), np.float32, 0)
    status, flag = nz.move_stats_device(b['raw'], b['raw_off'], b['move'], b['mv_off'], b['first'], b['ev_off'], blk.ptr)
    got = blk.to_host()[:int(b['ev_off'][-1])]
    blk.free()
    return got, status, flag


def _device_tables(nz, b):
    """the same batch (all reads valid) through the existing entry point with the host-built tables"""
    status, mev_off, start, length = _host_tables(b)
    assert not status.any() and np.array_equal(mev_off, b['ev_off'])
    blk = DeviceArray((int(mev_off[-1]), 3), np.float32, 0)
    fe, flag = nz.event_stats_device(b['raw'], b['raw_off'], start, length, mev_off, blk.ptr)
    assert np.array_equal(fe, np.diff(mev_off))             # every event of a read that passed is non-empty
    got = blk.to_host()
    blk.free()
    return got, flag


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _check_golden(got, b, cases):
    for i, g in enumerate(cases):
        rows = got[b['ev_off'][i]:b['ev_off'][i + 1]]
        assert _same_bits(rows[:, 0], g['mean']) and _same_bits(rows[:, 1], g['stdv']), i
        assert _same_bits(rows[:, 2], g['length'].astype(np.float64).astype(np.float32)), i


def test_golden_cases_bit_for_bit_and_equal_to_the_host_table_form(golden, gpu_device):
    cases = list(golden.values())
    b = _batch([_read(g) for g in cases])
    nz, nz2 = dm_signal.SignalNormalizer(0), dm_signal.SignalNormalizer(0)
    try:
        got, status, flag = _device_move(nz, b)
        assert not status.any()
        _check_golden(got, b, cases)
        want, want_flag = _device_tables(nz2, b)
        assert _same_bits(got, want) and flag == want_flag == 0
        # every read alone: the same bits (a one-read batch has other chunk numbers and offsets)
        for g in cases:
            b1 = _batch([_read(g)])
            got1, status1, _ = _device_move(nz, b1)
            assert not status1.any()
            _check_golden(got1, b1, [g])
    finally:
        nz.close()
        nz2.close()


def test_handle_with_stale_tables(golden, gpu_device):
    """the handle's event tables, move tables, chunk counts and value tables all hold another batch's data first (a wide event-table batch as
    tests/test_gpu_signal_edges.py poisons its handles, then a different move batch)"""
    from test_gpu_signal_edges import _poison_reads
    cases = list(golden.values())
    b = _batch([_read(g) for g in cases])
    rng = np.random.default_rng(77)
    other = _batch([_random_read(rng, int(rng.integers(100, 3000))) for _ in range(len(cases) + 3)])
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    poison = _poison_reads(len(cases) + 3, 5)
    nz = dm_signal.SignalNormalizer(0)
    try:
        blk = DeviceArray((int(sum(len(p[2]) for p in poison)), 3), np.float32, 0)
        nz.event_stats_device(np.concatenate([p[1] for p in poison]), off([p[1] for p in poison]), np.concatenate([p[2] for p in poison]),
                              np.concatenate([p[3] for p in poison]), off([p[2] for p in poison]), blk.ptr)
        blk.free()
        got_other, status, _ = _device_move(nz, other)
        assert not status.any()
        got, status, flag = _device_move(nz, b)
        assert not status.any() and flag == 0
        _check_golden(got, b, cases)
        want_other, _ = _device_tables(nz, other)           # ... and the event-table form behind move batches on the same handle
        assert _same_bits(got_other, want_other)
    finally:
        nz.close()


def test_buffer_growth_3_40_3_reads(golden, gpu_device):
    rng = np.random.default_rng(3)
    small = [_read(golden[c]) for c in ('ordinary_300', 'tiny_one_entry', 'value_two')]
    big = [_random_read(rng, int(rng.integers(50, 4000))) for _ in range(40)]
    nz, nz2 = dm_signal.SignalNormalizer(0), dm_signal.SignalNormalizer(0)
    try:
        for reads in (small, big, small):
            b = _batch(reads)
            got, status, flag = _device_move(nz, b)
            want, want_flag = _device_tables(nz2, b)
            assert not status.any() and _same_bits(got, want) and flag == want_flag
        _check_golden(got, b, [golden[c] for c in ('ordinary_300', 'tiny_one_entry', 'value_two')])
    finally:
        nz.close()
        nz2.close()


def test_batch_of_4096_reads(gpu_device):
    rng = np.random.default_rng(4096)
    reads = [_random_read(rng, int(rng.integers(1, 60))) for _ in range(4096)]
    b = _batch(reads)
    nz = dm_signal.SignalNormalizer(0)
    try:
        got, status, flag = _device_move(nz, b)
        want, want_flag = _device_tables(nz, b)
        assert not status.any() and _same_bits(got, want) and flag == want_flag
        one_more = _batch(reads + reads[:1])
        with pytest.raises(_lib.DeepModHipError):
            _device_move(nz, one_more)
    finally:
        nz.close()


def test_tables_that_straddle_the_chunk(gpu_device, hip_lib):
    """boundaries on both sides of every chunk edge: the last entries of a chunk, the first of the next, for every position of the read's table
    relative to the 16-byte words the kernels load (the chunk size comes from the library)"""
    chunk = int(hip_lib.dm_signal_move_chunk())
    assert chunk >= 64 and chunk % 16 == 0
    rng = np.random.default_rng(11)
    reads = []
    for shift in range(17):
        L = 2 * chunk + int(rng.integers(40, 400))
        move = (rng.random(L) < 0.2).astype(np.uint8)
        for edge in (chunk, 2 * chunk):
            move[edge - 34:edge + 34] = 0
            move[edge - 18:edge + 18] = 1                       # every entry around the edge, whatever the table's alignment (|shift| <= 16)
            move[[edge - 30, edge + 30]] = 2
        move[64 - 2:64 + 2] = 1
        move[L - 1] = 1
        first = int(rng.integers(0, 50))
        n_bases = int((move[1:] == 1).sum()) + 1
        n_raw = first + 2 * L
        raw = np.round(rng.normal(480, 60, n_raw)).astype(np.int16)
        reads.append((raw, move, first, n_bases))
        reads.append(_random_read(rng, 3 + shift, tail=1 + (shift + 7 * len(reads)) % 16))      # moves the next table off the 16-byte grid
    b = _batch(reads)
    assert len({int(o) % 16 for o in b['mv_off'][:-1:2]}) > 8
    # a table longer than one workgroup's scan tile (256 chunks) with a lone boundary behind a long run of zeros, and a table of exactly one chunk
    L = 300 * chunk + 5
    move = np.zeros(L, np.uint8)
    move[[1, chunk - 1, chunk, 257 * chunk, L - 1]] = 1
    reads.append((np.round(rng.normal(480, 60, 9 + 2 * L)).astype(np.int16), move, 9, 6))
    move = np.zeros(chunk, np.uint8)
    move[[chunk - 1]] = 1
    reads.append((np.round(rng.normal(480, 60, 2 * chunk)).astype(np.int16), move, 0, 2))
    b = _batch(reads)
    nz = dm_signal.SignalNormalizer(0)
    try:
        got, status, flag = _device_move(nz, b)
        want, want_flag = _device_tables(nz, b)
        assert not status.any() and _same_bits(got, want) and flag == want_flag
    finally:
        nz.close()


def test_malformed_tables_beside_valid_reads(golden, gpu_device):
    """One of each invalid kind between valid reads: the device's statuses are dm_move_events', the valid reads' rows are those of a batch
    without the invalid ones, an invalid read's rows are (NaN, NaN, 0), and the call returns without a device error (the handle goes on
    working).  A check of the guards on ordinary malformed data."""
    rng = np.random.default_rng(5)
    valid = [_read(golden[c]) for c in ('ordinary_300', 'wave_edges_last_at_L-1', 'long_zero_runs', 'tiny_empty_table')] + [_random_read(rng, 700)]
    r, m, f, nb = _random_read(rng, 900)
    chunk_read = _random_read(rng, 2500)
    invalid = [
        (r, m, f, nb - 7),                                       # too many boundaries for the bases (the surplus must not reach the next read's slots)
        (r, m, f, nb + 40),                                      # too few
        (r[:f + 2 * int(np.flatnonzero(m == 1)[-1])], m, f, nb),           # the last boundary at the end of the signal
        (r[:f + 2 * int(np.flatnonzero(m == 1)[-1]) - 5], m, f, nb),       # ... past it
        (r, m, len(r), nb),                                      # first >= samples
        (r, m, -1, nb),                                          # first < 0
        (r, np.zeros(0, np.uint8), f, nb),                       # empty table
        (chunk_read[0], chunk_read[1], chunk_read[2], 3),        # thousands of surplus boundaries, over several chunks
    ]
    reads = []
    for i, bad in enumerate(invalid):
        reads += [valid[i % len(valid)], bad]
    reads.append(valid[-1])
    is_valid = [i % 2 == 0 for i in range(len(reads))]
    b = _batch(reads)
    want_status = _host_tables(b)[0]
    assert [s == 0 for s in want_status.tolist()] == is_valid
    assert sorted(set(want_status.tolist())) == [_lib.DM_MOVE_OK, _lib.DM_MOVE_COUNT, _lib.DM_MOVE_OUTSIDE]
    nz, nz2 = dm_signal.SignalNormalizer(0), dm_signal.SignalNormalizer(0)
    try:
        got, status, flag = _device_move(nz, b)
        assert status.tolist() == want_status.tolist() and flag == 0
        only = _batch([rd for rd, ok in zip(reads, is_valid) if ok])
        want, _ = _device_tables(nz2, only)
        k = 0
        for i, ok in enumerate(is_valid):
            rows = got[b['ev_off'][i]:b['ev_off'][i + 1]]
            if ok:
                assert _same_bits(rows, want[only['ev_off'][k]:only['ev_off'][k + 1]]), i
                k += 1
            else:
                assert np.isnan(rows[:, :2]).all() and (rows[:, 2] == 0).all(), i
        again, status, _ = _device_move(nz, only)               # the handle goes on working
        assert not status.any() and _same_bits(again, want)
    finally:
        nz.close()
        nz2.close()


def test_range_flag_keeps_its_meaning(golden, gpu_device):
    """The flag covers the means / stdvs the call COMPUTED.  A failed read's (NaN, NaN, 0) rows are not computed values and leave it clear; a valid
    read of a constant signal beside them (scale 0: the reference divides by zero, every statistic NaN - the batch must take the fp32 kernel)
    raises it, exactly as the host-table form does for the same read."""
    rng = np.random.default_rng(8)
    good = _read(golden['ordinary_300'])
    r, m, f, nb = _random_read(rng, 400)
    bad = (r, m, f, nb + 3)                                       # too few boundaries
    cm = np.zeros(300, np.uint8)
    cm[10::10] = 1
    const = (np.full(40 + 2 * len(cm), 612, np.int16), cm, 40, int((cm[1:] == 1).sum()) + 1)
    nz, nz2 = dm_signal.SignalNormalizer(0), dm_signal.SignalNormalizer(0)
    try:
        b = _batch([good, bad])
        got, status, flag = _device_move(nz, b)
        assert status.tolist() == [0, _lib.DM_MOVE_COUNT] and flag == 0
        assert np.isnan(got[b['ev_off'][1]:, :2]).all()
        b = _batch([good, bad, const])
        got, status, flag = _device_move(nz, b)
        assert status.tolist() == [0, _lib.DM_MOVE_COUNT, 0] and flag == 1
        only = _batch([good, const])
        want, want_flag = _device_tables(nz2, only)
        assert want_flag == 1
        assert _same_bits(got[:b['ev_off'][1]], want[:only['ev_off'][1]]) and np.isnan(want[only['ev_off'][1]:, :2]).all()
        assert _same_bits(got[b['ev_off'][2]:], want[only['ev_off'][1]:])
        _check_golden(got, b, [golden['ordinary_300']])
        b = _batch([good, bad])                                   # ... and the flag is the call's, not the handle's
        assert _device_move(nz, b)[2] == 0
    finally:
        nz.close()
        nz2.close()


# ---- the command ----
def _detect(wrk, prefix, out, fid, extra=(), env=None, threads='2'):
    cmd = [sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'detect', '--wrkBase', str(wrk), '--modfile', prefix, '--Ref', os.path.join(str(wrk), 'genome.fa'),
           '--outFolder', out, '--FileID', fid, '--threads', threads, '--files_per_thread', '2', '--Base', 'C', '--gpus', '1', '--alignStr', 'minimap2'] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))


def _beds(out, fid):
    return {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob('%s/%s/*.bed' % (out, fid)))}


def _fp32_batches(stdout):
    m = re.search(r'classifier: (\d+) of (\d+) batches switched to the fp32 kernel', stdout)
    assert m, stdout[-1500:]
    return int(m.group(1)), int(m.group(2))


def test_detect_move_end_to_end(tmp_path, gpu_device):
    """`detect --move` on a generated move run = `detect` on the twin event-table run = the oracle chain on the twin containers = the command's other
    forms, byte for byte.  Conditions (checked here): no read is skipped and the oracle reports no window within 1e-4 of a tie for this seed."""
    wrk, twin = tmp_path / 'mv', tmp_path / 'twin'
    files, fasta = synth_reads.write_synthetic_raw_run(str(wrk), n_reads=18, reads_per_file=4, genome_len=20000, seed=22, chrom='chrS', move=True, twin_dir=str(twin))
    prefix = str(tmp_path / 'model' / 'm')
    os.makedirs(os.path.dirname(prefix))
    w = synth.write_synthetic_checkpoint(prefix, seed=9, scale=4.0)         # smallest |p1 - 0.5| 1.2e-4 on this read set, 21 % class 1
    out = str(tmp_path / 'out')
    # the oracle chain first (CPU)
    from oracle_pipeline import oracle_raw_container
    genome = readmap.read_fasta(fasta)['chrS']
    by_strand, n_reads, n_ties = {'+': [], '-': []}, 0, 0
    for f in files:
        got_reads, n, margin, ties = oracle_raw_container(os.path.join(str(twin), os.path.basename(f)), genome, w)
        for strand in '+-':
            by_strand[strand].extend(got_reads[strand])
        n_reads += n
        n_ties += sum(len(v) for v in ties.values())
        assert margin > 1e-4, 'the generated set has a near-tie window (%.2e); pick another seed' % margin
    assert n_reads == 18 and n_ties == 0
    want = {'mod_pos.chrS%s.C.bed' % s: detect_oracle.sum_handler_oracle('chrS', s, 'C', by_strand[s]) for s in '+-'}
    assert all(len(v) > 500 for v in want.values())

    runs = {}
    for fid, src, extra, env in (('move', wrk, ['--move'], {}), ('twin', twin, [], {}), ('move_host_tables', wrk, ['--move'], {'DEEPMOD_MOVE_ON_DEVICE': '0'}),
                                 ('move_host_stats', wrk, ['--move'], {'DEEPMOD_STATS_ON_DEVICE': '0'}), ('move_py', wrk, ['--move'], {'DEEPMOD_ROWS_IN_C': '0'})):
        res = _detect(src, prefix, out, fid, extra, env)
        assert res.returncode == 0, fid + res.stdout[-1500:] + res.stderr[-3000:]
        assert 'Streaming detect: 18 reads' in res.stdout, fid + res.stdout[-1500:]
        assert 'Cannot open fast5' not in res.stdout and 'No move data' not in res.stdout and 'Less Event' not in res.stdout, fid + res.stdout[-1500:]
        runs[fid] = (_beds(out, fid), res.stdout)
    for fid, (beds, stdout) in runs.items():
        assert beds == want, fid
    m = re.search(r'event statistics resident on the device for (\d+) of (\d+) rows', runs['move'][1])
    assert m and int(m.group(1)) == int(m.group(2)) > 0, runs['move'][1][-1500:]
    # the default form posted the move tables themselves (one byte per two samples); with DEEPMOD_MOVE_ON_DEVICE=0 none travelled
    m = re.search(r'in (\d+) requests \((\d+) of them carried move tables, segmented on the device: (\d+) table bytes\)', runs['move'][1])
    assert m and int(m.group(1)) == int(m.group(2)) > 0 and int(m.group(3)) > 0, runs['move'][1][-1500:]
    assert 'carried move tables' not in runs['move_host_tables'][1] and 'carried move tables' not in runs['twin'][1]
    m = re.search(r'event statistics resident on the device for (\d+) of (\d+) rows', runs['move_host_stats'][1])
    assert m and int(m.group(1)) == 0
    fp32 = {fid: _fp32_batches(stdout) for fid, (_, stdout) in runs.items()}
    assert all(v == fp32['move'] for v in fp32.values()), fp32      # the fp32 batch counts are equal across the forms


def test_detect_without_move_on_containers_that_carry_both_tables(tmp_path, gpu_device):
    """Without --move nothing changes, also for a container that carries both tables: the command on containers with event tables AND move members
    writes the BED of the twin (event tables only) run and posts no move table; with --move the same files give the same BED from their move tables."""
    import shutil
    wrk, twin, both = tmp_path / 'mv', tmp_path / 'twin', tmp_path / 'both'
    files, fasta = synth_reads.write_synthetic_raw_run(str(wrk), n_reads=18, reads_per_file=4, genome_len=20000, seed=22, chrom='chrS', move=True, twin_dir=str(twin))
    both.mkdir()
    shutil.copy(fasta, str(both / 'genome.fa'))
    for f in files:
        name = os.path.basename(f)
        mv, tw = rawreads.load_raw_container(f), rawreads.load_raw_container(str(twin / name))
        rawreads.save_raw_container(str(both / name), [dict(a, events_data=b['events_data']) for a, b in zip(mv, tw)])
        shutil.copy(f[:-len(rawreads.RAW_SUFFIX)] + '.sam', str(both / name)[:-len(rawreads.RAW_SUFFIX)] + '.sam')
    prefix = str(tmp_path / 'model' / 'm')
    os.makedirs(os.path.dirname(prefix))
    synth.write_synthetic_checkpoint(prefix, seed=9, scale=4.0)
    out = str(tmp_path / 'out')
    runs = {}
    for fid, src, extra in (('twin', twin, []), ('both', both, []), ('both_move', both, ['--move'])):
        res = _detect(src, prefix, out, fid, extra)
        assert res.returncode == 0 and 'Streaming detect: 18 reads' in res.stdout, fid + res.stdout[-1500:] + res.stderr[-3000:]
        runs[fid] = (_beds(out, fid), res.stdout)
    assert len(runs['twin'][0]) == 2 and all(len(v) > 500 for v in runs['twin'][0].values())
    assert runs['both'][0] == runs['twin'][0] and runs['both_move'][0] == runs['twin'][0]
    assert 'carried move tables' not in runs['both'][1] and 'carried move tables' in runs['both_move'][1]
    sig = lambda so: re.search(r'signal stage: (\d+) samples, (\d+) merged events in (\d+) requests', so).groups()
    assert sig(runs['both'][1])[:2] == sig(runs['twin'][1])[:2]


def test_detect_move_with_two_ranks(tmp_path, gpu_device):
    """`detect --move --gpus 2` (both ranks on device 0, the shared-memory stand-in for the collective library, as tests/test_gpu_multirank.py runs its raw
    case) writes the one-process BED files"""
    from shim import build as shim_build
    wrk = tmp_path / 'mv'
    synth_reads.write_synthetic_raw_run(str(wrk), n_reads=36, reads_per_file=3, genome_len=30000, seed=5, chrom='chrM2', min_len=300, max_len=1200, move=True)
    prefix = str(tmp_path / 'model' / 'm')
    os.makedirs(os.path.dirname(prefix))
    synth.write_synthetic_checkpoint(prefix, seed=26, scale=4.0)
    env = dict(os.environ, DEEPMOD_RCCL_LIBRARY=shim_build.library(), DEEPMOD_ONE_DEVICE='1')
    env.pop('DM_BENCH_FORCE_DIST', None)
    out = str(tmp_path / 'out')
    one = _detect(wrk, prefix, out, 'one', ['--move'], threads='4')
    assert one.returncode == 0, one.stdout[-1500:] + one.stderr[-3000:]
    cmd = [sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'detect', '--wrkBase', str(wrk), '--modfile', prefix, '--Ref', str(wrk / 'genome.fa'), '--outFolder', out,
           '--FileID', 'many', '--threads', '4', '--Base', 'C', '--alignStr', 'minimap2', '--move', '--gpus', '2']
    many = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert many.returncode == 0, many.stdout[-1500:] + many.stderr[-3000:]
    assert 'event statistics resident on the device' in many.stdout
    assert len(_beds(out, 'one')) == 2 and all(len(v) > 2000 for v in _beds(out, 'one').values())
    assert _beds(out, 'many') == _beds(out, 'one')


def test_detect_move_on_an_event_table_container(tmp_path, gpu_device):
    """--move on containers without move data: every read under "No move data" (the reference's reason), the exit of a run whose reads all failed"""
    wrk = tmp_path / 'raw'
    synth_reads.write_synthetic_raw_run(str(wrk), n_reads=8, reads_per_file=4, genome_len=20000, seed=8, chrom='chrS')
    prefix = str(tmp_path / 'model' / 'm')
    os.makedirs(os.path.dirname(prefix))
    synth.write_synthetic_checkpoint(prefix, seed=26, scale=4.0)
    out = str(tmp_path / 'out')
    plain = _detect(wrk, prefix, out, 'plain')
    assert plain.returncode == 0 and 'Streaming detect: 8 reads' in plain.stdout, plain.stdout[-1500:] + plain.stderr[-3000:]
    res = _detect(wrk, prefix, out, 'nomove', ['--move'])
    both = res.stdout + res.stderr
    assert re.search(r'No move data 8\b', both), both[-3000:]
    assert 'Streaming detect: 0 reads' in res.stdout, both[-3000:]
    assert not any(len(v) for v in _beds(out, 'nomove').values())
    # ... "as for other all-failed runs": the same exit code as a run whose containers cannot be opened at all
    bad = tmp_path / 'bad'
    bad.mkdir()
    (bad / ('x' + rawreads.RAW_SUFFIX)).write_bytes(b'not a container')
    (bad / 'genome.fa').write_bytes(open(str(wrk / 'genome.fa'), 'rb').read())
    failed = _detect(bad, prefix, out, 'bad')
    assert res.returncode == failed.returncode, (res.returncode, failed.returncode, both[-2000:])
