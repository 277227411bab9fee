"""CPU: reads with basecaller move tables (detect --move).  The host definition dm_move_events and its Python restatement
(rawreads.getEvent's move branch) against tests/golden/host_move.npz - recorded from the reference's own getFast5Info with
moptions['move'] = True (tests/golden/make_golden_move.py) -, the cases where the reference is undefined, damaged tables (also under
AddressSanitizer: tests/move_asan_driver.cpp), the container members, the CLI flag and the generator."""
import ctypes
import hashlib
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from deepmod_amd import _lib, rawreads, signal as dm_signal, synth_reads


@pytest.fixture(scope='module')
def golden():
    z = np.load(os.path.join(GOLDEN, 'host_move.npz'))
    return {c: {k: z[c + '_' + k] for k in ('raw', 'move', 'first', 'fq_seq', 'basecall', 'start', 'length', 'mean', 'stdv')} for c in z['cases'].tolist()}


def _one(move, first, nsig, fq):
    """dm_move_events on one read, every array exactly as long as the call says (no slack behind the tables)"""
    move = np.array(move, np.uint8)
    fq = fq.encode() if isinstance(fq, str) else fq
    return dm_signal.move_events(move, [0, len(move)], [first], [0, nsig], fq, [0, len(fq)])


def test_golden_covers_the_cases_the_kernels_care_about(golden):
    assert len(golden) >= 12
    bounds = {c: 1 + np.flatnonzero(g['move'][1:] == 1) for c, g in golden.items()}
    assert any({63, 64, 65} <= set(b.tolist()) for b in bounds.values())
    assert any(len(b) and b[-1] == len(golden[c]['move']) - 1 for c, b in bounds.items())
    assert any((g['move'] == 2).any() for g in golden.values())
    assert {int(g['move'][0]) for g in golden.values() if len(g['move'])} >= {0, 1}
    assert {int(g['first']) % 2 for g in golden.values()} == {0, 1}
    gaps = np.concatenate([np.diff(b) for b in bounds.values() if len(b) > 1])
    assert (gaps > 64).any() and (gaps > 1024).any()
    assert min(len(str(g['fq_seq'])) for g in golden.values()) == 1 and max(len(str(g['fq_seq'])) for g in golden.values()) >= 3000


def test_host_function_equals_the_reference(hip_lib, golden):
    for name, g in golden.items():
        fq = str(g['fq_seq'])
        mev_off, status, start, length, bases = _one(g['move'], int(g['first']), len(g['raw']), fq)
        assert status.tolist() == [_lib.DM_MOVE_OK] and mev_off.tolist() == [0, len(fq)], name
        assert start.dtype == np.uint64 and np.array_equal(start, g['start']) and np.array_equal(length, g['length']), name
        assert bases.tobytes().decode() == str(g['basecall']) == fq, name
        # every event of a read that passes is non-empty and inside the signal
        assert (length > 0).all() and int(start[-1] + length[-1]) == len(g['raw']), name


def test_all_reads_of_a_container_in_one_call(hip_lib, golden):
    gs = list(golden.values())
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    fqs = [str(g['fq_seq']).encode() for g in gs]
    mev_off, status, start, length, bases = dm_signal.move_events(np.concatenate([g['move'] for g in gs]), off([g['move'] for g in gs]), [int(g['first']) for g in gs],
                                                                  off([g['raw'] for g in gs]), b''.join(fqs), off(fqs))
    assert not status.any() and np.array_equal(mev_off, off(fqs))
    assert np.array_equal(start, np.concatenate([g['start'] for g in gs])) and np.array_equal(length, np.concatenate([g['length'] for g in gs]))
    assert bases.tobytes() == b''.join(fqs)


def test_python_restatement_equals_the_reference(golden):
    for name, g in golden.items():
        sp = {'f5status': '', 'raw_signals': g['raw'], 'move': g['move'], 'first_sample_template': int(g['first']), 'fq_seq': str(g['fq_seq'])}
        rawreads.getEvent({'move': True}, sp)
        assert sp['f5status'] == '' and sp['m_event_basecall'] == str(g['basecall']) and sp['left_right_skip'] == (0, 0), name
        assert np.array_equal(sp['m_event']['start'], g['start']) and np.array_equal(sp['m_event']['length'], g['length']), name
        assert ''.join(rawreads.event_bases(sp['m_event']['model_state']).tolist()) == str(g['fq_seq']), name


# table, first, samples, bases -> status: the cases where the reference is undefined
INVALID = {
    'too many boundaries': ([1, 1, 0, 1, 1, 0], 4, 40, 'ACG', _lib.DM_MOVE_COUNT),
    'too few boundaries': ([1, 0, 0, 1, 0, 0], 4, 40, 'ACG', _lib.DM_MOVE_COUNT),
    'no bases': ([1, 0, 0], 4, 40, '', _lib.DM_MOVE_COUNT),
    'empty table': ([], 4, 40, 'ACG', _lib.DM_MOVE_COUNT),
    'last boundary at the end of the signal': ([1, 0, 1, 0, 0, 1], 4, 14, 'ACG', _lib.DM_MOVE_OUTSIDE),
    'last boundary past the signal': ([1, 0, 1, 0, 0, 1], 4, 9, 'ACG', _lib.DM_MOVE_OUTSIDE),
    'first at the end of the signal': ([1, 0, 1, 0, 0, 1], 40, 40, 'ACG', _lib.DM_MOVE_OUTSIDE),
    'first past the signal': ([0], 41, 40, 'A', _lib.DM_MOVE_OUTSIDE),
    'first negative': ([1, 0, 1, 0, 0, 1], -1, 40, 'ACG', _lib.DM_MOVE_OUTSIDE),
    'no samples': ([1], 0, 0, 'A', _lib.DM_MOVE_OUTSIDE),
    'count decided before the signal': ([1, 1, 1, 1], -3, 2, 'AC', _lib.DM_MOVE_COUNT),
}


@pytest.mark.parametrize('case', sorted(INVALID))
def test_undefined_cases_fail_the_read(hip_lib, case):
    move, first, nsig, fq, want = INVALID[case]
    mev_off, status, start, length, bases = _one(move, first, nsig, fq)
    assert status.tolist() == [want] and mev_off.tolist() == [0, 0] and len(start) == 0
    sp = {'f5status': '', 'raw_signals': np.zeros(nsig, np.int16), 'move': np.array(move, np.uint8), 'first_sample_template': first, 'fq_seq': fq}
    with pytest.raises(ValueError):                       # get_Event_Signals files it under "Cannot open fast5 or other errors"
        rawreads.getEvent({'move': True}, sp)


def test_last_boundary_one_sample_before_the_end_is_valid(hip_lib):
    mev_off, status, start, length, _ = _one([1, 0, 1, 0, 0, 1], 4, 15, 'ACG')
    assert status.tolist() == [0] and start.tolist() == [4, 8, 14] and length.tolist() == [4, 6, 1]


def test_an_invalid_read_leaves_its_neighbours_alone(hip_lib, golden):
    a, b = golden['ordinary_300'], golden['value_two']
    bad = np.array([1, 1, 1, 1], np.uint8)
    parts = [a['move'], bad, b['move']]
    off = lambda p: np.concatenate([[0], np.cumsum([len(x) for x in p])]).astype(np.int64)
    fqs = [str(a['fq_seq']).encode(), b'AC', str(b['fq_seq']).encode()]
    mev_off, status, start, length, bases = dm_signal.move_events(np.concatenate(parts), off(parts), [int(a['first']), 0, int(b['first'])],
                                                                  [0, len(a['raw']), len(a['raw']) + 30, len(a['raw']) + 30 + len(b['raw'])], b''.join(fqs), off(fqs))
    assert status.tolist() == [0, _lib.DM_MOVE_COUNT, 0]
    assert mev_off.tolist() == [0, len(fqs[0]), len(fqs[0]), len(fqs[0]) + len(fqs[2])]
    assert np.array_equal(start, np.concatenate([a['start'], b['start']])) and np.array_equal(length, np.concatenate([a['length'], b['length']]))
    assert bases.tobytes() == fqs[0] + fqs[2]


def test_damaged_offsets_are_an_error_code(hip_lib):
    lib = hip_lib
    move, fq = np.array([1, 0, 1, 0, 1, 0], np.uint8), np.frombuffer(b'ACGTAC', np.uint8).copy()
    out = [np.empty(8, np.int64), np.empty(8, np.int32), np.empty(8, np.uint64), np.empty(8, np.uint64), np.empty(8, 'S1')]

    def call(mv_off, raw_off, fq_off, n=2, n_move=len(move), n_fq=len(fq)):
        arrs = [np.array(a, np.int64) for a in (mv_off, [2, 3], raw_off, fq_off)]
        return lib.dm_move_events(n, n_move, move.ctypes.data, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, n_fq, fq.ctypes.data,
                                  arrs[3].ctypes.data, *[o.ctypes.data for o in out])
    assert call([0, 3, 6], [0, 20, 40], [0, 2, 4]) == 4
    assert call([0, 3, 7], [0, 20, 40], [0, 2, 4]) == _lib.DM_EINVAL            # the table ends before its offsets do
    assert call([0, 4, 3], [0, 20, 40], [0, 2, 4]) == _lib.DM_EINVAL            # offsets that decrease
    assert call([-1, 3, 6], [0, 20, 40], [0, 2, 4]) == _lib.DM_EINVAL
    assert call([0, 3, 6], [0, 20, 40], [0, 2, 7]) == _lib.DM_EINVAL            # more bases than the sequence holds
    assert call([0, 3, 6], [0, 20, 40], [0, 5, 4]) == _lib.DM_EINVAL
    assert call([0, 3, 6], [0, 20, 10], [0, 2, 4]) == _lib.DM_EINVAL            # sample offsets that decrease
    assert call([0, 3, 6], [0, 20, 40], [0, 2, 4], n=-1) == _lib.DM_EINVAL
    assert call([0, 3, 6], [0, 20, 40], [0, 2, 4], n_move=5) == _lib.DM_EINVAL
    assert b'offsets' in lib.dm_last_error()
    assert lib.dm_move_events(1, 0, None, None, None, None, 0, None, None, None, None, None, None, None) == _lib.DM_EINVAL


def test_host_function_under_address_sanitizer(tmp_path):
    """tests/move_asan_driver.cpp: the host part of the ABI as tests/asan/host_shim.cpp restates it (included, not changed), built as a PROGRAM with
    -fsanitize=address,undefined and the sanitizer runtime linked in statically - every table in a heap block of exactly its size, valid, undefined
    and damaged cases.  The program runs in the environment of the test as it is (a statically linked runtime needs no place in the library order)."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'move_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'move_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'MOVE-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]


# ---- containers ----
def _move_reads(n=7, seed=5, twin=True):
    rng = np.random.default_rng(seed)
    genome = synth_reads.synthetic_genome(20000, seed)
    return [synth_reads.synthetic_raw_read(rng, genome, 'chrT', 'mv_%d' % i, min_len=200, max_len=500, move=True, twin=twin) for i in range(n)]


def test_container_round_trip_move_both_and_old(tmp_path, hip_lib):
    from deepmod_amd import npzmap
    reads = _move_reads()
    # a move container: no ev_* members
    p = str(tmp_path / ('a' + rawreads.RAW_SUFFIX))
    rawreads.save_raw_container(p, reads)
    z = npzmap.load(p)
    assert set(rawreads.MOVE_MEMBERS) <= set(z) and not any(k.startswith('ev_') for k in z) and int(z['format']) == 2
    assert z['mv'].dtype == np.uint8 and z['mv_off'].dtype == np.int64 and z['mv_first'].dtype == np.int64 and z['fq'].dtype == np.uint8
    back = rawreads.load_raw_container(p)
    for rd, b in zip(reads, back):
        assert b['read_id'] == rd['read_id'] and np.array_equal(b['raw'], rd['raw']) and np.array_equal(b['move'], rd['move'])
        assert b['first_sample_template'] == rd['first_sample_template'] and b['fq_seq'] == rd['fq_seq'] and 'events_data' not in b
    # both tables
    both = [dict(rd, events_data=rd['twin']['events_data']) for rd in reads]
    p2 = str(tmp_path / ('b' + rawreads.RAW_SUFFIX))
    rawreads.save_raw_container(p2, both)
    back = rawreads.load_raw_container(p2)
    for rd, b in zip(both, back):
        assert np.array_equal(b['move'], rd['move']) and b['fq_seq'] == rd['fq_seq']
        for f in ('start', 'length', 'move', 'model_state', 'mean', 'stdv'):
            assert np.array_equal(b['events_data'][f], rd['events_data'][f])
    # without --move a container with both tables is an event-table container: getEvent takes the events
    sp = {'f5status': '', 'raw_signals': back[0]['raw'], 'events_data': back[0]['events_data'], 'move': back[0]['move'],
          'first_sample_template': back[0]['first_sample_template'], 'fq_seq': back[0]['fq_seq']}
    rawreads.getEvent({}, sp)
    assert np.array_equal(sp['m_event']['start'], both[0]['events_data']['start'])
    # an event-table container as before this change: the same members, byte for byte the same file as a container of reads without move keys
    p3, p4 = str(tmp_path / ('c' + rawreads.RAW_SUFFIX)), str(tmp_path / ('d' + rawreads.RAW_SUFFIX))
    rawreads.save_raw_container(p3, [rd['twin'] for rd in reads])
    assert sorted(npzmap.load(p3)) == sorted(['format', 'raw', 'raw_off', 'ev_off', 'meta'] + ['ev_' + f for f in rawreads._EV_FIELDS])
    back = rawreads.load_raw_container(p3)
    assert all('move' not in b and len(b['events_data']) == len(rd['fq_seq']) for b, rd in zip(back, reads))
    # ... and under --move it has no move data
    sp = {'f5status': '', 'raw_signals': back[0]['raw'], 'events_data': back[0]['events_data'], 'move': None}
    rawreads.getEvent({'move': True}, sp)
    assert sp['f5status'] == 'No move data'


class _PostedOnly:
    """stands where a feeder's signal normalizer stands: records what the compiled batch builder posts to the signal stage (no device)"""

    def __init__(self):
        self.posted = []

    def post_arrays(self, *a):
        self.posted.append(('tables', a))
        return (0, len(self.posted))

    def post_move(self, *a):
        self.posted.append(('move', a))
        return (0, len(self.posted))


def test_compiled_batch_builder_without_move_takes_the_event_tables_of_a_container_with_both(tmp_path, hip_lib):
    """Without --move nothing changes, also for a container that carries both tables: stream._prepare_batch_c on the `both` containers posts the same
    event-table request and builds the same batch as on the twin (event tables only) containers; with --move the same files post their move tables
    and the batch is again the same."""
    from deepmod_amd import stream
    d, t, both = str(tmp_path / 'mv'), str(tmp_path / 'twin'), str(tmp_path / 'both')
    files, fasta = synth_reads.write_synthetic_raw_run(d, n_reads=8, reads_per_file=4, genome_len=20000, seed=22, chrom='chrS', move=True, twin_dir=t)
    os.makedirs(both)
    for f in files:
        name = os.path.basename(f)
        mv, tw = rawreads.load_raw_container(f), rawreads.load_raw_container(os.path.join(t, name))
        rawreads.save_raw_container(os.path.join(both, name), [dict(a, events_data=b['events_data']) for a, b in zip(mv, tw)])
        shutil.copy(f[:-len(rawreads.RAW_SUFFIX)] + '.sam', os.path.join(both, name)[:-len(rawreads.RAW_SUFFIX)] + '.sam')

    def run(folder, move):
        st = _PostedOnly()
        mo = {'Base': 'C', 'Ref': fasta, 'alignStr': 'minimap2', 'move': move, 'region': [[None, None, None]], 'ConUnk': True, 'rows_in_c': True}
        return stream.prepare_batch(mo, [os.path.join(folder, os.path.basename(f)) for f in files], make_normalizer=lambda: st), st.posted
    want, want_posted = run(t, False)
    assert want.n_reads == 8 and not want.errors and [k for k, _ in want_posted] == ['tables']
    for folder, move, kind in ((both, False, 'tables'), (both, True, 'move'), (d, True, 'move')):
        got, posted = run(folder, move)
        assert [k for k, _ in posted] == [kind] and got.n_reads == 8 and not got.errors
        for name in ('code', 'rdesc', 'pos', 'flags', 'sel'):
            assert np.array_equal(getattr(got, name), getattr(want, name)), (folder, move, name)
        assert got.groups == want.groups and got.f32 == want.f32 and got.n_rows == want.n_rows
        if kind == 'tables':            # raw parts, raw_off, start, length, ev_off, first_empty: the request of the twin run
            a, b = posted[0][1], want_posted[0][1]
            assert np.array_equal(np.concatenate(a[0]), np.concatenate(b[0])) and all(np.array_equal(a[i], b[i]) for i in range(1, 6))
            assert a[6] is None and a[7] is None


def test_damaged_move_members_fail_the_container(tmp_path):
    from deepmod_amd import npzmap
    reads = _move_reads(4, twin=False)
    p = str(tmp_path / ('a' + rawreads.RAW_SUFFIX))
    rawreads.save_raw_container(p, reads)
    z = dict(npzmap.load(p))
    for key, edit in (('mv_off', lambda a: a[:-1]), ('mv_off', lambda a: a + 10 ** 9), ('mv_off', lambda a: a[::-1]), ('fq_off', lambda a: a * 3),
                      ('mv_first', lambda a: a[:2]), ('mv', lambda a: a[:10])):
        arrays = {k: np.array(v) for k, v in z.items()}
        arrays[key] = np.ascontiguousarray(edit(arrays[key]))
        q = str(tmp_path / ('bad' + rawreads.RAW_SUFFIX))
        with open(q, 'wb') as fh:
            npzmap.savez_aligned(fh, **arrays)
        with pytest.raises(ValueError):
            rawreads.load_raw_container(q)


# ---- command line ----
def test_detect_move_reaches_the_worker_options(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location('_dm_cli_move', os.path.join(ROOT, 'bin', 'DeepMod.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    from deepmod_amd import detect
    seen = []
    monkeypatch.setattr(detect, 'mDetect_manager', lambda mo: seen.append(dict(mo)))
    monkeypatch.setattr(cli, 'kfd_gpu_count', lambda: 1)
    (tmp_path / 'in').mkdir()
    (tmp_path / 'model.index').write_text('')
    common = ['detect', '--wrkBase', str(tmp_path / 'in'), '--modfile', str(tmp_path / 'model'), '--outFolder', str(tmp_path / 'out'), '--gpus', '1']
    for extra, want in ((['--move'], True), ([], False)):
        args = cli.build_parser().parse_args(common + extra)
        args.func(args)
        assert seen[-1]['move'] is want
    assert 'compatibility' not in [a for a in cli.build_parser()._subparsers._group_actions[0].choices['detect']._actions if '--move' in a.option_strings][0].help


# ---- generator ----
# sha256 of what write_synthetic_raw_run(d, n_reads=12, reads_per_file=5, genome_len=20000, seed=3) wrote before the move generator was added
DEFAULT_RUN_DIGESTS = {
    'genome.fa': '4b9f4c90b9459573ab5dd83d1f5073f6abd59a09d2fdb1b6610ba4dc508b1c05',
    'raw_0000.dmraw.npz': 'ba48e27149c810ebecf0ed1f12f02b2326c33f549baf8da04306872517dd27d5',
    'raw_0000.sam': '62bac96004d17452e22e7ac36cd0018006bc0a124c52a522f5e57ccf33e38dcc',
    'raw_0001.dmraw.npz': 'b675bcf7b82addb3f3d4fa89a829285a75cb48c0d7fef0589425e98011622c9f',
    'raw_0001.sam': '6c08ff8fff28100058f075679107971945b39c2466575424611419e7d406546b',
    'raw_0002.dmraw.npz': '92ce1eeef7c6dd83ccc88b911c781bed56f411c656c895cf773f2cde7cb8a13a',
    'raw_0002.sam': 'dcf047379b49341ce661d47c348c4bdb31cb216d2d86d884932168cbc3e26071',
}


def test_default_generator_output_is_unchanged(tmp_path):
    d = str(tmp_path / 'run')
    synth_reads.write_synthetic_raw_run(d, n_reads=12, reads_per_file=5, genome_len=20000, seed=3)
    assert {f: hashlib.sha256(open(os.path.join(d, f), 'rb').read()).hexdigest() for f in sorted(os.listdir(d))} == DEFAULT_RUN_DIGESTS


def test_generated_move_run_and_its_twin(tmp_path, hip_lib):
    d, t = str(tmp_path / 'mv'), str(tmp_path / 'twin')
    files, fasta = synth_reads.write_synthetic_raw_run(d, n_reads=11, reads_per_file=4, genome_len=20000, seed=9, move=True, twin_dir=t)
    assert len(files) == 3 and sorted(os.listdir(d)) == sorted(os.listdir(t))
    assert open(fasta, 'rb').read() == open(os.path.join(t, 'genome.fa'), 'rb').read()
    firsts = []
    for f in files:
        assert open(f[:-len(rawreads.RAW_SUFFIX)] + '.sam').read() == open(os.path.join(t, os.path.basename(f))[:-len(rawreads.RAW_SUFFIX)] + '.sam').read()
        mv, tw = rawreads.load_raw_container(f), rawreads.load_raw_container(os.path.join(t, os.path.basename(f)))
        off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        fqs = [rd['fq_seq'].encode() for rd in mv]
        mev_off, status, start, length, bases = dm_signal.move_events(np.concatenate([rd['move'] for rd in mv]), off([rd['move'] for rd in mv]),
                                                                      [rd['first_sample_template'] for rd in mv], off([rd['raw'] for rd in mv]), b''.join(fqs), off(fqs))
        assert not status.any()
        for i, (a, b) in enumerate(zip(mv, tw)):
            assert 'events_data' not in a and 'move' not in b and a['read_id'] == b['read_id'] and np.array_equal(a['raw'], b['raw'])
            ev = b['events_data']
            assert (np.asarray(ev['move']) == 1).all() and len(ev) == len(a['fq_seq'])
            assert np.array_equal(ev['start'], start[mev_off[i]:mev_off[i + 1]]) and np.array_equal(ev['length'], length[mev_off[i]:mev_off[i + 1]])
            assert ev['model_state'].tolist() == ['NN' + c + 'NN' for c in a['fq_seq']]
            assert ((np.asarray(ev['start'], np.int64) - a['first_sample_template']) % 2 == 0).all()
            firsts.append(a['first_sample_template'])
    assert len({f % 2 for f in firsts}) == 2
