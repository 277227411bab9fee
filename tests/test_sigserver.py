"""CPU: the bookkeeping of the signal server thread (deepmod_amd/sigserver.py signal_server), without a device: the three device calls, the page-locked
buffer, the dm_signal handle and the block pool are stand-ins; the requests are real request files written by RemoteSignalNormalizer.  What is held:
the acknowledgement goes out once per resident request, whatever fails; a block taken from the pool is registered with its result or given back, never
both, never neither; a failing request never ends the thread; the synchronous form writes its outputs back behind the inputs."""
import ctypes
import queue
import threading
import types

import numpy as np
import pytest

from deepmod_amd import _lib, model, sigserver, signal as dmsignal


class _Pinned:
    """model.PinnedArray over numpy memory"""
    made = []

    def __init__(self, nbytes, device=0):
        self.nbytes, self._a, self.freed = int(nbytes), np.zeros(max(int(nbytes), 1), np.uint8), 0
        self.ptr = self._a.ctypes.data
        _Pinned.made.append(self)

    def view(self, dtype, count, offset=0):
        return np.frombuffer(self._a, dtype, count, offset)

    def free(self):
        self.freed += 1


class _Pool:
    """DeviceBlockPool that counts: a block is a numpy array with .ptr"""

    def __init__(self):
        self.taken, self.given = [], []

    def take(self, nbytes):
        blk = types.SimpleNamespace(nbytes=nbytes, a=np.zeros(nbytes, np.uint8))
        blk.ptr = blk.a.ctypes.data
        self.taken.append(blk)
        return blk

    def give(self, blk):
        self.given.append(blk)


def _i64(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_int64 * n).from_address(ptr)).copy()


@pytest.fixture
def server(tmp_path, monkeypatch):
    """A signal_server thread over stand-ins -> namespace(norm: the feeder's client, script: what the next device call returns, calls, pool, results,
    answers, stats, handle, stop())"""
    _Pinned.made = []
    handle = types.SimpleNamespace(_h=1234, closed=0)
    handle.close = lambda: setattr(handle, 'closed', handle.closed + 1)
    script = {'rc': 0, 'status': None, 'flags': 0}
    calls = []

    def event_device(h, n, raw, raw_off, ev_start, ev_length, ev_off, first_empty, fb_mean, fb_stdv, blk, unused, flags):
        calls.append(('event', h, n, _i64(raw_off, n + 1), _i64(ev_off, n + 1), _i64(first_empty, n), fb_mean is not None, blk))
        flags._obj.value = script['flags']
        return script['rc']

    def move_device(h, n, raw, raw_off, move, mv_off, first, ev_off, blk, status, unused, flags):
        calls.append(('move', h, n, _i64(raw_off, n + 1), _i64(mv_off, n + 1), _i64(first, n), blk))
        (ctypes.c_int32 * n).from_address(status)[:] = script['status'] or [0] * n
        flags._obj.value = script['flags']
        return script['rc']

    def event_batch(h, n, raw, raw_off, ev_start, ev_length, ev_off, mean, stdv, norm6, first_empty):
        n_ev = int(_i64(ev_off, n + 1)[-1])
        calls.append(('batch', h, n, _i64(raw_off, n + 1), n_ev))
        (ctypes.c_float * n_ev).from_address(mean)[:] = [1.0 + i for i in range(n_ev)]
        (ctypes.c_float * n_ev).from_address(stdv)[:] = [0.5 * i for i in range(n_ev)]
        (ctypes.c_int64 * n).from_address(first_empty)[:] = [7 + i for i in range(n)]
        return script['rc']

    lib = types.SimpleNamespace(dm_signal_event_stats_device=event_device, dm_signal_move_stats_device=move_device,
                                dm_signal_event_stats_batch=event_batch, dm_last_error=lambda: b'scripted failure')
    monkeypatch.setattr(_lib, 'load', lambda: lib)
    monkeypatch.setattr(model, 'PinnedArray', _Pinned)
    monkeypatch.setattr(dmsignal, 'SignalNormalizer', lambda device: handle)
    requests, answers, results, pool = queue.Queue(), [queue.Queue()], sigserver.SignalResults(), _Pool()
    stats = {k: 0.0 for k in ('signal_server', 'signal_server_call', 'signal_server_copy', 'signal_requests', 'signal_samples', 'signal_events',
                               'signal_move_requests', 'signal_move_bytes')}
    th = threading.Thread(target=sigserver.signal_server, args=(requests, answers, 0, stats, results, pool), daemon=True)
    th.start()
    norm = sigserver.RemoteSignalNormalizer(0, str(tmp_path), requests, answers[0])

    def stop():
        requests.put(None)
        th.join(timeout=10)
        assert not th.is_alive()

    yield types.SimpleNamespace(norm=norm, script=script, calls=calls, pool=pool, results=results, answers=answers[0], stats=stats, handle=handle,
                                requests=requests, stop=stop, thread=th)
    if th.is_alive():
        stop()
    norm.close()


def _reads(n=3, samples=300, seed=1):
    rng = np.random.default_rng(seed)
    raws = [rng.integers(300, 900, samples + 7 * i).astype(np.int16) for i in range(n)]
    lens = [rng.integers(3, 12, samples // 10).astype(np.uint64) for _ in range(n)]
    starts = [np.concatenate([[5], 5 + np.cumsum(ln)[:-1]]).astype(np.uint64) for ln in lens]
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return raws, off(raws), np.concatenate(starts), np.concatenate(lens), off(lens), np.array([len(x) for x in lens], np.int64)


def _post(s, with_fb=False):
    raws, raw_off, st, ln, ev_off, fe = _reads()
    fb = (np.ones(len(st), np.float32), np.ones(len(st), np.float32)) if with_fb else (None, None)
    return s.norm.post_arrays(raws, raw_off, st, ln, ev_off, fe, *fb), raw_off, ev_off, fe


def _post_move(s):
    raws, raw_off, _, _, ev_off, _ = _reads()
    moves = [np.ones(len(r) // 2, np.uint8) for r in raws]
    mv_off = np.concatenate([[0], np.cumsum([len(m) for m in moves])]).astype(np.int64)
    first = np.array([3, 0, 17], np.int64)
    return s.norm.post_move(raws, raw_off, moves, mv_off, first, ev_off), raw_off, mv_off, first, ev_off


def test_resident_request_registers_its_block_with_the_flags(server):
    s = server
    s.script['flags'] = 1
    key, raw_off, ev_off, fe = _post(s, with_fb=True)
    blk, flags, err = s.results.take(key, timeout=10)
    assert err is None and flags == 1 and blk is s.pool.taken[0] and blk.nbytes == 12 * int(ev_off[-1])
    assert s.pool.given == [] and len(s.pool.taken) == 1                   # registered: not given back
    assert s.answers.get(timeout=10) == ('ack', 1, None) and s.answers.empty()
    kind, h, n, c_raw_off, c_ev_off, c_fe, has_fb, ptr = s.calls[0]
    assert (kind, h, n, has_fb, ptr) == ('event', 1234, 3, True, blk.ptr)      # the copied inputs are the posted ones, the output is the block
    assert np.array_equal(c_raw_off, raw_off) and np.array_equal(c_ev_off, ev_off) and np.array_equal(c_fe, fe)
    s.stop()
    assert s.stats['signal_requests'] == 1 and s.stats['signal_samples'] == raw_off[-1] and s.stats['signal_events'] == ev_off[-1]
    assert s.stats['signal_move_requests'] == 0 and s.stats['signal_server_copy'] > 0 and s.stats['signal_server_call'] > 0


def test_resident_request_whose_call_fails_gives_its_block_back(server):
    s = server
    s.script['rc'] = 5
    key = _post(s)[0]
    blk, flags, err = s.results.take(key, timeout=10)
    assert blk is None and flags == 0 and err == 'signal stage: scripted failure'
    assert s.answers.get(timeout=10) == ('ack', 1, None)
    s.stop()
    assert len(s.pool.taken) == 1 and s.pool.given == s.pool.taken and s.answers.empty()
    assert s.stats['signal_requests'] == 1


def test_move_request_and_a_move_table_the_device_fails(server):
    s = server
    key, raw_off, mv_off, first, ev_off = _post_move(s)
    blk, flags, err = s.results.take(key, timeout=10)
    assert err is None and blk is s.pool.taken[0] and s.pool.given == []
    kind, h, n, c_raw_off, c_mv_off, c_first, ptr = s.calls[0]
    assert (kind, h, n, ptr) == ('move', 1234, 3, blk.ptr)
    assert np.array_equal(c_raw_off, raw_off) and np.array_equal(c_mv_off, mv_off) and np.array_equal(c_first, first)
    s.script['status'] = [0, 3, 1]
    key2 = _post_move(s)[0]
    blk2, flags2, err2 = s.results.take(key2, timeout=10)
    assert blk2 is None and err2 == 'signal stage: the device fails 2 move tables that dm_move_events passed'
    s.stop()
    assert len(s.pool.taken) == 2 and s.pool.given == [s.pool.taken[1]]
    assert [s.answers.get(timeout=10) for _ in range(2)] == [('ack', 1, None), ('ack', 2, None)] and s.answers.empty()
    assert s.stats['signal_move_requests'] == 2 and s.stats['signal_move_bytes'] == 2 * mv_off[-1] and s.stats['signal_requests'] == 2


def test_request_naming_a_missing_file_acks_once_and_the_thread_goes_on(server):
    s = server
    s.requests.put(('res', 0, s.norm.path + '_nowhere', 4096, 3, 100, 30, 9, False))
    blk, flags, err = s.results.take((0, 9), timeout=10)
    assert blk is None and err.startswith('signal server: ') and 'FileNotFoundError' in err
    assert s.answers.get(timeout=10) == ('ack', 9, None) and s.answers.empty()
    assert s.pool.taken == [] and s.pool.given == []                        # it failed before it took a block
    key = _post(s)[0]                                                       # the thread serves the next request
    blk, flags, err = s.results.take(key, timeout=10)
    assert err is None and blk is s.pool.taken[0] and s.thread.is_alive()
    assert s.answers.get(timeout=10) == ('ack', 1, None)
    # the synchronous twin: the error text is the answer
    s.requests.put((0, s.norm.path + '_nowhere', 4096, 3, 100, 30))
    msg = s.answers.get(timeout=10)
    assert isinstance(msg, str) and msg.startswith('signal server: ') and s.thread.is_alive()


def test_synchronous_request_gets_its_outputs_behind_the_inputs(server):
    s = server
    raws, raw_off, st, ln, ev_off, _ = _reads()
    n_ev = int(ev_off[-1])
    mean, stdv, first_empty = s.norm.event_stats_arrays(raws, raw_off, st, ln, ev_off)
    assert np.array_equal(mean, 1.0 + np.arange(n_ev, dtype=np.float32)) and np.array_equal(stdv, 0.5 * np.arange(n_ev, dtype=np.float32))
    assert np.array_equal(first_empty, [7, 8, 9]) and s.answers.empty()
    o = sigserver._sig_layout(3, int(raw_off[-1]), n_ev)
    assert np.array_equal(np.frombuffer(s.norm.mm, np.int16, int(raw_off[-1]), o['raw']), np.concatenate(raws))      # the inputs are as they were
    assert s.calls[0][0] == 'batch' and np.array_equal(s.calls[0][3], raw_off) and s.pool.taken == []
    s.script['rc'] = 5
    with pytest.raises(_lib.DeepModHipError, match='scripted failure'):
        s.norm.event_stats_arrays(raws, raw_off, st, ln, ev_off)
    assert s.thread.is_alive()
    s.stop()
    assert s.stats['signal_requests'] == 1                                  # (the failed call is not counted)


def test_none_ends_the_thread_and_frees_what_it_held(server):
    s = server
    key = _post(s)[0]
    s.results.take(key, timeout=10)
    s.stop()
    assert s.handle.closed == 1 and len(_Pinned.made) == 1 and _Pinned.made[0].freed == 1
