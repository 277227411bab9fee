"""The signal stage of a streaming run across processes (deepmod_amd/stream.py has the overview of the path): the request layouts, the feeder-side
client (`RemoteSignalNormalizer`), the server thread of the GPU process (`signal_server`) and what it hands to the batch loop (`SignalResults`,
`DeviceBlockPool`)."""
from __future__ import annotations

import ctypes
import os
import threading
import time
from collections import namedtuple
from typing import Optional

import numpy as np

from .handover import _layout, map_file


# ---------------------------------------------------------------------------------------------
# signal server: feeder processes do not own a HIP context.  The signal statistics of a raw-container batch
# (dm_signal_event_stats_batch) are computed by a thread of the GPU process: the feeder writes the samples and event tables
# of its batch into a shared-memory request file and waits for the answer.  (Every feeder with its own context capped a
# GPU at ~8 feeders: beyond that the hardware queues are oversubscribed and the classifier's queue is time-sliced.)
# ---------------------------------------------------------------------------------------------
def _sig_layout(n: int, n_raw: int, n_ev: int):
    """byte offsets of [raw i16 | raw_off i64 | ev_off i64 | ev_start u64 | ev_length u64 || mean f32 | stdv f32 | norm6 f64 | first_empty i64]"""
    return _layout((('raw', 2 * n_raw), ('raw_off', 8 * (n + 1)), ('ev_off', 8 * (n + 1)), ('ev_start', 8 * n_ev), ('ev_length', 8 * n_ev), ('in_end', 0),
                    ('mean', 4 * n_ev), ('stdv', 4 * n_ev), ('norm6', 48 * n), ('first_empty', 8 * n)))


def _sig_layout_res(n: int, n_raw: int, n_ev: int, with_fb: bool):
    """request of the resident form: [raw i16 | raw_off i64 | ev_off i64 | ev_start u64 | ev_length u64 | first_empty i64 | fb_mean f32 | fb_stdv f32]
    (the last two only when some read of the batch has an empty event) - inputs only: the statistics stay on the device"""
    return _layout((('raw', 2 * n_raw), ('raw_off', 8 * (n + 1)), ('ev_off', 8 * (n + 1)), ('ev_start', 8 * n_ev), ('ev_length', 8 * n_ev),
                    ('first_empty', 8 * n), ('fb_mean', 4 * n_ev if with_fb else 0), ('fb_stdv', 4 * n_ev if with_fb else 0)))


def _sig_layout_move(n: int, n_raw: int, n_mv: int):
    """request of the resident form for move reads: [raw i16 | raw_off i64 | ev_off i64 | mv_off i64 | first i64 | move u8] - inputs only"""
    return _layout((('raw', 2 * n_raw), ('raw_off', 8 * (n + 1)), ('ev_off', 8 * (n + 1)), ('mv_off', 8 * (n + 1)), ('first', 8 * n), ('move', n_mv)))


_SIG_DTYPES = {'raw': np.int16, 'move': np.uint8, 'ev_start': np.uint64, 'ev_length': np.uint64, 'fb_mean': np.float32, 'fb_stdv': np.float32}   # other inputs: int64


def _map_request_file(path: str, nbytes: int, old=None):
    """Create or grow a request file and map it -> (mapping, size): 1.5 x what is asked for, 4 MB at least; `old`, the mapping it replaces, is closed."""
    if old is not None:
        old.close()
    size = max(1 << 22, int(nbytes * 1.5))
    return map_file(path, size, os.O_CREAT), size


class SignalResults:
    """GPU process: what the signal server threads hand to the batch loop - per resident request (feeder, number) the device block of its
    statistics, the range flag of dm_signal_event_stats_device and an error text.  The server registers a result when its call has returned (the block
    is then complete: nothing the batch loop queues afterwards needs a cross-stream wait); the loop takes it when the batch that names it arrives."""

    def __init__(self):
        self._cv = threading.Condition()
        self._done = {}

    def put(self, key, block, flags: int = 0, err: Optional[str] = None):
        with self._cv:
            self._done[tuple(key)] = (block, flags, err)
            self._cv.notify_all()

    def take(self, key, timeout: float = 300.0):
        key = tuple(key)
        end = time.perf_counter() + timeout
        with self._cv:
            while key not in self._done:
                left = end - time.perf_counter()
                if left <= 0:
                    raise RuntimeError('the signal stage never answered request %r' % (key,))
                self._cv.wait(left)
            return self._done.pop(key)

    def pending(self):
        with self._cv:
            return list(self._done)


class DeviceBlockPool:
    """Grow-only device blocks for the statistics of resident signal requests: taken by a server thread, given back by the batch loop once the launches
    that read a block have finished (its staging set's marker has passed)."""

    def __init__(self, device: int):
        self.device = device
        self._lock = threading.Lock()
        self._free = []
        self.allocated = 0

    def take(self, nbytes: int):
        from . import model as dm
        with self._lock:
            best = None
            for i, b in enumerate(self._free):
                if b.nbytes >= nbytes and (best is None or b.nbytes < self._free[best].nbytes):
                    best = i
            if best is not None:
                return self._free.pop(best)
        blk = dm.DeviceArray((int(nbytes * 1.25) + 4096,), np.uint8, self.device)
        with self._lock:
            self.allocated += 1
        return blk

    def give(self, blk):
        if blk is not None:
            with self._lock:
                self._free.append(blk)

    def close(self):
        with self._lock:
            blocks, self._free = self._free, []
        for b in blocks:
            b.free()


class RemoteSignalNormalizer:
    """Feeder-process side of the signal server: the interface of signal.SignalNormalizer that the raw path uses."""

    def __init__(self, wid: int, shm_dir: str, requests, answers):
        self.wid, self.requests, self.answers = wid, requests, answers
        self.path = os.path.join(shm_dir, 'sig_%d' % wid)
        self.mm = None
        self.size = 0
        self._posted = 0                   # resident requests posted so far
        self._acked = set()                # ... whose request file the server has copied (it may be written again)
        self._res_files = [None, None]     # (mapping, size, path) of the two request files of the resident form

    # ---- resident form: post and go on ----
    def _request_file(self, seq: int, nbytes: int):
        """the request file of resident request `seq` (the file of request seq - 2, which the server must have copied), at least nbytes large"""
        while seq - 2 > 0 and (seq - 2) not in self._acked:
            self._take_answer(block=True)
        self._acked.discard(seq - 2)
        slot = seq % 2
        cur = self._res_files[slot]
        if cur is None or cur[1] < nbytes:
            path = self.path + '_r%d' % slot
            cur = self._res_files[slot] = _map_request_file(path, nbytes, cur and cur[0]) + (path,)
        return cur

    def _write(self, mm, o, **fields):
        """Fill a request: every named array goes to its offset of layout `o` - a list of parts is concatenated straight into the mapping, None is left out."""
        for name, a in fields.items():
            if a is None:
                continue
            parts = [np.asarray(p) for p in a] if isinstance(a, (list, tuple)) else None
            view = np.frombuffer(mm, _SIG_DTYPES.get(name, np.int64), len(a) if parts is None else sum(len(p) for p in parts), o[name])
            if o[name] + view.nbytes > min([v for v in o.values() if v > o[name]] or [o['end']]):
                raise ValueError('signal request: %s is larger than the layout says' % name)
            if parts is None:
                view[:] = a
            elif len(view):
                np.concatenate(parts, out=view, casting='same_kind')

    def post_move(self, raw_parts, raw_off, move_parts, mv_off, first, ev_off):
        """post_arrays for move reads (dm_signal_move_stats_device): the move tables travel instead of (start, length) tables - the server's kernels
        segment them.  ev_off: the cumulative Fastq lengths, the event count every read must have (the feeder has checked it: dm_move_events)."""
        seq = self._posted = self._posted + 1
        n, n_raw, n_ev, n_mv = len(raw_off) - 1, int(raw_off[-1]), int(ev_off[-1]), int(mv_off[-1])
        o = _sig_layout_move(n, n_raw, n_mv)
        mm, size, path = self._request_file(seq, o['end'])
        self._write(mm, o, raw=list(raw_parts), raw_off=raw_off, ev_off=ev_off, mv_off=mv_off, first=first, move=list(move_parts))
        self.requests.put(('mov', self.wid, path, size, n, n_raw, n_ev, seq, n_mv))
        return (self.wid, seq)

    def post_arrays(self, raw_parts, raw_off, ev_start, ev_length, ev_off, first_empty, fb_mean=None, fb_stdv=None):
        """Write a request of the resident form (dm_signal_event_stats_device) into one of this feeder's two request files and queue it: no wait for the
        statistics - they stay on the device, the GPU process finds them under the returned (feeder, number) when the batch arrives.  The only wait is
        for the file itself: request k reuses the file of request k - 2, which the server must have copied into its page-locked memory (its
        acknowledgement; usually long there)."""
        seq = self._posted = self._posted + 1
        n, n_raw, n_ev = len(raw_off) - 1, int(raw_off[-1]), int(ev_off[-1])
        with_fb = fb_mean is not None and fb_stdv is not None
        o = _sig_layout_res(n, n_raw, n_ev, with_fb)
        mm, size, path = self._request_file(seq, o['end'])
        self._write(mm, o, raw=list(raw_parts), raw_off=raw_off, ev_off=ev_off, ev_start=ev_start, ev_length=ev_length, first_empty=first_empty,
                    fb_mean=fb_mean if with_fb else None, fb_stdv=fb_stdv if with_fb else None)
        self.requests.put(('res', self.wid, path, size, n, n_raw, n_ev, seq, with_fb))
        return (self.wid, seq)

    def _take_answer(self, block: bool = True):
        """One message from the server: ('ack', number, error) of a resident request, or the answer (None / error text) of a synchronous one."""
        from . import _lib
        msg = self.answers.get() if block else self.answers.get_nowait()
        if isinstance(msg, tuple) and msg and msg[0] == 'ack':
            if msg[2] is not None:
                raise _lib.DeepModHipError(msg[2])
            self._acked.add(msg[1])
            return 'ack'
        return ('answer', msg)

    def _wait_answer(self):
        while True:
            got = self._take_answer(block=True)
            if got != 'ack':
                return got[1]

    def _ensure(self, nbytes: int):
        if nbytes > self.size:
            self.mm, self.size = _map_request_file(self.path, nbytes, self.mm)

    def _ask(self, n: int, raw_off, ev_off, **columns):
        """One synchronous request (raw, ev_start, ev_length in `columns`) -> (layout, mapping, events): the server's answer is in the mapping."""
        from . import _lib
        n_raw, n_ev = int(raw_off[-1]), int(ev_off[-1])
        o = _sig_layout(n, n_raw, n_ev)
        self._ensure(o['end'])
        self._write(self.mm, o, raw_off=raw_off, ev_off=ev_off, **columns)
        self.requests.put((self.wid, self.path, self.size, n, n_raw, n_ev))
        err = self._wait_answer()
        if err is not None:
            raise _lib.DeepModHipError(err)
        return o, self.mm, n_ev

    def event_stats_batch(self, reads):
        if not reads:
            return []
        n = len(reads)
        raw_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.int64)
        ev_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.int64)
        o, mm, n_ev = self._ask(n, raw_off, ev_off, raw=[r[0] for r in reads], ev_start=[r[1] for r in reads], ev_length=[r[2] for r in reads])
        mean = np.frombuffer(mm, np.float32, n_ev, o['mean']).copy()
        stdv = np.frombuffer(mm, np.float32, n_ev, o['stdv']).copy()
        norm6 = np.frombuffer(mm, np.float64, 6 * n, o['norm6']).reshape(n, 6)
        first_empty = np.frombuffer(mm, np.int64, n, o['first_empty'])
        keys = ("mshift", "mscale", "read_med", "read_mad", "lower_lim", "upper_lim")
        return [(mean[ev_off[i]:ev_off[i + 1]], stdv[ev_off[i]:ev_off[i + 1]], dict(zip(keys, norm6[i].tolist())), int(first_empty[i]))
                for i in range(n)]

    def event_stats_arrays(self, raw_parts, raw_off, ev_start, ev_length, ev_off):
        """Same request as event_stats_batch, from arrays that are already back to back (see signal.SignalNormalizer.event_stats_arrays)."""
        n = len(raw_off) - 1
        o, mm, n_ev = self._ask(n, raw_off, ev_off, raw=list(raw_parts), ev_start=ev_start, ev_length=ev_length)
        return (np.frombuffer(mm, np.float32, n_ev, o['mean']).copy(), np.frombuffer(mm, np.float32, n_ev, o['stdv']).copy(),
                np.frombuffer(mm, np.int64, n, o['first_empty']).copy())

    def event_stats(self, raw, ev_start, ev_length, want_signal: bool = False):
        if want_signal:
            raise ValueError('the signal server returns event statistics only')
        mean, stdv, norm, first_empty = self.event_stats_batch([(raw, ev_start, ev_length)])[0]
        return mean, stdv, norm, first_empty, None

    def close(self):
        if self.mm is not None:
            self.mm.close()
            self.mm = None
        for cur in self._res_files:
            if cur is not None:
                cur[0].close()
        self._res_files = [None, None]


# a request as the server works on it: kind 'sync', 'res' or 'mov'; size: of the request file; seq: the number of a resident request;
# with_fb ('res'): the fall-back values are in it; n_mv ('mov'): the bytes of its move tables
_Request = namedtuple('_Request', 'kind wid path size n n_raw n_ev seq with_fb n_mv', defaults=(None, False, 0))


def _decode(req) -> _Request:
    """a wire tuple (signal_server's docstring) -> the record"""
    if req[0] == 'mov':
        return _Request(*req[:8], n_mv=req[8])
    return _Request(*req) if req[0] == 'res' else _Request('sync', *req)


def _request_layout(rq: _Request):
    if rq.kind == 'mov':
        return _sig_layout_move(rq.n, rq.n_raw, rq.n_mv)
    return _sig_layout_res(rq.n, rq.n_raw, rq.n_ev, rq.with_fb) if rq.kind == 'res' else _sig_layout(rq.n, rq.n_raw, rq.n_ev)


class _SignalServer:
    """What one server thread keeps between requests: its dm_signal handle, the mappings of the request files it has seen, its page-locked buffer."""

    def __init__(self, answers, device: int, stats, results, blocks):
        from . import _lib
        self.answers, self.device, self.stats, self.results, self.blocks = answers, device, stats, results, blocks
        self.norm = None           # its dm_signal handle is made for the first request: a run of feature containers never needs one, and
        self.lib = _lib.load()     # a raw run's first request arrives after the model is on the device (no three-way race for the HIP start-up)
        self.maps = {}
        self.pinned = None

    def copy_in(self, rq: _Request):
        """The inputs of a request, from its file into page-locked memory -> (layout, mapping of the file, view of the page-locked bytes)"""
        from . import model as dm, signal as dmsignal
        if self.norm is None:
            self.norm = dmsignal.SignalNormalizer(self.device)
        if self.maps.get(rq.path, (None, 0))[1] != rq.size:
            if rq.path in self.maps:
                self.maps[rq.path][0].close()
            self.maps[rq.path] = (map_file(rq.path, rq.size), rq.size)
        mm = self.maps[rq.path][0]
        o = _request_layout(rq)
        n_in = o.get('in_end', o['end'])          # a resident request holds inputs only
        if self.pinned is None or self.pinned.nbytes < o['end']:
            if self.pinned is not None:
                self.pinned.free()
            self.pinned = dm.PinnedArray(int(o['end'] * 1.5) + 4096, self.device)
        pv = self.pinned.view(np.uint8, o['end'])
        pv[:n_in] = np.frombuffer(mm, np.uint8, n_in)
        return o, mm, pv

    def resident_call(self, rq: _Request, o, blk, t0: float, t1: float) -> bool:
        """The statistics of a resident request into `blk`, registered in `results` -> True if the block went with them"""
        from . import _lib
        lib, h, base, key = self.lib, self.norm._h, self.pinned.ptr, (rq.wid, rq.seq)
        flags = ctypes.c_int32(0)
        bad = 0
        if rq.kind == 'mov':
            status = np.empty(rq.n, np.int32)
            rc = lib.dm_signal_move_stats_device(h, rq.n, base + o['raw'], base + o['raw_off'], base + o['move'], base + o['mv_off'],
                                                 base + o['first'], base + o['ev_off'], blk.ptr, status.ctypes.data, None, ctypes.byref(flags))
            bad = int(np.count_nonzero(status)) if rc == 0 else 0
        else:
            rc = lib.dm_signal_event_stats_device(h, rq.n, base + o['raw'], base + o['raw_off'], base + o['ev_start'], base + o['ev_length'],
                                                  base + o['ev_off'], base + o['first_empty'], (base + o['fb_mean']) if rq.with_fb else None,
                                                  (base + o['fb_stdv']) if rq.with_fb else None, blk.ptr, None, ctypes.byref(flags))
        if self.stats is not None:
            self.stats['signal_server_call'] += time.perf_counter() - t1
            self.stats['signal_server_copy'] += t1 - t0
        if rc != 0:
            self.results.put(key, None, 0, 'signal stage: ' + _lib.last_error())
        elif bad:           # the feeder posts only reads that passed dm_move_events: the device disagrees with the host definition
            self.results.put(key, None, 0, 'signal stage: the device fails %d move tables that dm_move_events passed' % bad)
        else:
            self.results.put(key, blk, int(flags.value), None)
        return rc == 0 and not bad

    def synchronous_call(self, rq: _Request, o, mm, pv, t1: float) -> bool:
        """The statistics of a synchronous request back into its file; the feeder gets None or the error text -> False if the call failed"""
        from . import _lib
        base = self.pinned.ptr
        rc = self.lib.dm_signal_event_stats_batch(self.norm._h, rq.n, base + o['raw'], base + o['raw_off'], base + o['ev_start'], base + o['ev_length'],
                                                  base + o['ev_off'], base + o['mean'], base + o['stdv'], base + o['norm6'], base + o['first_empty'])
        if self.stats is not None:
            self.stats['signal_server_call'] += time.perf_counter() - t1
        if rc != 0:
            self.answers[rq.wid].put(_lib.last_error())
            return False
        np.frombuffer(mm, np.uint8, o['end'] - o['in_end'], o['in_end'])[:] = pv[o['in_end']:]
        self.answers[rq.wid].put(None)
        return True

    def serve(self, rq: _Request) -> None:
        """One request.  Whatever fails, the feeder and the batch loop hear of it and the thread goes on: the feeder turns it into a per-read
        failure / the batch loop fails the run."""
        t0 = time.perf_counter()
        acked, blk, counted = False, None, True
        try:
            o, mm, pv = self.copy_in(rq)
            t1 = time.perf_counter()
            if rq.kind != 'sync':
                self.answers[rq.wid].put(('ack', rq.seq, None))          # the request file is free again
                acked = True
                blk = self.blocks.take(12 * max(rq.n_ev, 1))
                if self.resident_call(rq, o, blk, t0, t1):
                    blk = None              # the batch loop owns it now
            else:
                counted = self.synchronous_call(rq, o, mm, pv, t1)      # (a call that failed is not counted below: so it has always been)
        except Exception as exc:
            if rq.kind != 'sync':
                if not acked:
                    self.answers[rq.wid].put(('ack', rq.seq, None))
                self.results.put((rq.wid, rq.seq), None, 0, 'signal server: %r' % (exc,))
            else:
                self.answers[rq.wid].put('signal server: %r' % (exc,))
        finally:
            if blk is not None:             # a request that failed after taking its block
                self.blocks.give(blk)
        if counted and self.stats is not None:
            self.count(rq, t0)

    def count(self, rq: _Request, t0: float) -> None:
        stats = self.stats
        stats['signal_server'] += time.perf_counter() - t0
        stats['signal_requests'] += 1
        stats['signal_samples'] += rq.n_raw
        stats['signal_events'] += rq.n_ev
        if rq.kind == 'mov':
            stats['signal_move_requests'] += 1
            stats['signal_move_bytes'] += rq.n_mv

    def close(self) -> None:
        for mm, _ in self.maps.values():
            mm.close()
        if self.pinned is not None:
            self.pinned.free()
        if self.norm is not None:
            self.norm.close()


def signal_server(requests, answers, device: int, stats=None, results: Optional[SignalResults] = None, blocks: Optional[DeviceBlockPool] = None):
    """Thread body in the GPU process: requests until None.
      (wid, path, file size, n, n_raw, n_ev)                          synchronous form: answers[wid] gets None or an error text; the statistics
                                                                       go back into the request file;
      ('res', wid, path, file size, n, n_raw, n_ev, number, with_fb)  resident form (round 6): answers[wid] gets ('ack', number, error) as soon
                                                                       as the request file has been copied (the feeder may write it again), the
                                                                       statistics go into a device block registered in `results` under (wid, number);
      ('mov', wid, path, file size, n, n_raw, n_ev, number, n_mv)     resident form for move reads (detect --move): move tables instead of event
                                                                       tables (dm_signal_move_stats_device), answered like 'res'.
    Inputs are copied to page-locked memory (uploads from the shared-memory mapping itself are slow)."""
    server = _SignalServer(answers, device, stats, results, blocks)
    try:
        while True:
            req = requests.get()
            if req is None:
                return
            server.serve(_decode(req))
    finally:
        server.close()


