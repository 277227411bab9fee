"""GPU (-m gpu): every entry point of the signal stage against the numpy oracle on the edge fixtures (tests/golden/host_signal_edges.npz,
pinned to the reference's own functions by test_signal.py::test_oracle_matches_reference_edge_golden).

The batched and resident forms keep one 65,536-entry value table per read slot of the handle and reuse it across calls, so every test first
runs a POISONING batch through its handle: wide reads over the whole int16 range, each with its own normalisation, that write every entry of
every slot the edge batch will use.  An entry the edge batch forgets to write then holds a wrong value for certain, not by luck.

Bit for bit: the six norm values with ==, mean / stdv as float32 bit patterns after the reference's cut rule (myDetect.py:332-343)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import signal_oracle
from test_signal import EDGE_CASES, EVENT_DTYPE, _apply_reference_rule, _same_f32

pytestmark = pytest.mark.gpu

NORM_KEYS = ("mshift", "mscale", "read_med", "read_mad", "lower_lim", "upper_lim")


@pytest.fixture(scope="module")
def edges():
    """name -> (raw, start, length) of every edge case"""
    z = np.load(os.path.join(GOLDEN, "host_signal_edges.npz"))
    return {n: (z[n + '.raw'], z[n + '.start'], z[n + '.length']) for n in EDGE_CASES}


_ORACLE = {}


def _oracle(key, raw, start, length, want_signal=False):
    """-> (mean, stdv, norm dict, first_empty) of the oracle, cached per key (+ the normalised signal if want_signal)"""
    if key not in _ORACLE:
        ev = np.zeros(len(start), dtype=EVENT_DTYPE)
        ev['start'], ev['length'] = start, length
        sig, norm = signal_oracle.mnormalized(raw, ev)
        mean, stdv, first_empty = signal_oracle.event_stats(sig, ev)
        _ORACLE[key] = (mean, stdv, norm, first_empty, sig if key in EDGE_CASES else None)
    return _ORACLE[key] if want_signal else _ORACLE[key][:4]


def _filler(i):
    """an ordinary read with an odd sample count (so the reads after it start off the 8-sample grid) and contiguous events"""
    rng = np.random.default_rng(1000 + i)
    n = 301 + 2 * int(rng.integers(0, 200))
    raw = np.round(rng.normal(400 + 7 * (i % 50), 30 + (i % 13), n)).astype(np.int16)
    length = np.maximum(1, rng.geometric(1 / 9.0, n // 9 + 4)).astype(np.uint64)
    start = (int(rng.integers(0, 20)) + np.concatenate([[0], np.cumsum(length[:-1])])).astype(np.uint64)
    keep = start + length <= n
    return ('filler%d' % i, raw, start[keep].copy(), length[keep].copy())


def _poison_reads(n_reads, seed, n=2000):
    """wide reads: every one holds -32768 and 32767 inside its covered slice (its table is written over the whole int16 range), and a
    normalisation of its own - a uniform spread of its own width (2,000 - 30,000) around a centre of its own (|c| < 2,000).  Its table maps
    every value below 1,000 to |v| < 3, where an edge read clips the open pore and the tail above its strand to its upper limit (~ +5)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_reads):
        w = int(rng.integers(2000, 30000))
        c = int(rng.integers(-2000, 2000))
        raw = np.clip(rng.integers(c - w, c + w, n), -32768, 32767).astype(np.int16)
        raw[[5, 9]] = -32768, 32767
        length = np.full(n // 200, 200, np.uint64)
        start = (np.arange(n // 200) * 200).astype(np.uint64)
        out.append(('poison%d_%d' % (seed, i), raw, start, length))
    return out


def _edge_layout(edges, n_reads, order=1, skip=()):
    """n_reads reads: the edge cases (in `order`, without `skip`), each behind a filler read of odd length, then more fillers"""
    names = [n for n in EDGE_CASES[::order] if n not in skip]
    reads, k = [], 0
    while len(reads) < n_reads:
        reads.append(_filler(k))
        k += 1
        if names and len(reads) < n_reads:
            nm = names.pop(0)
            reads.append((nm,) + tuple(edges[nm]))
    return reads


class Mismatch:
    """collects per-read differences so one assertion names every case that differs and by how many events"""

    def __init__(self, what):
        self.what, self.bad = what, []

    def check(self, name, mean, stdv, norm, first_empty, want, rule=True):
        wm, ws, wn, wf = want
        msg = []
        if first_empty != wf:
            msg.append('first_empty %d != %d' % (first_empty, wf))
        if norm is not None:
            diff = [k for k in NORM_KEYS if not (norm[k] == wn[k])]
            if diff:
                msg.append('norm ' + ','.join(diff))
        if rule:
            ev = np.zeros(len(wm), dtype=EVENT_DTYPE)
            got, exp = _apply_reference_rule(ev, mean, stdv, first_empty), _apply_reference_rule(ev, wm, ws, wf)
            gm, gs, em, es = got['mean'], got['stdv'], exp['mean'], exp['stdv']
        else:
            gm, gs, em, es = mean, stdv, wm, ws
        if len(gm) != len(em):
            msg.append('%d events kept != %d' % (len(gm), len(em)))
        else:
            n_bad = int(np.count_nonzero((np.asarray(gm, np.float32).view(np.uint32) != np.asarray(em, np.float32).view(np.uint32)) |
                                         (np.asarray(gs, np.float32).view(np.uint32) != np.asarray(es, np.float32).view(np.uint32))))
            if n_bad:
                msg.append('%d of %d events differ' % (n_bad, len(em)))
        if msg:
            self.bad.append('%s: %s' % (name, '; '.join(msg)))

    def done(self):
        assert not self.bad, '%s: %d reads differ from the oracle:\n  %s' % (self.what, len(self.bad), '\n  '.join(self.bad))


def _check_batch(nz, reads, what):
    """the batched call on `reads` against the oracle"""
    res = nz.event_stats_batch([r[1:] for r in reads])
    mm = Mismatch(what)
    for (name, raw, st, ln), (mean, stdv, norm, fe) in zip(reads, res):
        mm.check(name, mean, stdv, norm, fe, _oracle(name, raw, st, ln))
    mm.done()


def _batch_arrays(reads):
    raw_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in reads])]).astype(np.int64)
    ev_off = np.concatenate([[0], np.cumsum([len(r[2]) for r in reads])]).astype(np.int64)
    return (np.concatenate([r[1] for r in reads]), raw_off, np.concatenate([r[2] for r in reads]), np.concatenate([r[3] for r in reads]), ev_off)


def test_single_read_call_on_edges_host_and_device_signal(edges):
    """dm_signal_event_stats writes all 65,536 entries of its table every call: with the signal on the host and on the device"""
    from deepmod_amd import _lib, signal
    from deepmod_amd.model import DeviceArray
    nz = signal.SignalNormalizer(0)
    lib = _lib.load()
    for name, raw, st, ln in _poison_reads(1, 7):
        nz.event_stats(raw, st, ln)
    host, dev = Mismatch('single-read call, host signal'), Mismatch('single-read call, device signal')
    for name in EDGE_CASES:
        raw, st, ln = edges[name]
        *want, wsig = _oracle(name, raw, st, ln, want_signal=True)
        mean, stdv, norm, fe, sig = nz.event_stats(raw, st, ln, want_signal=True)
        host.check(name, mean, stdv, norm, fe, want)
        if not np.array_equal(sig, wsig):
            host.bad.append('%s: normalised signal differs' % name)
        d_raw = DeviceArray.from_host(np.ascontiguousarray(raw), 0)
        m2, s2, n6, fe2 = np.empty(len(st), np.float32), np.empty(len(st), np.float32), np.empty(6, np.float64), ctypes.c_int64(0)
        st_c, ln_c = np.ascontiguousarray(st, np.uint64), np.ascontiguousarray(ln, np.uint64)
        _lib.check(lib.dm_signal_event_stats(nz._h, d_raw.ptr, len(raw), st_c.ctypes.data, ln_c.ctypes.data, len(st), m2.ctypes.data, s2.ctypes.data,
                                             n6.ctypes.data, ctypes.byref(fe2), None))
        d_raw.free()
        dev.check(name, m2, s2, dict(zip(NORM_KEYS, n6.tolist())), int(fe2.value), want)
    nz.close()
    host.done()
    dev.done()


@pytest.mark.parametrize("host_norm", [False, True], ids=["device_order_statistics", "host_order_statistics"])
def test_batched_call_on_edges_after_poisoning(edges, monkeypatch, host_norm):
    """dm_signal_event_stats_batch with device order statistics and with DEEPMOD_SIGNAL_HOST_NORM=1, on a handle whose table slots hold another
    normalisation over the whole int16 range; the edge reads in two orders (each behind an odd-length read: raw_off off the 8-sample grid).  The first
    batch leaves out distinct_4097, so that every read takes the device order statistics; the second has it, and the batch is handed to the host."""
    from deepmod_amd import signal
    if host_norm:
        monkeypatch.setenv('DEEPMOD_SIGNAL_HOST_NORM', '1')
    else:
        monkeypatch.delenv('DEEPMOD_SIGNAL_HOST_NORM', raising=False)
    nz = signal.SignalNormalizer(0)
    for order, skip in ((1, ('distinct_4097',)), (-1, ())):
        reads = _edge_layout(edges, 2 * len(EDGE_CASES) + 1, order, skip)
        assert sum(int(o) % 8 != 0 for o in _batch_arrays(reads)[1][1:-1]) >= len(reads) // 2
        nz.event_stats_batch([r[1:] for r in _poison_reads(len(reads), 11 + order)])
        _check_batch(nz, reads, 'batched call (%s, order %d)' % ('host' if host_norm else 'device', order))
    nz.close()


def test_resident_form_on_edges_after_poisoning(edges):
    """dm_signal_plan_batch + dm_signal_event_stats_device: the block read back, fall-back values merged behind each read's first empty event; without
    distinct_4097 (device order statistics) and with it (the batch handed to the host order statistics)"""
    from deepmod_amd import signal
    from deepmod_amd.model import DeviceArray
    nz = signal.SignalNormalizer(0)
    mm = Mismatch('resident form')
    for order, skip in ((1, ('distinct_4097',)), (-1, ())):
        reads = _edge_layout(edges, 2 * len(EDGE_CASES) + 1, order, skip)
        raw, raw_off, st, ln, ev_off = _batch_arrays(reads)
        n_ev = int(ev_off[-1])
        rng = np.random.default_rng(3)
        fb_mean, fb_stdv = rng.normal(0, 1, n_ev).astype(np.float32), rng.random(n_ev).astype(np.float32)
        blk = DeviceArray((n_ev, 3), np.float32, 0)
        p_raw, p_ro, p_st, p_ln, p_eo = _batch_arrays(_poison_reads(len(reads), 21 + order))
        p_blk = DeviceArray((int(p_eo[-1]), 3), np.float32, 0)
        nz.event_stats_device(p_raw, p_ro, p_st, p_ln, p_eo, p_blk.ptr)
        fe, flag = nz.event_stats_device(raw, raw_off, st, ln, ev_off, blk.ptr, fb_mean, fb_stdv)
        got = blk.to_host()
        for r, (name, rr, rs, rl) in enumerate(reads):
            e0, e1 = int(ev_off[r]), int(ev_off[r + 1])
            wm, ws, wn, wf = _oracle(name, rr, rs, rl)
            want_mean, want_stdv = fb_mean[e0:e1].copy(), fb_stdv[e0:e1].copy()
            want_mean[:wf], want_stdv[:wf] = wm[:wf], ws[:wf]
            mm.check('%s (order %d)' % (name, order), got[e0:e1, 0], got[e0:e1, 1], None, int(fe[r]), (want_mean, want_stdv, wn, wf), rule=False)
            if not _same_f32(got[e0:e1, 2], rl.astype(np.float64).astype(np.float32)):
                mm.bad.append('%s: length column' % name)
        assert flag == 0                      # every statistic of this batch is inside the split-f16 kernels' range
        blk.free()
        p_blk.free()
    nz.close()
    mm.done()


def test_sp_param_batch_on_edges_after_poisoning(edges):
    """mnormalized_event_stats_batch: the m_event tables and norm dicts the command sees"""
    from deepmod_amd import signal
    nz = signal.SignalNormalizer(0)
    reads = _edge_layout(edges, 2 * len(EDGE_CASES) + 1, -1)
    nz.event_stats_batch([r[1:] for r in _poison_reads(len(reads), 31)])
    sps = []
    for name, raw, st, ln in reads:
        ev = np.zeros(len(st), dtype=EVENT_DTYPE)
        ev['start'], ev['length'] = st, ln
        sps.append({'raw_signals': raw, 'm_event': ev, 'mfile_path': name})
    errs = signal.mnormalized_event_stats_batch({}, sps, nz)
    assert errs == [None] * len(reads)
    mm = Mismatch('sp_param batch')
    for (name, raw, st, ln), sp in zip(reads, sps):
        wm, ws, wn, wf = _oracle(name, raw, st, ln)
        ev = np.zeros(len(st), dtype=EVENT_DTYPE)
        want = _apply_reference_rule(ev, wm, ws, wf)
        mm.check(name, sp['m_event']['mean'], sp['m_event']['stdv'], sp['norm'], wf, (want['mean'], want['stdv'], wn, wf), rule=False)
    nz.close()
    mm.done()


def test_handle_life_cycle_3_40_3_reads(edges):
    """one handle, batches of 3, 40 and 3 reads: the 40-read batch grows every per-read buffer (its poisoning batch is the first call on the new
    buffers and is checked too), the last batch runs on slots that held 40 reads' tables"""
    from deepmod_amd import signal
    nz = signal.SignalNormalizer(0)
    edge = lambda name: (name,) + tuple(edges[name])
    batches = [[_filler(90), edge('open_pore_a'), edge('overlap_tail')], _edge_layout(edges, 40, -1), [edge('open_pore_b'), _filler(91), edge('extreme_values')]]
    for step, reads in enumerate(batches):
        _check_batch(nz, _poison_reads(len(reads), 41 + step), 'poisoning batch %d of %d reads' % (step, len(reads)))
        _check_batch(nz, reads, 'batch %d of %d reads' % (step, len(reads)))
    nz.close()


def test_batch_of_4096_reads(edges):
    """the largest batch a call takes: 4,096 reads, the edge cases spread among small ordinary reads, after a poisoning batch as large"""
    from deepmod_amd import _lib, signal
    nz = signal.SignalNormalizer(0)
    nz.event_stats_batch([r[1:] for r in _poison_reads(4096, 51, n=600)])
    reads = _edge_layout(edges, 4096, skip=('distinct_4097',))      # (which would send the whole batch to the host order statistics)
    assert len(reads) == 4096 and sum(r[0] in EDGE_CASES for r in reads) == len(EDGE_CASES) - 1
    _check_batch(nz, reads, 'batch of 4,096 reads')
    with pytest.raises(_lib.DeepModHipError, match='at most 4096'):
        nz.event_stats_batch([r[1:] for r in reads] + [reads[0][1:]])
    nz.close()


def _small_read(i):
    """200 to 500 samples, contiguous events of 1 to ~30 samples from a small offset on"""
    rng = np.random.default_rng(7000 + i)
    n = 200 + int(rng.integers(0, 301))
    raw = np.round(rng.normal(450 + 11 * (i % 17), 25 + (i % 7), n)).astype(np.int16)
    length = np.maximum(1, rng.geometric(1 / 8.0, n // 8 + 4)).astype(np.uint64)
    start = (int(rng.integers(0, 12)) + np.concatenate([[0], np.cumsum(length[:-1])])).astype(np.uint64)
    keep = start + length <= n
    return raw, start[keep].copy(), length[keep].copy()


def _small_move_read(i):
    """the same sizes with a move table: -> (raw, move uint8[L], first, bases); every boundary's event starts inside the signal"""
    rng = np.random.default_rng(7500 + i)
    n = 200 + int(rng.integers(0, 301))
    raw = np.round(rng.normal(500 + 9 * i, 30, n)).astype(np.int16)
    first = int(rng.integers(0, 9))
    move = (rng.random((n - first) // 2) < 0.3).astype(np.uint8)
    return raw, move, first, 1 + int(move[1:].sum())


def test_one_handle_through_every_form_equals_fresh_handles():
    """One handle makes a single-read call, a host-table batch of 3 reads, a resident batch of 40, a move-table batch of 3 and the host-table batch
    again; every result is, byte for byte, what the same call returns on a handle of its own.  The paired tables of the handle (start | length,
    mean | stdv, the fall-back pair, the chunk triple) lie at a stride of the call, and the blocks they lie in were sized by other forms' calls."""
    from deepmod_amd import signal
    from deepmod_amd.model import DeviceArray
    three = [_small_read(i) for i in range(3)]
    forty = [_small_read(10 + i) for i in range(40)]
    r5, s5, l5 = forty[5]
    forty[5] = (r5, np.append(s5, np.uint64(len(r5))), np.append(l5, np.uint64(4)))          # an empty event: the fall-back values show behind it
    moved = [_small_move_read(i) for i in range(3)]

    def flat(res):
        return b''.join(np.ascontiguousarray(a).tobytes() for a in res)

    def single(nz):
        mean, stdv, norm, fe, _ = nz.event_stats(*three[1])
        return flat([mean, stdv, np.array(list(norm.values())), np.array([fe])])

    def host_batch(nz):
        return b''.join(flat([m, s, np.array(list(n.values())), np.array([f])]) for m, s, n, f in nz.event_stats_batch(three))

    def resident(nz):
        raw, raw_off, st, ln, ev_off = _batch_arrays([('r%d' % i,) + r for i, r in enumerate(forty)])
        n_ev = int(ev_off[-1])
        rng = np.random.default_rng(5)
        blk = DeviceArray((n_ev, 3), np.float32, 0)
        fe, flag = nz.event_stats_device(raw, raw_off, st, ln, ev_off, blk.ptr, rng.normal(0, 1, n_ev).astype(np.float32), rng.random(n_ev).astype(np.float32))
        got = blk.to_host()
        blk.free()
        assert fe[5] == len(forty[5][1]) - 1 and flag == 0
        return flat([got, fe])

    def move_batch(nz):
        raw = np.concatenate([m[0] for m in moved])
        move = np.concatenate([m[1] for m in moved])
        raw_off = np.cumsum([0] + [len(m[0]) for m in moved])
        mv_off = np.cumsum([0] + [len(m[1]) for m in moved])
        ev_off = np.cumsum([0] + [m[3] for m in moved])
        blk = DeviceArray((int(ev_off[-1]), 3), np.float32, 0)
        status, flag = nz.move_stats_device(raw, raw_off, move, mv_off, [m[2] for m in moved], ev_off, blk.ptr)
        got = blk.to_host()
        blk.free()
        assert not status.any() and flag == 0 and (got[:, 2] > 0).all()
        return flat([got, status])

    nz = signal.SignalNormalizer(0)
    for step, call in enumerate((single, host_batch, resident, move_batch, host_batch)):
        fresh = signal.SignalNormalizer(0)
        want = call(fresh)
        fresh.close()
        assert call(nz) == want, 'call %d (%s) on the shared handle differs from a fresh handle' % (step, call.__name__)
    nz.close()
