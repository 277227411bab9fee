"""Golden vectors for raw-signal normalisation + per-event statistics, produced by running the REFERENCE's own
functions (/root/reference/bin/DeepMod_scripts/myDetect.py: getFast5Info :297-343, which calls mnormalized :266-282)
in the build container with stub `tensorflow` / `h5py` modules and an in-memory stand-in for the FAST5 reader.

Output (plain data): host_signal.npz — per case: raw int16 signal, event start/length, and the reference's results:
m_event mean/stdv (float32) after the loop, the number of events kept, the normalised signal.
With --edges: host_signal_edges.npz instead (host_signal.npz is left alone) - irregular event tables and the value / length /
alignment edges of the device kernels (edge_cases below), same fields.

Run only here (needs /root/reference):  python tests/golden/make_golden_signal.py [--edges]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_host import EVENT_DTYPE, import_reference  # noqa: E402


class _DS:
    def __init__(self, v):
        self.v = v

    def __getitem__(self, k):
        return self.v


class _Reader(dict):
    pass


def run_reference(myDetect, raw, start, length):
    ev = np.zeros(len(start), dtype=EVENT_DTYPE)
    ev['start'] = start
    ev['length'] = length
    ev['model_state'] = 'NNANN'
    myDetect.get_channel_info = lambda mo, sp: sp.__setitem__('channel_info', {'ok': 1})
    myDetect.getAlbacoreVersion = lambda mo, sp: sp.__setitem__('used_albacore_version', 2)
    myDetect.getRawInfo = lambda mo, sp: sp.__setitem__('raw_signals', raw.copy())
    myDetect.getEvent = lambda mo, sp: sp.__setitem__('m_event', ev)
    mo = {'basecall_1d': 'Basecall_1D_000', 'basecall_2strand': 'BaseCalled_template', 'outLevel': 2}
    fq_path = ''.join([myDetect.fast5_analysis, '/', mo['basecall_1d'], '/', mo['basecall_2strand'], '/', myDetect.fast5_basecall_fq])
    sp = {'mfile_path': 'synthetic.fast5', 'f5status': '', 'f5reader': _Reader({fq_path: _DS(b"@read1\nACGT\n+\n!!!!\n")})}
    myDetect.getFast5Info(mo, sp)
    assert sp['f5status'] == ''
    return sp


def make_case(rng, n_raw, first, mean_len, loc=480.0, scale=70.0, long_at=None, long_len=0, overrun=None, outliers=0):
    raw = np.clip(np.round(rng.normal(loc, scale, n_raw)), -32768, 32767).astype(np.int16)
    if outliers:
        idx = rng.integers(0, n_raw, outliers)
        raw[idx] = rng.choice(np.array([-30000, -9000, 25000, 32000, 1500, -20], np.int16), outliers)
    lens = []
    pos = first
    while True:
        ln = int(rng.geometric(1.0 / mean_len))
        if long_at is not None and len(lens) == long_at:
            ln = long_len
        if pos + ln > n_raw - 5:
            break
        lens.append(ln)
        pos += ln
    length = np.array(lens, np.uint64)
    start = (first + np.concatenate([[0], np.cumsum(length[:-1])])).astype(np.uint64)
    if overrun == 'clamp':          # last event runs past the end of the signal: numpy clamps the slice
        length[-1] = np.uint64(n_raw - int(start[-1]) + 40)
    elif overrun is not None:       # event `overrun` and everything after it start beyond the signal
        start[overrun:] += np.uint64(n_raw)
    return raw, start, length


def _strand(rng, n_raw, first, mean_len, loc=480.0, scale=70.0, margin=5):
    """raw int16 [n_raw] ~ N(loc, scale) and contiguous events from sample `first` that end at least `margin` samples before the end"""
    raw = np.clip(np.round(rng.normal(loc, scale, n_raw)), -32768, 32767).astype(np.int16)
    length = np.maximum(1, rng.geometric(1.0 / mean_len, int(n_raw / mean_len) + 10)).astype(np.uint64)
    start = (first + np.concatenate([[0], np.cumsum(length[:-1])])).astype(np.uint64)
    keep = start + length <= n_raw - margin
    return raw, start[keep].copy(), length[keep].copy()


def edge_cases(rng):
    """Inputs where the device kernels can go wrong: events that reach outside the covered slice [start_0, start_last + length_last), the
    ends of the int16 range and of the LDS bins, numpy's summation boundaries, every 16-byte head / tail residue, the distinct-value cap of
    the device order statistics (NORM_CAP = 4,096)."""
    cases = {}
    # open pore: the strand's events start at sample 2,000; the samples before sit ~8 mscale above the strand's level (MAD of N(480, 70) ~ 47)
    def open_pore():
        raw, start, length = _strand(rng, 30000, 2000, 9.0)
        raw[:2000] = np.round(rng.normal(480.0 + 8 * 47.0, 6.0, 2000)).astype(np.int16)
        return raw, start, length
    raw, start, length = open_pore()
    start[len(start) // 2] = 100                                        # (a) one event in the middle starts in the open pore
    cases['open_pore_a'] = (raw, start, length)
    raw, start, length = open_pore()                                    # (b) events 0-2 (in the open pore) listed after event 3 (the strand's first)
    start = np.r_[start[:1], [1940, 1960, 1980], start[1:]].astype(np.uint64)
    length = np.r_[length[:1], [20, 20, 20], length[1:]].astype(np.uint64)
    cases['open_pore_b'] = (raw, start, length)
    raw, start, length = open_pore()                                    # (c) as (b), but the early events lie inside the slice
    start = np.r_[start[:1], [2100, 2120, 2140], start[1:]].astype(np.uint64)
    length = np.r_[length[:1], [20, 20, 20], length[1:]].astype(np.uint64)
    cases['open_pore_c'] = (raw, start, length)
    # overlapping tail: a middle event runs past the end of the slice into 40 samples above the strand's level and spikes at -30,000 and 32,000
    raw, start, length = _strand(rng, 30000, 50, 9.0, margin=60)
    hi = int(start[-1] + length[-1])
    raw[hi:hi + 40] = np.round(rng.normal(950.0, 20.0, 40)).astype(np.int16)
    raw[hi + 3], raw[hi + 4], raw[hi + 9] = -30000, 32000, 32000
    k = len(start) // 2
    length[k] = hi + 40 - int(start[k])
    cases['overlap_tail'] = (raw, start, length)
    # extreme values inside the slice: the table's first and last entries, both sides of the LDS-bin edges
    raw, start, length = _strand(rng, 20000, 7, 9.0)
    ext = np.array([-32768, 32767, -2049, -2048, -2047, 6143, 6144, 6145, -32768, 32767], np.int16)
    raw[rng.choice(np.arange(100, 19000), len(ext), replace=False)] = ext
    raw[5000:5004] = [-32768, -32768, 32767, 32767]
    cases['extreme_values'] = (raw, start, length)
    # numpy's pairwise leaf (8 lanes, 128-element blocks) and its 8,192-element buffer
    sizes = [1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, 16385]
    raw, start, length = _strand(rng, 45000, 13, 9.0)
    lens = np.array(sizes + [9] * 300, np.uint64)
    lens = lens[rng.permutation(len(lens))]
    st = (13 + np.concatenate([[0], np.cumsum(lens[:-1])])).astype(np.uint64)
    cases['sum_boundaries'] = (raw, st, lens)
    # the 16-byte head and tail of the histogram's body: a slice start and end at every residue mod 8, and a slice inside one 8-sample group
    for res in range(8):
        raw, start, length = _strand(rng, 6000 + res, 16 + res, 6.0, margin=16)
        end_res = (7 - res + 3) % 8
        hi = int(start[-1] + length[-1])
        length[-1] += np.uint64((end_res - hi) % 8)
        cases['slice_mod8_%d' % res] = (raw, start, length)
    raw = rng.integers(400, 600, 64).astype(np.int16)
    cases['slice_in_one_group'] = (raw, np.array([9, 10, 12], np.uint64), np.array([1, 2, 3], np.uint64))
    # the device order statistics take at most 4,096 distinct values of a slice; 4,097 go to the host
    for nv in (4096, 4097):
        raw, start, length = _strand(rng, 20000, 40, 9.0)
        vals = (200 + np.arange(nv)).astype(np.int16)
        lo, hi = int(start[0]), int(start[-1] + length[-1])
        raw[lo:hi] = vals[rng.integers(0, nv, hi - lo)]
        raw[lo:lo + nv] = vals[rng.permutation(nv)]
        cases['distinct_%d' % nv] = (raw, start, length)
    return cases


def main_edges():
    myDetect = import_reference()
    out = {}
    for name, (raw, start, length) in edge_cases(np.random.default_rng(20261015)).items():
        sp = run_reference(myDetect, raw, start, length)
        ev = sp['m_event']
        out[name + '.raw'] = raw
        out[name + '.start'] = start
        out[name + '.length'] = length
        out[name + '.n_kept'] = np.int64(len(ev))
        out[name + '.mean'] = ev['mean'].astype(np.float32)
        out[name + '.stdv'] = ev['stdv'].astype(np.float32)
        if name in ('open_pore_a', 'extreme_values'):      # the normalised signal itself (float64) for two cases
            out[name + '.signal'] = np.asarray(sp['raw_signals'], np.float64)
        print(name, len(raw), 'samples', len(start), 'events ->', len(ev), 'kept; mean[0..3]', ev['mean'][:3], 'stdv', ev['stdv'][:3])
    np.savez_compressed(os.path.join(HERE, 'host_signal_edges.npz'), **out)


def main():
    if '--edges' in sys.argv[1:]:
        return main_edges()
    myDetect = import_reference()
    rng = np.random.default_rng(20260928)
    cases = {
        'typical': make_case(rng, 30011, 137, 9.0),
        'even_slice': make_case(rng, 20000, 0, 7.0, loc=100.0, scale=3.0),              # tiny value range: x.5 medians
        'long_events': make_case(rng, 60000, 50, 12.0, long_at=20, long_len=20011),      # > 8192 and > 128 samples
        'mid_events': make_case(rng, 16000, 3, 150.0),                                    # 8 <= n <= 128 and recursion
        'outliers': make_case(rng, 25000, 11, 9.0, outliers=400),                         # values outside the LDS bins
        'clamped_tail': make_case(rng, 12000, 20, 9.0, overrun='clamp'),
        'empty_late': make_case(rng, 12000, 20, 9.0, overrun=700),                        # first empty event i > 500
        'empty_early': make_case(rng, 12000, 20, 9.0, overrun=300),                       # i <= 500: table kept
    }
    out = {}
    for name, (raw, start, length) in cases.items():
        sp = run_reference(myDetect, raw, start, length)
        ev = sp['m_event']
        out[name + '.raw'] = raw
        out[name + '.start'] = start
        out[name + '.length'] = length
        out[name + '.n_kept'] = np.int64(len(ev))
        out[name + '.mean'] = ev['mean'].astype(np.float32)
        out[name + '.stdv'] = ev['stdv'].astype(np.float32)
        if name in ('typical', 'outliers'):      # the normalised signal itself (float64) for two cases
            out[name + '.signal'] = np.asarray(sp['raw_signals'], np.float64)
        print(name, len(raw), 'samples', len(start), 'events ->', len(ev), 'kept; mean[0..3]', ev['mean'][:3], 'stdv', ev['stdv'][:3])
    np.savez_compressed(os.path.join(HERE, 'host_signal.npz'), **out)


if __name__ == '__main__':
    main()
