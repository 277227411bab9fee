"""Golden vectors for reads with basecaller MOVE TABLES (detect --move), produced by running the REFERENCE's own functions: getFast5Info
(bin/DeepMod_scripts/myDetect.py:297-343 of the reference tree) with moptions['move'] = True under stub `tensorflow` / `h5py` modules and an in-memory
stand-in for the FAST5 reader, so that getEvent's move branch (:136-153), MoveTable.getMove_Info (MoveTable.py:7-54), mnormalized (:266-282) and the
statistics loop (:332-343) all run.

Output (plain data): host_move.npz - per case: raw int16 signal, the move table (uint8), first (first_sample_template), fq_seq, and the reference's
results: m_event start / length / mean / stdv and m_event_basecall.

Only VALID reads go in: where the reference is undefined (boundaries != bases - 1, an event outside the signal) there is no result to record.
The smallest read the reference handles without error, found by running it: ONE base with a table that holds no boundary - an empty table, a table of
one entry (move[0] is never looked at) or any table without a 1 behind index 0 - and one sample behind `first`.  Zero bases raise IndexError at
MoveTable.py:50.  With a single sample (or any constant slice) mnormalized's scale is 0 and every value NaN, with RuntimeWarnings but no error; the
tiny_* cases keep the one-base / empty-table / one-entry-table shapes and a handful of samples, so that the recorded values are numbers.

Run where the reference tree is present (make_golden_host.import_reference finds it):  python tests/golden/make_golden_move.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_host import import_reference  # noqa: E402

_LEVEL = {'A': -1.0, 'C': -0.3, 'G': 0.4, 'T': 1.1}


class _DS:
    """a dataset (`reader[path][()]`) or a group with attributes (`reader[path].attrs[...]`)"""

    def __init__(self, v=None, attrs=None):
        self.v = v
        self.attrs = attrs or {}

    def __getitem__(self, k):
        return self.v


def run_reference(myDetect, raw, move, first, fq_seq):
    myDetect.get_channel_info = lambda mo, sp: sp.__setitem__('channel_info', {'ok': 1})
    myDetect.getAlbacoreVersion = lambda mo, sp: sp.__setitem__('used_albacore_version', 2)
    myDetect.getRawInfo = lambda mo, sp: sp.__setitem__('raw_signals', raw.copy())
    mo = {'basecall_1d': 'Basecall_1D_000', 'basecall_2strand': 'BaseCalled_template', 'outLevel': 2, 'move': True}
    base = ''.join([myDetect.fast5_analysis, '/', mo['basecall_1d'], '/', mo['basecall_2strand'], '/'])
    reader = {base + myDetect.fast5_basecall_fq: _DS(("@read1\n%s\n+\n%s\n" % (fq_seq, '!' * len(fq_seq))).encode()),
              '/'.join(['', 'Analyses', mo['basecall_1d'], mo['basecall_2strand'], 'Move']): _DS(move.copy()),
              '/Analyses/Segmentation_000/Summary/segmentation': _DS(attrs={'first_sample_template': first, 'duration_template': len(raw) - first})}
    sp = {'mfile_path': 'synthetic.fast5', 'f5status': '', 'f5reader': reader}
    myDetect.getFast5Info(mo, sp)
    assert sp['f5status'] == '', sp['f5status']
    return sp


def make_case(rng, gaps, first, tail, move0=1, twos=0, last_len=None):
    """A read of len(gaps) + 1 bases: boundary k at table index sum(gaps[:k + 1]) (gaps in strides of 2 samples), `tail` table entries behind the
    last boundary (tail >= 1; tail == 1: the last boundary is at L - 1), the signal ends last_len samples (default 2 * tail) behind the last boundary.
    twos: that many table entries that are neither 0 nor 1 (value 2: no boundary)."""
    idx = np.cumsum(np.asarray(gaps, np.int64))
    L = int(idx[-1]) + tail if len(idx) else tail
    move = np.zeros(L, np.uint8)
    move[idx] = 1
    if L:
        move[0] = move0
    free = np.flatnonzero(move == 0)
    free = free[free > 0]
    if twos:
        move[rng.choice(free, twos, replace=False)] = 2
    last = int(idx[-1]) if len(idx) else 0
    n_raw = first + 2 * last + (2 * tail if last_len is None else last_len)
    fq = ''.join(rng.choice(list('ACGT'), len(gaps) + 1))
    starts = np.concatenate([[first], first + 2 * idx]).astype(np.int64)
    level = np.zeros(n_raw)
    for k, b in enumerate(fq):
        level[starts[k]:(starts[k + 1] if k + 1 < len(starts) else n_raw)] = _LEVEL[b]
    raw = np.clip(np.round(520 + 75 * (level + rng.normal(0, 0.35, n_raw))), -32768, 32767).astype(np.int16)
    return raw, move, first, fq


def cases(rng):
    geo = lambda n, p=0.25: (1 + rng.geometric(p, n)).tolist()
    out = {}
    # ordinary reads of a few hundred to a few thousand bases; `first` odd and even, move[0] 0 and 1
    out['ordinary_300'] = make_case(rng, geo(299), 57, 3, move0=1)
    out['ordinary_1200'] = make_case(rng, geo(1199), 140, 2, move0=0)
    out['ordinary_3000'] = make_case(rng, geo(2999), 33, 5, move0=1)
    # a value 2 in the table is no boundary
    out['value_two'] = make_case(rng, geo(400), 64, 4, move0=1, twos=40)
    out['value_two_at_0'] = make_case(rng, geo(350), 21, 2, move0=2)
    # runs of zeros longer than 64 and longer than 1,024 strides
    g = geo(500)
    g[100], g[101], g[300] = 70, 130, 1100
    out['long_zero_runs'] = make_case(rng, g, 12, 3)
    g = geo(260)
    g[259] = 1500
    out['long_run_before_last'] = make_case(rng, g, 75, 1)
    # boundaries at table indices 63, 64, 65 (and around the next multiples of 64) and at L - 1
    g = [9, 9, 9, 9, 9, 9, 9, 1, 1] + [62, 1, 1] + geo(200) + [1]
    assert np.cumsum(g)[6:9].tolist() == [63, 64, 65] and np.cumsum(g)[9:12].tolist() == [127, 128, 129]
    out['wave_edges_last_at_L-1'] = make_case(rng, g, 40, 1, move0=0)
    out['first_boundary_at_1'] = make_case(rng, [1] + geo(150), 3, 2)
    # `first` = 0 and the last event a single sample
    out['first_zero_last_one_sample'] = make_case(rng, geo(220), 0, 1, last_len=1)
    # the smallest reads the reference handles (see the docstring)
    out['tiny_empty_table'] = make_case(rng, [], 5, 0, last_len=7)
    out['tiny_one_entry'] = make_case(rng, [], 4, 1, last_len=6)
    out['tiny_two_bases'] = make_case(rng, [1], 2, 1, last_len=5)
    return out


def main():
    myDetect = import_reference()
    rng = np.random.default_rng(20261016)
    out = {}
    names = []
    for name, (raw, move, first, fq) in cases(rng).items():
        sp = run_reference(myDetect, raw, move, first, fq)
        ev = sp['m_event']
        assert sp['m_event_basecall'] == fq and len(ev) == len(fq)
        names.append(name)
        out[name + '_raw'] = raw
        out[name + '_move'] = move
        out[name + '_first'] = np.int64(first)
        out[name + '_fq_seq'] = np.array(fq)
        out[name + '_basecall'] = np.array(sp['m_event_basecall'])
        for f in ('start', 'length', 'mean', 'stdv'):
            out[name + '_' + f] = np.asarray(ev[f]).copy()
        print('%-28s bases %5d table %6d samples %6d first %4d' % (name, len(fq), len(move), len(raw), first))
    out['cases'] = np.array(names)
    np.savez_compressed(os.path.join(HERE, 'host_move.npz'), **out)
    print('wrote host_move.npz', os.path.getsize(os.path.join(HERE, 'host_move.npz')), 'bytes')


if __name__ == '__main__':
    main()
