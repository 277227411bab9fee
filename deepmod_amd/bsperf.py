"""`bsperf`: the predicted percentages of a run against whole-genome bisulfite replicates (docs/Reproducibility.md of the reference, Example 3,
Step 5 - the one step of its human workflow it ships no script for).

A position is *completely methylated* if its percentage is >= 90 in every replicate at coverage >= c (c = 1, 5, 10), *completely un-methylated*
if it is 0 in every replicate; the predicted percentages are scored on those two classes (ROC AUC, average precision), and against the mean
bisulfite percentage on every site (Pearson r, RMSE).

HostEngine below is the numpy statement of the semantics and the yardstick of the kernels (csrc/bsperf.hip.inc, DeviceEngine), as
siteperf.HostEngine is for `siteperf`.  Everything counted is an integer; the scores are float64 functions of the integers alone (measures).
The prediction side is merge.DeviceMerge: the summed counters of every *.<chr>+.<Base>.bed / *.<chr>-.<Base>.bed below --predFolder.  The truth side is
read by the rules of cluster_train.read_truth (readBed of hm_cluster_predict.py:20-41), with two departures: a line whose strand is neither '+' nor
'-' is skipped and counted, and a key that occurs twice in one replicate is refused (readBed keeps the later line).
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import _lib, merge, siteperf, tables

NPCT, MAX_THRESHOLDS, MAX_REPLICATES, MAX_CONTIGS, MAX_NAME, MAX_COV, SHORT_LINE = 101, 8, 4, 64, 63, 65535, 20
MAX_LENGTH = merge.MAX_LENGTH
LINE_KEYS = ('records', 'first_lines', 'short', 'other_strand', 'other_contig', 'zero_coverage')      # bsk::L_* of csrc/bsperf.inc
LABELS = ('unmethylated', 'methylated', 'intermediate')
KINDS = ('raw', 'clustered')
CHUNK_BYTES = 64 << 20                                   # of truth text handed to the device at once, cut at a line end


class BsPerfError(ValueError):
    pass


def pack_meta(contig, strand, cov, pct) -> np.ndarray:
    """coverage (saturated at 65,535) | percentage << 16 | strand << 23 | contig index << 24, as csrc/bsperf.inc packs a record."""
    cov = np.minimum(np.asarray(cov, np.int64), MAX_COV)
    return (cov | (np.asarray(pct, np.int64) << 16) | (np.asarray(strand, np.int64) << 23) | (np.asarray(contig, np.int64) << 24)).astype(np.uint32)


def unpack_meta(meta) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """-> contig index, strand, coverage, percentage."""
    m = np.asarray(meta, np.uint32).astype(np.int64)
    return m >> 24, (m >> 23) & 1, m & 0xffff, (m >> 16) & 0x7f


def _limits(names: Sequence[str], lengths) -> List[int]:
    return [MAX_LENGTH if lengths is None or lengths[k] is None or lengths[k] < 0 else int(lengths[k]) for k in range(len(names))]


def host_rows(text: bytes, names: Sequence[str], lengths=None, first_chunk: bool = True, where: str = '<text>', first_line: int = 1):
    """The host statement of the reading rules, line by line as readBed reads: split(), int(), the first-line skip and the <= 20 skip.
    -> (pos int32, meta uint32, lines int64 [6]) in line order; what no table can hold is refused as BsPerfError `file:line: reason`."""
    limit = _limits(names, lengths)
    index = {n.encode('ascii'): k for k, n in enumerate(names)}
    lines = np.zeros(len(LINE_KEYS), np.int64)
    pos, contig, strand, cov, pct = [], [], [], [], []
    raw = text.split(b'\n')
    if raw and raw[-1] == b'':
        raw.pop()
    for no, line in enumerate(raw, first_line):
        if first_chunk and no == first_line:
            lines[1] += 1
            continue
        line = line.strip()
        if len(line) <= SHORT_LINE:
            lines[2] += 1
            continue
        f = line.split()
        if len(f) != 11:
            raise BsPerfError('%s:%d: %d fields, a bedMethyl line has 11' % (where, no, len(f)))
        try:
            p, c, q = int(f[1]), int(f[9]), int(f[10])
        except ValueError as exc:
            raise BsPerfError('%s:%d: %s' % (where, no, exc))
        if not (0 <= p <= 2 ** 31 - 1 and 0 <= c <= 2 ** 31 - 1 and 0 <= q <= 100):
            raise BsPerfError('%s:%d: position %d, coverage %d, percentage %d: outside 0 .. 2^31 - 1, percentage <= 100' % (where, no, p, c, q))
        if f[5] not in (b'+', b'-'):
            lines[3] += 1
            continue
        k = index.get(f[0])
        if k is None:
            lines[4] += 1
            continue
        if p >= limit[k]:
            raise BsPerfError('%s:%d: position %d is not on %s (%d %s)' % (where, no, p, names[k], limit[k], 'bases' if limit[k] < MAX_LENGTH else 'positions at most'))
        if c == 0:
            lines[5] += 1
            continue
        lines[0] += 1
        pos.append(p)
        contig.append(k)
        strand.append(1 if f[5] == b'-' else 0)
        cov.append(c)
        pct.append(q)
    return np.array(pos, np.int32), pack_meta(np.array(contig, np.int64), np.array(strand, np.int64), np.array(cov, np.int64), np.array(pct, np.int64)), lines


def _names_args(names: Sequence[str], lengths):
    import ctypes
    enc = [n.encode('ascii', 'replace') for n in names]
    arr = (ctypes.c_char_p * max(len(enc), 1))(*enc)
    lens = np.array([-1 if lengths is None or lengths[k] is None else int(lengths[k]) for k in range(len(names))] or [-1], np.int64)
    return arr, lens


def parse_device_grammar(text: bytes, names: Sequence[str], lengths=None, first_chunk: bool = True):
    """The device's line routine compiled for the host (no GPU needed) -> ((pos, meta), lines int64 [6], flag, first bad line)."""
    import ctypes
    lib = _lib.load()
    arr, lens = _names_args(names, lengths)
    flag, bad = ctypes.c_int32(0), ctypes.c_int64(-1)
    lines = np.zeros(len(LINE_KEYS), np.int64)
    head = (ctypes.c_char_p(text), len(text), len(names), arr, lens.ctypes.data, int(bool(first_chunk)))
    n = lib.dm_bsperf_parse_host(*head, None, None, 0, lines.ctypes.data, ctypes.byref(flag), ctypes.byref(bad))
    if n < 0:
        _lib.check(int(n))
    pos, meta = np.zeros(n, np.int32), np.zeros(n, np.uint32)
    if n:
        lib.dm_bsperf_parse_host(*head, pos.ctypes.data, meta.ctypes.data, n, lines.ctypes.data, ctypes.byref(flag), ctypes.byref(bad))
    return (pos, meta), lines, flag.value, bad.value


def tile_bytes() -> int:
    return _lib.load().dm_bsperf_tile_bytes()


def _check_thresholds(thresholds) -> Tuple[int, ...]:
    t = tuple(int(v) for v in thresholds)
    if not 1 <= len(t) <= MAX_THRESHOLDS:
        raise BsPerfError('bsperf: --cov: 1 to %d coverage thresholds (got %d)' % (MAX_THRESHOLDS, len(t)))
    if any(v < 1 for v in t) or any(b <= a for a, b in zip(t, t[1:])):
        raise BsPerfError('bsperf: --cov: the coverage thresholds are positive and strictly ascending (got %s)' % (t,))
    return t


def _check_engine_options(names, thresholds, replicates, methylated, unmethylated, pred_cov):
    thresholds = _check_thresholds(thresholds)
    if not 1 <= len(names) <= MAX_CONTIGS:
        raise BsPerfError('bsperf: --chr: 1 to %d contigs (got %d)' % (MAX_CONTIGS, len(names)))
    for n in names:
        if not 1 <= len(n) <= MAX_NAME or any(not 0x21 <= ord(c) <= 0x7e for c in n):
            raise BsPerfError('bsperf: --chr: a contig name has 1 to %d printable bytes (got %r)' % (MAX_NAME, n))
    if len(set(names)) != len(names):
        raise BsPerfError('bsperf: --chr: a contig is named twice')
    if not 1 <= int(replicates) <= MAX_REPLICATES:
        raise BsPerfError('bsperf: --truth: 1 to %d replicate files (got %d)' % (MAX_REPLICATES, replicates))
    if not 0 <= int(unmethylated) < int(methylated) <= 100:
        raise BsPerfError('bsperf: --methylated / --unmethylated: 0 <= unmethylated < methylated <= 100 (got %d, %d)' % (unmethylated, methylated))
    if int(pred_cov) < 1:
        raise BsPerfError('bsperf: --predCov: the least prediction coverage is 1 or more (got %d)' % pred_cov)
    return thresholds


class HostEngine:
    """The semantics in numpy: one contig at a time, the counters accumulate over contigs.  Per (strand, position) of the open contig:
      truth       the site has truth if every replicate has a record; m = min coverage; bucket = (thresholds <= m) - 1, a site below the smallest
                  threshold is counted in below_threshold only; label 1 if every percentage >= methylated, else 0 if every percentage <=
                  unmethylated, else 2; y = the sum of the percentages
      prediction  kind 0: predicted if the summed coverage >= pred_cov, x = (100 * mod) // cov; kind 1: predicted if add_scores names it, x its percentage
    hist [kind][label][bucket][x] sites with truth and a prediction; moments [kind][bucket] = n, sum x, sum y, sum xy, sum x^2, sum y^2 of those;
    unpredicted [kind][label][bucket] sites with truth only; untruthed [kind] predicted sites without truth."""

    def __init__(self, names, thresholds=(1, 5, 10), replicates: int = 2, methylated: int = 90, unmethylated: int = 0, pred_cov: int = 1, lengths=None):
        self.names = list(names)
        self.thresholds = _check_engine_options(self.names, thresholds, replicates, methylated, unmethylated, pred_cov)
        self.R, self.methylated, self.unmethylated, self.pred_cov = int(replicates), int(methylated), int(unmethylated), int(pred_cov)
        self.limit = _limits(self.names, lengths)
        T = len(self.thresholds)
        self.hist = np.zeros((2, 3, T, NPCT), np.int64)
        self.unpredicted = np.zeros((2, 3, T), np.int64)
        self.moments = np.zeros((2, T, 6), np.int64)
        self.untruthed = np.zeros(2, np.int64)
        self.below_threshold = np.zeros(2, np.int64)
        self.lines = np.zeros(len(LINE_KEYS), np.int64)
        self.contig = None

    def close(self):
        pass

    def add_lines(self, lines):
        self.lines += np.asarray(lines, np.int64)

    def open(self, contig: int, plus, minus):
        """plus, minus: (cov, mod) of either strand, arrays of one length."""
        if not 0 <= contig < len(self.names):
            raise BsPerfError('bsperf: contig %d of %d' % (contig, len(self.names)))
        self.cov = np.stack([np.asarray(plus[0], np.int64), np.asarray(minus[0], np.int64)])
        self.mod = np.stack([np.asarray(plus[1], np.int64), np.asarray(minus[1], np.int64)])
        self.length = self.cov.shape[1]
        if not 1 <= self.length <= self.limit[contig]:
            raise BsPerfError('bsperf: tables of %d positions for a contig of %d' % (self.length, self.limit[contig]))
        self.truth = np.zeros((self.R, 2, self.length), np.uint32)
        self.contig, self.refused, self.counted, self.scored = contig, False, False, False

    def close_contig(self):
        self.contig = None

    def _opened(self):
        if self.contig is None:
            raise BsPerfError('bsperf: no contig')

    def fill(self, replicate: int, pos, meta):
        self._opened()
        pos, meta = np.asarray(pos, np.int64), np.asarray(meta, np.uint32)
        contig, strand, cov, pct = unpack_meta(meta)
        if not 0 <= replicate < self.R:
            raise BsPerfError('bsperf: replicate %d of %d' % (replicate, self.R))
        bad = (pos < 0) | (pos >= self.length) | (contig != self.contig) | (cov < 1) | (pct > 100)
        if bad.any():
            raise BsPerfError('bsperf: record %d is outside the open contig or the value ranges' % int(np.argmax(bad)))
        key = pos * 2 + strand
        taken = self.truth[replicate, strand, pos] != 0
        order = np.sort(key)
        twice = np.concatenate([order[1:][order[1:] == order[:-1]], key[taken]])
        if len(twice):
            self.refused = True
            k = int(twice.min())
            raise BsPerfError('bsperf: replicate %d holds position %d of strand %s twice' % (replicate, k >> 1, '+-'[k & 1]))
        self.truth[replicate, strand, pos] = (0x80000000 | (meta.astype(np.int64) & 0x7fffff)).astype(np.uint32)

    def _sweep(self, kind: int, predicted: np.ndarray, x: np.ndarray):
        t = self.truth.astype(np.int64)
        has = (t != 0).all(axis=0)
        cov, pct = t & 0xffff, (t >> 16) & 0x7f
        m, y = cov.min(axis=0), pct.sum(axis=0)
        label = np.where((pct >= self.methylated).all(axis=0), 1, np.where((pct <= self.unmethylated).all(axis=0), 0, 2))
        bucket = np.searchsorted(np.asarray(self.thresholds, np.int64), m, 'right')               # thresholds <= m
        self.untruthed[kind] += int((predicted & ~has).sum())
        self.below_threshold[kind] += int((has & (bucket == 0)).sum())
        ok = has & (bucket > 0)
        un, sc = ok & ~predicted, ok & predicted
        np.add.at(self.unpredicted[kind], (label[un], bucket[un] - 1), 1)
        np.add.at(self.hist[kind], (label[sc], bucket[sc] - 1, x[sc]), 1)
        xs, ys, bs = x[sc], y[sc], bucket[sc] - 1
        for b in range(len(self.thresholds)):
            xb, yb = xs[bs == b], ys[bs == b]
            self.moments[kind, b] += np.array([len(xb), xb.sum(), yb.sum(), (xb * yb).sum(), (xb * xb).sum(), (yb * yb).sum()], np.int64)

    def count(self):
        self._opened()
        if self.refused or self.counted:
            raise BsPerfError('bsperf: the contig was refused or has been counted')
        if ((self.cov < 0) | (self.mod < 0) | (self.mod > self.cov)).any():
            raise BsPerfError('bsperf: a sum is outside 0 <= modified <= coverage')
        predicted = self.cov >= self.pred_cov
        self._sweep(0, predicted, np.where(predicted, (100 * self.mod) // np.maximum(self.cov, 1), 0))
        self.counted = True

    def add_scores(self, pos, strand, pct):
        self._opened()
        if not self.counted or self.scored:
            raise BsPerfError('bsperf: add_scores comes once per contig, after count')
        pos, strand, pct = np.asarray(pos, np.int64), np.asarray(strand, np.int64), np.asarray(pct, np.int64)
        if ((pos < 0) | (pos >= self.length) | (strand < 0) | (strand > 1) | (pct < 0) | (pct > 100)).any() or len(np.unique(pos * 2 + strand)) != len(pos):
            raise BsPerfError('bsperf: a site is outside the contig or the value ranges, or occurs twice')
        predicted = np.zeros((2, self.length), bool)
        x = np.zeros((2, self.length), np.int64)
        predicted[strand, pos] = True
        x[strand, pos] = pct
        self._sweep(1, predicted, x)
        self.scored = True

    def fetch(self) -> Dict[str, object]:
        return {'hist': self.hist.copy(), 'unpredicted': self.unpredicted.copy(), 'moments': self.moments.copy(), 'untruthed': self.untruthed.copy(),
                'below_threshold': self.below_threshold.copy(), 'lines': self.lines.copy()}


class DeviceTruth:
    """The truth side of a device handle (bsk::Truth of csrc/bsperf.hip.inc: one copy of the code behind PREFIX_add_truth_text / _add_truth_records /
    _fetch_records / _fill), for a _lib.Handle whose command raises ERROR; read_truth_device drives the first three."""
    ERROR = None

    def _refuse(self, what: str):
        return self.ERROR('%s: %s' % (self.PREFIX[3:], what))

    def add_truth_text(self, replicate: int, text: bytes, first_chunk: bool):
        """-> (lines int64 [6], records, flag, first bad line (1-based, -1: none)); a flagged chunk adds nothing."""
        ct = self._ct
        lines = np.zeros(len(LINE_KEYS), np.int64)
        n, flag, bad = ct.c_int64(0), ct.c_int32(0), ct.c_int64(-1)
        self._n = 0
        self._libmod.check(self._fn('add_truth_text')(self._h, replicate, ct.c_char_p(text), len(text), int(bool(first_chunk)), lines.ctypes.data, ct.byref(n),
                                                      ct.byref(flag), ct.byref(bad)))
        self._n = n.value
        return lines, n.value, flag.value, bad.value

    def add_truth_records(self, replicate: int, pos, meta, lines):
        pos, lines = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(lines, np.int64)
        contig, strand, cov, pct = unpack_meta(meta)
        cols = [np.ascontiguousarray(contig, np.uint8), np.ascontiguousarray(strand, np.uint8), pos, np.ascontiguousarray(cov, np.int32), np.ascontiguousarray(pct, np.int32)]
        if len({len(a) for a in cols}) != 1 or len(lines) != len(LINE_KEYS):
            raise self._refuse('record arrays of different lengths')
        self._n = 0
        self._libmod.check(self._fn('add_truth_records')(self._h, replicate, len(pos), *[a.ctypes.data for a in cols], lines.ctypes.data))
        self._n = len(pos)

    def records(self):
        """(pos, meta) of the last add_truth_text / add_truth_records as they lie on the device."""
        pos, meta = np.zeros(self._n, np.int32), np.zeros(self._n, np.uint32)
        self._libmod.check(self._fn('fetch_records')(self._h, pos.ctypes.data, meta.ctypes.data))
        return pos, meta

    def fill(self, replicate: int, pos, meta):
        ct = self._ct
        pos, meta = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(meta, np.uint32)
        if len(pos) != len(meta):
            raise self._refuse('record arrays of different lengths')
        dup, strand = ct.c_int64(-1), ct.c_int32(-1)
        self._n = 0
        rc = self._fn('fill')(self._h, int(replicate), len(pos), pos.ctypes.data, meta.ctypes.data, ct.byref(dup), ct.byref(strand))
        if dup.value >= 0:
            raise self._refuse('replicate %d holds position %d of strand %s twice' % (replicate, dup.value, '+-'[strand.value & 1]))
        self._libmod.check(rc)


class DeviceEngine(DeviceTruth, _lib.Handle):
    """The same counting on one GPU (dm_bsperf_* of the C ABI); add_truth_text is the device parser.  open takes the two summary.PositionSummary
    tables of merge.DeviceMerge.  times(): ms of the parse / fill / count kernels so far."""
    PREFIX, N_TIMES, ERROR = 'dm_bsperf', 3, BsPerfError

    def __init__(self, names, thresholds=(1, 5, 10), replicates: int = 2, methylated: int = 90, unmethylated: int = 0, pred_cov: int = 1, lengths=None, device: int = 0):
        self.names = list(names)
        self.thresholds = _check_engine_options(self.names, thresholds, replicates, methylated, unmethylated, pred_cov)
        self.R = int(replicates)
        arr, lens = _names_args(self.names, lengths)
        t = np.asarray(self.thresholds, np.int32)
        self._create(device, len(self.names), arr, lens.ctypes.data, len(t), t.ctypes.data, self.R, int(methylated), int(unmethylated), int(pred_cov))
        self._n = 0

    def open(self, contig: int, plus, minus):
        self._libmod.check(self._lib.dm_bsperf_open(self._h, int(contig), plus._h, minus._h))

    def close_contig(self):
        self._libmod.check(self._lib.dm_bsperf_close_contig(self._h))

    def count(self):
        self._libmod.check(self._lib.dm_bsperf_count(self._h))

    def add_scores(self, pos, strand, pct):
        pos, strand, pct = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(strand, np.uint8), np.ascontiguousarray(pct, np.int32)
        if not len(pos) == len(strand) == len(pct):
            raise BsPerfError('bsperf: site arrays of different lengths')
        self._libmod.check(self._lib.dm_bsperf_add_scores(self._h, len(pos), pos.ctypes.data, strand.ctypes.data, pct.ctypes.data))

    def fetch(self) -> Dict[str, object]:
        T = len(self.thresholds)
        out = {'hist': np.zeros((2, 3, T, NPCT), np.int64), 'unpredicted': np.zeros((2, 3, T), np.int64), 'moments': np.zeros((2, T, 6), np.int64),
               'untruthed': np.zeros(2, np.int64), 'below_threshold': np.zeros(2, np.int64), 'lines': np.zeros(len(LINE_KEYS), np.int64)}
        self._libmod.check(self._lib.dm_bsperf_fetch(self._h, *[out[k].ctypes.data for k in ('hist', 'unpredicted', 'moments', 'untruthed', 'below_threshold', 'lines')]))
        return out


def correlation(mom, replicates: int) -> Tuple[float, float]:
    """(Pearson r, RMSE in percentage points) of x against y / R from n, sum x, sum y, sum xy, sum x^2, sum y^2: the numerator and the two
    variance terms in Python integers, one division and one square root at the end.  r is nan when a variance is 0, both are nan when n < 2."""
    n, sx, sy, sxy, sxx, syy = (int(v) for v in mom)
    if n < 2:
        return float('nan'), float('nan')
    R = int(replicates)
    rmse = math.sqrt((R * R * sxx - 2 * R * sxy + syy) / (R * R * n))
    num, vx, vy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    if vx <= 0 or vy <= 0:
        return float('nan'), rmse
    return num / math.sqrt(vx * vy), rmse


def measures(got: Dict[str, object], thresholds, replicates: int, kinds=(0,)) -> Dict[str, Dict[int, Dict[str, object]]]:
    """{kind: {threshold: the counts and scores over the sites whose truth coverage is >= threshold (buckets j .. T - 1)}}.  AUC and AP of label 1
    against label 0 in sklearn's arithmetic (siteperf.roc_from_hist / pr_from_hist)."""
    out = {}
    for kind in kinds:
        out[KINDS[kind]] = {}
        for j, t in enumerate(thresholds):
            h = got['hist'][kind][:, j:].sum(axis=1)                  # [label][pct]
            un = got['unpredicted'][kind][:, j:].sum(axis=1)
            mom = got['moments'][kind][j:].sum(axis=0)
            area, fpr, tpr, roc_pct = siteperf.roc_from_hist(h[1], h[0])
            ap, precision, recall, pr_pct = siteperf.pr_from_hist(h[1], h[0])
            r, rmse = correlation(mom, replicates)
            out[KINDS[kind]][int(t)] = {'methylated': int(h[1].sum()), 'unmethylated': int(h[0].sum()), 'intermediate': int(h[2].sum()),
                                        'methylated_unpredicted': int(un[1]), 'unmethylated_unpredicted': int(un[0]), 'intermediate_unpredicted': int(un[2]),
                                        'auc': area, 'ap': ap, 'n': int(mom[0]), 'r': r, 'rmse': rmse,
                                        'roc': {'fpr': fpr, 'tpr': tpr, 'pct': roc_pct}, 'pr': {'precision': precision, 'recall': recall, 'pct': pr_pct}}
    return out


def report_lines(meas) -> List[str]:
    """One line per kind and threshold."""
    lines = []
    for kind in KINDS:
        for t, m in meas.get(kind, {}).items():
            lines.append('%s cov>=%d methylated=%d unmethylated=%d methylated_unpredicted=%d unmethylated_unpredicted=%d auc=%.7f ap=%.5f n=%d r=%.5f rmse=%.3f'
                         % (kind, t, m['methylated'], m['unmethylated'], m['methylated_unpredicted'], m['unmethylated_unpredicted'], m['auc'], m['ap'], m['n'], m['r'],
                            m['rmse']))
    return lines


def check_options(mo: Dict[str, object]):
    """What can be refused before any file is read or any GPU asked for -> (contigs, thresholds, truth files, cluster checkpoint prefix or None,
    {contig: bases} of --Ref)."""
    truth = [p for p in (mo.get('truth') or []) if p]
    if not truth:
        raise BsPerfError('bsperf: --truth: the bisulfite bedMethyl replicates, separated by commas, are needed')
    if len(truth) > MAX_REPLICATES:
        raise BsPerfError('bsperf: --truth: 1 to %d replicate files (got %d)' % (MAX_REPLICATES, len(truth)))
    for p in truth:
        if not os.path.isfile(p):
            raise BsPerfError('bsperf: --truth: replicate file does not exist (%s)' % p)
    try:
        chrkeys, prefix, fasta = merge.check_options({k: mo.get(k) for k in ('predFolder', 'chr', 'Ref', 'clusterCpG', 'Base')})
    except merge.MergeError as exc:                                            # the options and rules are merge's; the command named is this one
        text = str(exc)
        raise BsPerfError('bsperf' + text[len('merge'):] if text.startswith('merge:') else text)
    thresholds = _check_engine_options(chrkeys, mo.get('cov') or (1, 5, 10), len(truth), int(mo.get('methylated', 90)), int(mo.get('unmethylated', 0)),
                                       int(mo.get('predCov', 1)))
    return chrkeys, thresholds, truth, prefix, fasta


def chunks_of(path: str, chunk_bytes: int = CHUNK_BYTES):
    """The file in pieces of about chunk_bytes, each cut behind a line end -> (bytes, is the file's first piece)."""
    first, rest = True, b''
    with open(path, 'rb') as fh:
        while True:
            block = fh.read(chunk_bytes)
            if not block:
                break
            cut = block.rfind(b'\n')
            if cut < 0:
                rest += block
                continue
            yield rest + block[:cut + 1], first
            first, rest = False, block[cut + 1:]
    if rest:
        yield rest, first


def read_truth_device(eng, replicate: int, path: str, names, lengths, notes: List[str], phase: Dict[str, float], chunk_bytes: int = CHUNK_BYTES):
    """One replicate file through the engine's parser, chunk by chunk -> ({contig index: (pos, meta)} in line order, lines int64 [6])."""
    import time
    parts: Dict[int, list] = {}
    lines = np.zeros(len(LINE_KEYS), np.int64)
    line_no = 1
    t0 = time.perf_counter()
    for text, first in chunks_of(path, chunk_bytes):
        t1 = time.perf_counter()
        phase['read'] += t1 - t0
        got, n, flag, bad = eng.add_truth_text(replicate, text, first)
        if flag:
            notes.append('%s: line %d is outside the device grammar: the chunk of %d lines from line %d on is parsed on the host'
                         % (path, line_no + bad - 1, text.count(b'\n') + (0 if text.endswith(b'\n') else 1), line_no))
            pos, meta, got = host_rows(text, names, lengths, first, path, line_no)
            eng.add_truth_records(replicate, pos, meta, got)
        pos, meta = eng.records()
        t2 = time.perf_counter()
        phase['parse'] += t2 - t1
        lines += got
        contig = (meta >> np.uint32(24)).astype(np.uint8)
        for c in np.unique(contig):
            sel = contig == c
            parts.setdefault(int(c), []).append((pos[sel], meta[sel]))
        line_no += text.count(b'\n') + (0 if text.endswith(b'\n') else 1)
        t0 = time.perf_counter()
        phase['bucket'] += t0 - t2
    t1 = time.perf_counter()
    out = {c: (np.concatenate([p for p, _ in v]), np.concatenate([m for _, m in v])) for c, v in parts.items()}
    phase['bucket'] += time.perf_counter() - t1
    return out, lines


def _clean(v):
    if isinstance(v, float) and math.isnan(v):
        return None
    if isinstance(v, dict):
        return {k: _clean(x) for k, x in v.items()}
    if isinstance(v, list):
        return [_clean(x) for x in v]
    return v


def bsperf(mo: Dict[str, object], device: int = 0, chunk_bytes: int = CHUNK_BYTES) -> Dict[str, object]:
    """The command.  mo: predFolder, truth (list of replicate files), Base, outFolder, FileID, chr (list; None: chr1..22, X, Y, M), cov (thresholds),
    predCov, methylated, unmethylated, Ref (None: a contig is as long as the largest position seen + 1), clusterCpG (None: raw scores only; '':
    DEEPMOD_CLUSTER_MODEL; else the checkpoint prefix), threads.  Writes <outFolder>/<FileID>_bsperf.txt / .json -> the JSON document (with
    'lines' and the wall-clock seconds of the phases in 'phase_s', which are not written)."""
    import json
    import time
    from concurrent.futures import ThreadPoolExecutor
    chrkeys, thresholds, truth, prefix, fasta = check_options(mo)
    folder, base, fileid = mo['predFolder'], str(mo['Base']), str(mo.get('FileID') or 'mod')
    methylated, unmethylated, pred_cov = int(mo.get('methylated', 90)), int(mo.get('unmethylated', 0)), int(mo.get('predCov', 1))
    from . import _lib, cluster
    if _lib.load().dm_device_count() < 1:
        raise BsPerfError('no gfx950 GPU visible (this build has no CPU path)')
    lengths = [len(fasta[ck]) if ck in fasta else -1 for ck in chrkeys]
    R = len(truth)
    phase = {k: 0.0 for k in ('read', 'parse', 'bucket', 'fill', 'merge', 'count', 'cluster')}

    eng = DeviceEngine(chrkeys, thresholds, R, methylated, unmethylated, pred_cov, lengths, device)
    dev = merge.DeviceMerge(device)
    model = cluster.ClusterModel.from_checkpoint(prefix, device) if prefix else None
    doc = {'inputs': {'predFolder': folder, 'truth': truth, 'Base': base, 'FileID': fileid, 'chr': chrkeys, 'cov': list(thresholds), 'predCov': pred_cov,
                      'methylated': methylated, 'unmethylated': unmethylated, 'Ref': mo.get('Ref'), 'clusterCpG': prefix},
           'truth': {}, 'contigs': {}, 'notes': []}
    try:
        records = []
        for r, path in enumerate(truth):
            by_contig, lines = read_truth_device(eng, r, path, chrkeys, lengths, doc['notes'], phase, chunk_bytes)
            records.append(by_contig)
            doc['truth'][path] = dict(zip(LINE_KEYS, (int(v) for v in lines)), lines_seen=int(lines.sum()))
        with ThreadPoolExecutor(max(int(mo.get('threads') or 1), 1)) as pool:
            for c, ck in enumerate(chrkeys):
                files = merge.find_bed_files(folder, ck, base)
                have = [records[r].get(c) for r in range(R)]
                entry = {'files': files, 'lines_read': 0, 'truth_records': [0 if h is None else int(len(h[0])) for h in have], 'notes': []}
                doc['contigs'][ck] = entry
                if not files and all(h is None for h in have):
                    continue
                t0 = time.perf_counter()
                seq = fasta.get(ck)
                dev.open(ck, len(seq) if seq is not None else None)
                try:
                    entry['lines_read'] = tables.fill(dev, files, pool, ck, len(seq) if seq is not None else MAX_LENGTH, entry['notes'])
                except merge.MergeError as exc:
                    raise BsPerfError(str(exc))
                if seq is None:                                                        # the contig is as long as the largest position seen + 1
                    need = max([dev.plus.length] + [int(h[0].max()) + 1 for h in have if h is not None and len(h[0])])
                    dev.plus.grow(need)
                    dev.minus.grow(need)
                t1 = time.perf_counter()
                phase['merge'] += t1 - t0
                eng.open(c, dev.plus, dev.minus)
                for r, h in enumerate(have):
                    if h is not None:
                        try:
                            eng.fill(r, h[0], h[1])
                        except BsPerfError as exc:
                            raise BsPerfError('%s: %s: %s' % (truth[r], ck, str(exc)[len('bsperf: '):]))
                t2 = time.perf_counter()
                phase['fill'] += t2 - t1
                eng.count()
                t3 = time.perf_counter()
                phase['count'] += t3 - t2
                if model is not None:
                    res = model.sites(dev.plus, dev.minus, seq)
                    n, n_plus = len(res['pos']), int(res['n_plus'])
                    entry['sites'] = int(n)
                    eng.add_scores(res['pos'], (np.arange(n) >= n_plus).astype(np.uint8), res['new'])
                    phase['cluster'] += time.perf_counter() - t3
                eng.close_contig()
                dev.close_contig()
        got = eng.fetch()
        kernel_ms = dict(zip(('parse', 'fill', 'count'), (round(v, 4) for v in eng.times())))
        kernel_ms.update(zip(('merge_parse', 'merge_add'), (round(v, 4) for v in dev.times()[:2])))
    finally:
        if model is not None:
            model.close()
        eng.close()
        dev.close()
    kinds = (0, 1) if model is not None else (0,)
    meas = measures(got, thresholds, R, kinds)
    lines = report_lines(meas)
    doc['lines_seen'] = int(got['lines'].sum())
    doc['lines'] = dict(zip(LINE_KEYS, (int(v) for v in got['lines'])))
    doc['counters'] = {KINDS[k]: {'below_threshold': int(got['below_threshold'][k]), 'untruthed': int(got['untruthed'][k]), 'unpredicted': got['unpredicted'][k].tolist(),
                                  'moments': got['moments'][k].tolist(), 'hist': got['hist'][k].tolist()} for k in kinds}
    doc['axes'] = {'hist': ['label (%s)' % ', '.join(LABELS), 'truth coverage bucket (thresholds <= min coverage, minus one)', 'predicted percentage'],
                   'unpredicted': ['label', 'bucket'], 'moments': ['bucket', 'n, sum x, sum y, sum xy, sum x^2, sum y^2 (y: the sum of the replicates\' percentages)']}
    doc['measures'] = _clean({kind: {str(t): m for t, m in by_t.items()} for kind, by_t in meas.items()})
    doc['kernel_ms'] = kernel_ms
    out_folder = str(mo['outFolder'])
    os.makedirs(out_folder, exist_ok=True)
    stem = os.path.join(out_folder, fileid)
    with open(stem + '_bsperf.txt', 'w') as fh:
        fh.write(''.join(ln + '\n' for ln in lines))
    with open(stem + '_bsperf.json', 'w') as fh:
        json.dump(doc, fh, indent=1)
    for ln in doc['notes'] + lines:
        print(ln, flush=True)
    doc['report'] = lines
    doc['phase_s'] = phase
    return doc
