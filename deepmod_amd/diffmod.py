"""`diffmod`: which sites differ between a run and its controls, and how sure are we?  Per-site differential modification by Fisher's exact test
with Benjamini-Hochberg q-values.  The reference ships no such tool; until now the answer meant exporting the BED files to R.

The test (one run per contig: HostEngine here in exact integers, csrc/diffmod.hip.inc on the GPU).  Options: cov c >= 1, alpha in (0, 1].  One
contig: the sample's '+' and '-' tables (coverage, modified count per position) and the pooled controls'.  For each key (strand s, position p) with
cA, mA of the sample and cB, mB of the controls, the first rule that applies decides:
  1  cA == 0 and cB == 0: ignored, not counted         2  cA < c: shallow_sample         3  cB < c: shallow_control
  4  cA + cB > MAX_TOTAL (2^20): too_deep, counted and noted                               5  tested
A tested key gets the two-sided p of R's fisher.test: with n1 = cA, n2 = cB, M = mA + mB the tables are x in [max(0, M - n2), min(n1, M)], table x
has the weight C(n1, x) C(n2, M - x), and p is the summed weight of the tables whose weight is at most (1 + 1e-7) times the observed table's,
over the weight of all of them.  The engines hand back the counters, the tested keys with p <= alpha as records in key order (ascending
position, '+' before '-') and a 20-bin histogram of the p of every tested key.

Pooling runs before an exact test ignores the variation between replicates: the p-values are those of the pooled counts, and they are smaller
than a replicate-aware (beta-binomial) test would give when replicates disagree.  Such a test, a motif restriction and merging the two strands of
a CpG are out of scope here.

On the host (bh_qvalues): the records of all contigs are sorted by p (stable: ties keep contig, position, strand order), m is the number of
tested keys of the whole run, q_j = min(1, min over k >= j of p_k m / k).  The records with p <= alpha suffice: a q-value is >= its p, and a
q-value <= alpha is a minimum over later ranks that themselves have p <= alpha, whose rank within the subset is their global rank.  A record is
listed iff q <= --fdr and 100 |mA cB - mB cA| >= minDelta cA cB (integers).
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
import re
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib, merge, motifs, siteperf

MAX_TOTAL = 1 << 20
MAX_LENGTH = merge.MAX_LENGTH
COUNT_KEYS = ('tested', 'shallow_sample', 'shallow_control', 'too_deep')
HIST_BINS = 20
FETCH_RUN = 1 << 20                                 # records fetched from the device per call
RECORD_FIELDS = (('pos', np.int32), ('strand', np.uint8), ('cA', np.int32), ('mA', np.int32), ('cB', np.int32), ('mB', np.int32), ('p', np.float64))
HEADER = 'chr\tpos\tstrand\tcovA\tmodA\tpctA\tcovB\tmodB\tpctB\tdelta\tp\tq'


class DiffmodError(ValueError):
    pass


def check_engine_options(cov, alpha) -> None:
    if int(cov) < 1 or int(cov) > 2 ** 31 - 1:
        raise DiffmodError('diffmod: --cov: the least coverage is 1 or more (got %s)' % cov)
    if not 0.0 < float(alpha) <= 1.0:
        raise DiffmodError('diffmod: --fdr: above 0 and at most 1 (got %s)' % alpha)


# ---- the exact test ---------------------------------------------------------------------------------------------------------------------------

def exact_weights(cA: int, mA: int, cB: int, mB: int) -> Tuple[int, List[int]]:
    """-> (the smallest x of the support, the integer weight C(cA, x) C(cB, M - x) of every table from there up)."""
    n1, n2, M = int(cA), int(cB), int(mA) + int(mB)
    lo, hi = max(0, M - n2), min(n1, M)
    w = math.comb(n1, lo) * math.comb(n2, M - lo)
    ws = [w]
    for x in range(lo, hi):
        w = w * (n1 - x) * (M - x) // ((x + 1) * (n2 - M + x + 1))          # exact: the quotient is the next weight
        ws.append(w)
    return lo, ws


@functools.lru_cache(maxsize=1 << 16)
def exact_p(cA: int, mA: int, cB: int, mB: int) -> float:
    """The two-sided p of the module's docstring in exact rationals, rounded once (a p below the float64 range is 0.0)."""
    lo, ws = exact_weights(cA, mA, cB, mB)
    if len(ws) == 1:
        return 1.0
    cut = ws[int(mA) - lo] * (10 ** 7 + 1)
    return min(1.0, sum(w for w in ws if w * 10 ** 7 <= cut) / sum(ws))


def empty_records() -> Dict[str, np.ndarray]:
    return {k: np.zeros(0, t) for k, t in RECORD_FIELDS}


def fates(cov: int, cA, cB) -> np.ndarray:
    """int64 per key: the index into COUNT_KEYS, -1 ignored."""
    cA, cB = np.asarray(cA, np.int64), np.asarray(cB, np.int64)
    f = np.full(len(cA), 0, np.int64)
    f[cA + cB > MAX_TOTAL] = 3
    f[cB < cov] = 2
    f[cA < cov] = 1
    f[(cA <= 0) & (cB <= 0)] = -1
    return f


class HostTables:
    """The two tables of a contig on the host, filled as merge.DeviceMerge fills its own (motifs.HostTables); length None: they grow with the files."""

    def __init__(self, name: str, length: Optional[int]):
        self.name, self.fixed = name, length is not None
        self.length = int(length) if self.fixed else 1
        self.plus = (np.zeros(self.length, np.int64), np.zeros(self.length, np.int64))
        self.minus = (np.zeros(self.length, np.int64), np.zeros(self.length, np.int64))
        self.cov_bound = 0

    def close(self):
        pass

    def add_text(self, text: bytes):
        rec, flag, bad = merge.parse_device_grammar(text, self.name, self.length if self.fixed else -1)
        if not flag:
            self.add_records(*rec)
        return len(rec[0]), flag, bad

    def add_records(self, pos, strand, cov, mod):
        pos, strand, cov, mod = (np.asarray(a).astype(np.int64) for a in (pos, strand, cov, mod))
        if len(pos) == 0:
            return
        if not self.fixed and int(pos.max()) >= self.length:
            self.length = int(pos.max()) + 1
            self.plus = tuple(np.concatenate([a, np.zeros(self.length - len(a), np.int64)]) for a in self.plus)
            self.minus = tuple(np.concatenate([a, np.zeros(self.length - len(a), np.int64)]) for a in self.minus)
        if (pos < 0).any() or (pos >= self.length).any() or (mod < 0).any() or (mod > cov).any():
            raise DiffmodError('diffmod: a record outside the contig or outside 0 <= modified <= coverage')
        self.cov_bound += int(cov.max())
        if self.cov_bound >= 2 ** 31:
            raise DiffmodError('diffmod: the largest coverages of this contig\'s files sum to %d (2^31 or more): the int32 tables cannot hold them' % self.cov_bound)
        for s, tab in enumerate((self.plus, self.minus)):
            sel = strand == s
            np.add.at(tab[0], pos[sel], cov[sel])
            np.add.at(tab[1], pos[sel], mod[sel])


def _padded(tabs):
    tabs = [(np.asarray(t[0]).astype(np.int64), np.asarray(t[1]).astype(np.int64)) for t in tabs]
    n = max(len(t[0]) for t in tabs)
    for t in tabs:
        if len(t[0]) != len(t[1]):
            raise DiffmodError('diffmod: a table with %d coverages and %d modified counts' % (len(t[0]), len(t[1])))
    return [tuple(np.concatenate([a, np.zeros(n - len(a), np.int64)]) for a in t) for t in tabs], n


class HostEngine:
    """The semantics, one contig per run(): numpy for the fates, exact integers for p (slow and correct: the oracle of every test).  A table is a
    pair (coverage, modified) of integer arrays."""

    def __init__(self, cov: int = 5, alpha: float = 0.05):
        check_engine_options(cov, alpha)
        self.cov, self.alpha = int(cov), float(alpha)
        self.reset()

    def close(self):
        pass

    def reset(self):
        self.hist = np.zeros(HIST_BINS, np.int64)
        self.counters = np.zeros((2, len(COUNT_KEYS)), np.int64)

    def new_tables(self, role: str, name: str, length: Optional[int]) -> HostTables:
        return HostTables(name, length)

    def run(self, plus, minus, ctrl_plus, ctrl_minus) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
        """-> (counters [2][4] of this contig, the records with p <= alpha in key order); hist and counters of the engine grow."""
        if ctrl_plus is None or ctrl_minus is None:
            raise DiffmodError('diffmod: the controls are missing (two tables, one per strand)')
        if plus is None or minus is None:
            raise DiffmodError('diffmod: two sample tables, one per strand')
        tabs, n = _padded([plus, minus, ctrl_plus, ctrl_minus])
        counters = np.zeros((2, len(COUNT_KEYS)), np.int64)
        rows = []
        for s in range(2):
            cA, cB = tabs[s][0], tabs[2 + s][0]
            mA, mB = np.clip(tabs[s][1], 0, cA), np.clip(tabs[2 + s][1], 0, cB)
            f = fates(self.cov, cA, cB)
            counters[s] = [int((f == k).sum()) for k in range(len(COUNT_KEYS))]
            for q in np.nonzero(f == 0)[0].tolist():
                p = exact_p(int(cA[q]), int(mA[q]), int(cB[q]), int(mB[q]))
                self.hist[min(HIST_BINS - 1, int(HIST_BINS * p))] += 1
                if p <= self.alpha:
                    rows.append((q, s, int(cA[q]), int(mA[q]), int(cB[q]), int(mB[q]), p))
        rows.sort(key=lambda r: (r[0], r[1]))
        self.counters += counters
        return counters, {k: np.array([r[j] for r in rows], t) for j, (k, t) in enumerate(RECORD_FIELDS)}

    def fetch_hist(self) -> np.ndarray:
        return self.hist.copy()

    def times(self) -> Tuple[float, float]:
        return 0.0, 0.0


def max_total() -> int:
    return _lib.load().dm_diffmod_max_total()


def tile_positions() -> int:
    return _lib.load().dm_diffmod_tile_positions()


def small_support() -> int:
    return _lib.load().dm_diffmod_small_support()


def host_routine(cov, alpha, plus, minus, ctrl_plus, ctrl_minus):
    """The run compiled for the host (dm_diffmod_test_host: the routines the kernels run per key, on the same table of lgamma; no GPU needed)
    -> (counters [2][4], hist [20], records)."""
    lib = _lib.load()
    tabs, n = _padded([plus, minus, ctrl_plus, ctrl_minus])
    arrs = [np.ascontiguousarray(a, np.int32) for t in (tabs[0], tabs[1], tabs[2], tabs[3]) for a in t]
    counters, hist = np.zeros((2, len(COUNT_KEYS)), np.int64), np.zeros(HIST_BINS, np.int64)
    cap = 2 * n
    rec = {k: np.zeros(max(cap, 1), t) for k, t in RECORD_FIELDS}
    got = ctypes.c_int64(0)
    _lib.check(lib.dm_diffmod_test_host(int(cov), float(alpha), n, *[a.ctypes.data for a in arrs], counters.ctypes.data, hist.ctypes.data, cap,
                                        *[rec[k].ctypes.data for k, _ in RECORD_FIELDS], ctypes.byref(got)))
    return counters, hist, {k: v[:got.value].copy() for k, v in rec.items()}


class DeviceEngine(_lib.Handle):
    """The same on one GPU (dm_diffmod_* of the C ABI).  A table is a summary.PositionSummary (the handles merge.DeviceMerge fills).
    times(): ms of the select kernels / of the test kernels so far."""
    PREFIX, N_TIMES = 'dm_diffmod', 2

    def __init__(self, cov: int = 5, alpha: float = 0.05, device: int = 0):
        check_engine_options(cov, alpha)
        self.cov, self.alpha, self.device = int(cov), float(alpha), device
        self._merge = {}
        self._create(device, self.cov, self.alpha)
        self.counters = np.zeros((2, len(COUNT_KEYS)), np.int64)
        self.n_records = 0

    def close(self):
        for dm in getattr(self, '_merge', {}).values():
            dm.close()
        self._merge = {}
        super().close()

    def new_tables(self, role: str, name: str, length: Optional[int]):
        """Fresh tables for the contig in the merge handle kept for `role` (the tables of the contig before are closed); length None: they grow."""
        if role not in self._merge:
            self._merge[role] = merge.DeviceMerge(self.device)
        self._merge[role].open(name, None if length is None else int(length))
        return self._merge[role]

    def run(self, plus, minus, ctrl_plus, ctrl_minus, fetch_run: int = FETCH_RUN) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
        tabs = [plus, minus, ctrl_plus, ctrl_minus]
        if all(t is not None for t in tabs):
            n = max(t.length for t in tabs)
            for t in tabs:
                if t.length < n:                                      # tables that grew with their files: to one length
                    t.grow(n)
        counters, got = np.zeros((2, len(COUNT_KEYS)), np.int64), ctypes.c_int64(0)
        self._libmod.check(self._lib.dm_diffmod_run(self._h, *[None if t is None else t._h for t in tabs], counters.ctypes.data, ctypes.byref(got)))
        self.counters += counters
        self.n_records = got.value
        return counters, self.fetch_records(0, self.n_records, fetch_run)

    def fetch_records(self, first: int, count: int, fetch_run: int = FETCH_RUN) -> Dict[str, np.ndarray]:
        """Records first .. first + count - 1 of the last run, fetched in runs of fetch_run at most."""
        rec = {k: np.zeros(count, t) for k, t in RECORD_FIELDS}
        for lo in range(0, count, max(int(fetch_run), 1)):
            n = min(int(fetch_run), count - lo)
            self._libmod.check(self._lib.dm_diffmod_fetch_records(self._h, first + lo, n, *[rec[k][lo:lo + n].ctypes.data for k, _ in RECORD_FIELDS]))
        return rec

    def fetch_hist(self) -> np.ndarray:
        hist = np.zeros(HIST_BINS, np.int64)
        self._libmod.check(self._lib.dm_diffmod_fetch_hist(self._h, hist.ctypes.data))
        return hist

    def reset(self):
        self._libmod.check(self._lib.dm_diffmod_reset(self._h))
        self.counters[:] = 0
        self.n_records = 0


# ---- q-values -----------------------------------------------------------------------------------------------------------------------------------

def bh_qvalues(p, m: int) -> np.ndarray:
    """Benjamini-Hochberg q-values of the p-values p (any order) among m tests, m >= len(p): with the p sorted ascending (stable),
    q_j = min(1, min over k >= j of p_k m / k); returned in the order of p."""
    p = np.asarray(p, np.float64)
    n = len(p)
    if int(m) < n:
        raise DiffmodError('diffmod: %d p-values among %d tests' % (n, int(m)))
    order = np.argsort(p, kind='stable')
    ranked = p[order] * float(int(m)) / np.arange(1, n + 1, dtype=np.float64)
    q = np.empty(n, np.float64)
    q[order] = np.minimum(1.0, np.minimum.accumulate(ranked[::-1])[::-1])
    return q


def delta_passes(cA, mA, cB, mB, min_delta: int) -> np.ndarray:
    """100 |mA cB - mB cA| >= min_delta cA cB in int64: the percentages differ by min_delta points or more."""
    cA, mA, cB, mB = (np.asarray(a, np.int64) for a in (cA, mA, cB, mB))
    return 100 * np.abs(mA * cB - mB * cA) >= int(min_delta) * cA * cB


# ---- the command --------------------------------------------------------------------------------------------------------------------------------

def _contigs_of(folder: str, base: str) -> List[str]:
    found = set()
    for path in motifs._stranded_beds(folder, base):
        found.add(re.search(r'\.([^/.]*)[+-]\.%s\.bed$' % re.escape(base), path).group(1))
    return sorted(found)


def check_options(mo: Dict[str, object]):
    """What can be refused before a BED file is read or any GPU asked for -> (options dict, contigs, {contig: length or None}, {contig: sample
    files}, {contig: control files})."""
    base = str(mo.get('Base') or 'C')
    try:
        o = {'Base': base, 'cov': int(mo.get('cov', 5)), 'fdr': float(mo.get('fdr', 0.05)), 'minDelta': int(mo.get('minDelta', 10)), 'all': int(mo.get('all') or 0)}
    except (TypeError, ValueError) as exc:
        raise DiffmodError('diffmod: %s' % exc)
    if len(base) != 1 or base not in 'ACGT':
        raise DiffmodError('diffmod: --Base: one of A, C, G, T (got %r)' % (base,))
    check_engine_options(o['cov'], o['fdr'])
    if not 0 <= o['minDelta'] <= 100:
        raise DiffmodError('diffmod: --minDelta: percentage points, 0 to 100 (got %d)' % o['minDelta'])
    if o['all'] not in (0, 1):
        raise DiffmodError('diffmod: --all: 0 or 1 (got %d)' % o['all'])
    folder = mo.get('predFolder')
    if not folder or not os.path.isdir(folder):
        raise DiffmodError('diffmod: --predFolder: the folder of the sample\'s runs does not exist (%s)' % folder)
    controls = [c for c in (mo.get('control') or []) if c]
    if not controls:
        raise DiffmodError('diffmod: --control: the folder(s) of the control runs are needed (the test is of the sample against them)')
    for c in controls:
        if not os.path.isdir(c):
            raise DiffmodError('diffmod: --control: no folder %s' % c)
    ref = mo.get('Ref')
    if ref and not os.path.isfile(ref):
        raise DiffmodError('diffmod: --Ref: reference file does not exist (%s)' % ref)
    fasta = siteperf.read_fasta(ref) if ref else {}
    named = list(mo.get('chr') or [])
    if ref:
        missing = [ck for ck in named if ck not in fasta]
        if missing:
            raise DiffmodError('diffmod: --chr: %s holds no contig %s' % (ref, ', '.join(missing)))
    chrkeys = named or list(fasta) or _contigs_of(folder, base)
    lengths = {ck: (len(fasta[ck]) if ck in fasta else None) for ck in chrkeys}
    for ck in chrkeys:
        if lengths[ck] is not None and not 1 <= lengths[ck] <= MAX_LENGTH:
            raise DiffmodError('diffmod: --Ref: contig %s has %d bases (1 to 2^31 - 1)' % (ck, lengths[ck]))
    files = {ck: sorted(merge.find_bed_files(folder, ck, base)) for ck in chrkeys}          # (sorted: the order of the notes)
    ctrl_files = {ck: [p for c in controls for p in sorted(merge.find_bed_files(c, ck, base))] for ck in chrkeys}
    if not any(files.values()):
        raise DiffmodError('diffmod: --predFolder: no *.<chr>+.%s.bed / *.<chr>-.%s.bed one to three levels below %s' % (base, base, folder))
    if not any(ctrl_files.values()):
        raise DiffmodError('diffmod: --control: no *.<chr>+.%s.bed / *.<chr>-.%s.bed one to three levels below %s' % (base, base, ', '.join(controls)))
    return o, chrkeys, lengths, files, ctrl_files


def _read_into(tables, path: str, text: bytes, name: str, length: Optional[int], notes: List[str]) -> int:
    """One file into the tables, as merge_runs adds it: the device grammar first, the host parse for a text outside it.  -> lines added"""
    lines, flag, bad = tables.add_text(text)
    if flag:
        notes.append('%s: line %d is outside the device grammar: the file is parsed on the host' % (path, bad))
        try:
            rec = merge.host_rows(path, name, MAX_LENGTH if length is None else length)      # MergeError: `file:line: reason`
        except merge.MergeError as exc:
            raise DiffmodError('diffmod: %s' % exc)
        tables.add_records(*rec)
        lines = len(rec[0])
    return int(lines)


def report_text(rows) -> str:
    """rows: (chr, pos, strand 0 / 1, cA, mA, cB, mB, p, q) -> the header and one line per row."""
    out = [HEADER]
    for ck, pos, s, cA, mA, cB, mB, p, q in rows:
        out.append('%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t%.6e\t%.6e' % (ck, pos, '+-'[s], cA, mA, 100 * mA // cA, cB, mB, 100 * mB // cB,
                                                                              100.0 * mA / cA - 100.0 * mB / cB, p, q))
    return ''.join(r + '\n' for r in out)


def diffmod(mo: Dict[str, object], engine=None) -> Dict[str, object]:
    """The command.  mo: predFolder, control (list of folders), Base, outFolder, FileID, chr (list; None: the contigs of --Ref, or without it those
    the sample's file names hold), Ref (None: the tables grow with the files), cov, fdr, minDelta, all, threads.  engine: an object with
    HostEngine's interface (default: DeviceEngine on GPU 0), made with cov and alpha = fdr (1 under all).  Writes
    <outFolder>/<FileID>_diffmod.txt / _diffmod.json -> the JSON document."""
    import json
    from concurrent.futures import ThreadPoolExecutor
    o, chrkeys, lengths, files, ctrl_files = check_options(mo)
    alpha = 1.0 if o['all'] else o['fdr']
    controls = [c for c in (mo.get('control') or []) if c]
    own = engine is None
    if own:
        if _lib.load().dm_device_count() < 1:
            raise DiffmodError('no gfx950 GPU visible (this build has no CPU path)')
        engine = DeviceEngine(o['cov'], alpha)
    elif (engine.cov, engine.alpha) != (o['cov'], alpha):
        raise DiffmodError('diffmod: the engine was made for cov %d alpha %g' % (engine.cov, engine.alpha))

    def read(path):
        with open(path, 'rb') as fh:
            return fh.read()

    notes: List[str] = []
    doc = {'inputs': dict(o, predFolder=mo['predFolder'], control=controls, Ref=mo.get('Ref'), chr=chrkeys, FileID=str(mo.get('FileID') or 'mod'),
                          files=[p for ck in chrkeys for p in files[ck]], control_files=[p for ck in chrkeys for p in ctrl_files[ck]]),
           'contigs': {}}
    per_contig = []
    try:
        engine.reset()
        with ThreadPoolExecutor(max(int(mo.get('threads') or 1), 1)) as pool:
            for ck in chrkeys:
                if not files[ck] and not ctrl_files[ck]:
                    continue
                entry = {'length': lengths[ck], 'files': len(files[ck]), 'control_files': len(ctrl_files[ck]), 'lines_read': 0, 'control_lines_read': 0}
                tabs = []
                for role, paths, key in (('sample', files[ck], 'lines_read'), ('control', ctrl_files[ck], 'control_lines_read')):
                    t = engine.new_tables(role, ck, lengths[ck])
                    for path, text in zip(paths, pool.map(read, paths)):          # the threads read ahead
                        try:
                            entry[key] += _read_into(t, path, text, ck, lengths[ck], notes)
                        except DiffmodError:
                            raise
                        except (ValueError, RuntimeError) as exc:                 # the tables' own refusals (a coverage sum past int32)
                            raise DiffmodError('diffmod: %s: %s' % (path, exc))
                    tabs.extend([t.plus, t.minus])
                counters, rec = engine.run(*tabs)
                for s, strand in enumerate('+-'):
                    entry[strand] = dict(zip(COUNT_KEYS, (int(v) for v in counters[s])))
                    if counters[s][3]:
                        notes.append('%s %s: %d keys with a pooled coverage above %d were not tested' % (ck, strand, int(counters[s][3]), MAX_TOTAL))
                doc['contigs'][ck] = entry
                per_contig.append((ck, rec))
        hist = engine.fetch_hist()
        times = engine.times()
    finally:
        if own:
            engine.close()
    m = int(sum(doc['contigs'][ck][s]['tested'] for ck in doc['contigs'] for s in '+-'))
    p_all = np.concatenate([rec['p'] for _, rec in per_contig]) if per_contig else np.zeros(0)
    q_all = bh_qvalues(p_all, m)
    rows, hyper, hypo, at = [], 0, 0, 0
    for ck, rec in per_contig:
        n = len(rec['p'])
        q = q_all[at:at + n]
        at += n
        cA, mA, cB, mB = (rec[k].astype(np.int64) for k in ('cA', 'mA', 'cB', 'mB'))
        keep = np.ones(n, bool) if o['all'] else (q <= o['fdr']) & delta_passes(cA, mA, cB, mB, o['minDelta'])
        sign = np.sign(mA * cB - mB * cA)
        for s, strand in enumerate('+-'):
            doc['contigs'][ck][strand]['listed'] = int((keep & (rec['strand'] == s)).sum())
        hyper += int((keep & (sign > 0)).sum())
        hypo += int((keep & (sign < 0)).sum())
        for i in np.nonzero(keep)[0].tolist():
            rows.append((ck, int(rec['pos'][i]), int(rec['strand'][i]), int(cA[i]), int(mA[i]), int(cB[i]), int(mB[i]), float(rec['p'][i]), float(q[i])))
    if m == 0:
        notes.append('no key had --cov %d reads in both the sample and the controls' % o['cov'])
    doc['m'] = m
    doc['listed'], doc['hyper'], doc['hypo'] = len(rows), hyper, hypo
    doc['p_histogram'] = [int(v) for v in hist]
    doc['notes'] = notes
    doc['times'] = {'select_ms': round(times[0], 4), 'fisher_ms': round(times[1], 4)}
    out_folder = str(mo['outFolder'])
    os.makedirs(out_folder, exist_ok=True)
    prefix = os.path.join(out_folder, doc['inputs']['FileID'])
    with open(prefix + '_diffmod.txt', 'w') as fh:
        fh.write(report_text(rows))
    with open(prefix + '_diffmod.json', 'w') as fh:
        json.dump(doc, fh, indent=1)
    for ln in notes:
        print(ln, flush=True)
    print('diffmod: %d keys tested, %d listed (%d above the controls, %d below) -> %s_diffmod.txt' % (m, len(rows), hyper, hypo, prefix), flush=True)
    return doc
