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
than a replicate-aware test gives when replicates disagree.  --replicates 1 is that test: every folder a replicate, a quasi-binomial F test per
key (RepHostEngine below, csrc/diffrep.hip.inc on the GPU).  A motif restriction and merging the two strands of a CpG are out of
scope in both.

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
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib, merge, tables

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

    def new_tables(self, role: str, name: str, length: Optional[int]) -> tables.HostTables:
        return tables.HostTables(name, length)

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


def _to_one_length(tabs) -> None:
    """Device tables that grew with their files: to one length."""
    if tabs and all(t is not None for t in tabs):
        n = max(t.length for t in tabs)
        for t in tabs:
            if t.length < n:
                t.grow(n)


class DeviceEngine(tables.MergeHandles, _lib.Handle):
    """The same on one GPU (dm_diffmod_* of the C ABI).  A table is a summary.PositionSummary (the handles merge.DeviceMerge fills).
    times(): ms of the select kernels / of the test kernels so far."""
    PREFIX, N_TIMES, FIELDS = 'dm_diffmod', 2, RECORD_FIELDS

    def __init__(self, cov: int = 5, alpha: float = 0.05, device: int = 0):
        self._made(device, cov, alpha)

    def _made(self, device: int, cov, alpha, *more):
        check_engine_options(cov, alpha)
        self.cov, self.alpha, self.device = int(cov), float(alpha), device
        self._create(device, self.cov, self.alpha, *more)
        self.counters = np.zeros((2, len(COUNT_KEYS)), np.int64)
        self.n_records = 0

    def _run(self, fetch_run: int, *args) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
        counters, got = np.zeros((2, len(COUNT_KEYS)), np.int64), ctypes.c_int64(0)
        self._libmod.check(self._fn('run')(self._h, *args, counters.ctypes.data, ctypes.byref(got)))
        self.counters += counters
        self.n_records = got.value
        return counters, self.fetch_records(0, self.n_records, fetch_run)

    def run(self, plus, minus, ctrl_plus, ctrl_minus, fetch_run: int = FETCH_RUN) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
        tabs = [plus, minus, ctrl_plus, ctrl_minus]
        _to_one_length(tabs)
        return self._run(fetch_run, *[None if t is None else t._h for t in tabs])

    def fetch_records(self, first: int, count: int, fetch_run: int = FETCH_RUN) -> Dict[str, np.ndarray]:
        """Records first .. first + count - 1 of the last run, fetched in runs of fetch_run at most."""
        rec = {k: np.zeros(count, t) for k, t in self.FIELDS}
        for lo in range(0, count, max(int(fetch_run), 1)):
            n = min(int(fetch_run), count - lo)
            self._libmod.check(self._fn('fetch_records')(self._h, first + lo, n, *[rec[k][lo:lo + n].ctypes.data for k, _ in self.FIELDS]))
        return rec

    def fetch_hist(self) -> np.ndarray:
        hist = np.zeros(HIST_BINS, np.int64)
        self._libmod.check(self._fn('fetch_hist')(self._h, hist.ctypes.data))
        return hist

    def reset(self):
        self._libmod.check(self._fn('reset')(self._h))
        self.counters[:] = 0
        self.n_records = 0


# ---- the replicate-aware test (--replicates 1) ------------------------------------------------------------------------------------
# Quasi-binomial F test of a two-group logistic model, the McCullagh-Nelder overdispersion correction, in closed form.  Every folder of --predFolder
# is one sample replicate (KA of them), every folder of --control one control replicate (KB), 1..8 each and 3 or more together.  A key is (strand,
# position); a modified count is first held to 0..coverage; replicate i is used at the key iff c_i >= cov; nA, nB are the used replicates of either
# group, C_g and M_g the sums of c and m over them.  The first rule that applies decides:
#   1  every c_i == 0: ignored       2  nA < a: shallow_sample       3  nB < b: shallow_control       4  C_A + C_B > MAX_TOTAL: too_deep       5  tested
# with (a, b) = --minReps (default KA, KB).  A tested key: nu = nA + nB - 2, C = C_A + C_B, M = M_A + M_B.  M_A C_B == M_B C_A: p = 1, phi = 1.  Else
#   h(M, C) = M ln(M / C) + (C - M) ln((C - M) / C)  (a term whose factor is 0 is 0),      D = max(0, 2 [h(M_A, C_A) + h(M_B, C_B) - h(M, C)]),
#   X2 = sum over groups and used i of r_i^2 / (c_i M_g (C_g - M_g)),  r_i = m_i C_g - c_i M_g  (a group with M_g in {0, C_g} adds 0),
#   phi = max(1, X2 / nu),  F = D / phi,  p = I_x(nu / 2, 1 / 2) at x = nu / (nu + F): the regularized incomplete beta, P(F(1, nu) >= F).
# A record carries the sums over the used replicates as cA, mA, cB, mB, then nA, nB, phi and p.

MAX_REPS = 8
REP_RECORD_FIELDS = RECORD_FIELDS[:6] + (('nA', np.uint8), ('nB', np.uint8), ('phi', np.float64), ('p', np.float64))
REP_HEADER = 'chr\tpos\tstrand\tcovA\tmodA\tpctA\tcovB\tmodB\tpctB\tdelta\trepA\trepB\tphi\tp\tq'
REP_DIGITS = 50
_PI = '3.14159265358979323846264338327950288419716898596868385569518'


def check_rep_counts(n_a, n_b, min_a, min_b) -> None:
    if not (1 <= int(n_a) <= MAX_REPS and 1 <= int(n_b) <= MAX_REPS):
        raise DiffmodError('diffmod: --replicates 1: 1 to %d folders in --predFolder and in --control (got %d and %d)' % (MAX_REPS, n_a, n_b))
    if int(n_a) + int(n_b) < 3:
        raise DiffmodError('diffmod: --replicates 1: 3 or more replicates together (got %d and %d): no variation between replicates can be seen in fewer' % (n_a, n_b))
    if not (1 <= int(min_a) <= int(n_a) and 1 <= int(min_b) <= int(n_b) and int(min_a) + int(min_b) >= 3):
        raise DiffmodError('diffmod: --minReps: a,b with 1 <= a <= %d, 1 <= b <= %d and a + b >= 3 (got %d,%d)' % (n_a, n_b, min_a, min_b))


def _rep_context():
    import decimal
    return decimal.Context(prec=REP_DIGITS, Emin=-999999, Emax=999999)


def rep_beta(nu: int):
    """B(nu / 2, 1 / 2) as a decimal: a rational for even nu, a rational times pi for odd nu."""
    import decimal
    from fractions import Fraction
    ctx = _rep_context()
    k = int(nu) // 2
    half = Fraction(math.factorial(2 * k), 4 ** k * math.factorial(k))                    # Gamma(k + 1/2) / sqrt(pi)
    if nu % 2 == 0:
        b = Fraction(math.factorial(k - 1)) / half                                        # Gamma(k) sqrt(pi) / Gamma(k + 1/2)
        return ctx.divide(decimal.Decimal(b.numerator), decimal.Decimal(b.denominator))
    b = half / math.factorial(k)                                                          # Gamma(k + 1/2) sqrt(pi) / Gamma(k + 1), over pi
    return ctx.multiply(ctx.divide(decimal.Decimal(b.numerator), decimal.Decimal(b.denominator)), decimal.Decimal(_PI))


def rep_tail(nu: int, F):
    """P(F(1, nu) >= F) = I_x(nu / 2, 1 / 2) at x = nu / (nu + F), as a 50-digit decimal: the hypergeometric series
    I_x(a, b) = x^a (1 - x)^b / (a B(a, b)) sum over n of x^n (a + b)_n / (a + 1)_n for x <= 1/2, and 1 - I_(1-x)(b, a) by the same series above."""
    import decimal
    ctx = _rep_context()
    D = decimal.Decimal
    F = D(F) if not isinstance(F, decimal.Decimal) else F
    if F <= 0:
        return D(1)
    den = ctx.add(D(int(nu)), F)
    x, y = ctx.divide(D(int(nu)), den), ctx.divide(F, den)
    rx, ry = ctx.sqrt(x), ctx.sqrt(y)

    def series(a2, b2, z):                                            # sum of z^n (a2 / 2)_n / (b2 / 2)_n
        t = s = D(1)
        n = 0
        while True:
            t = ctx.divide(ctx.multiply(ctx.multiply(t, z), D(a2 + 2 * n)), D(b2 + 2 * n))
            s = ctx.add(s, t)
            n += 1
            if t < s.scaleb(-(REP_DIGITS + 4)):
                return s

    front = ctx.divide(ctx.multiply(ctx.power(rx, int(nu)), ry), rep_beta(nu))              # x^a (1 - x)^(1/2) / B
    if x <= D('0.5'):
        return ctx.divide(ctx.multiply(ctx.multiply(front, D(2)), series(nu + 1, nu + 2, x)), D(int(nu)))
    return ctx.subtract(D(1), ctx.multiply(ctx.multiply(front, D(2)), series(nu + 1, 3, y)))


def rep_fate(cov: int, min_a: int, min_b: int, c_a, m_a, c_b, m_b):
    """The fate of a key from the counts of its replicates as the tables hold them -> (index into COUNT_KEYS or -1 for ignored, the used (c, m) of
    the sample, those of the controls), modified counts held to 0..coverage."""
    groups = []
    for cs, ms in ((c_a, m_a), (c_b, m_b)):
        cs = [max(int(c), 0) for c in cs]
        groups.append([(c, min(max(int(m), 0), c)) for c, m in zip(cs, ms)])
    if not any(c for g in groups for c, _ in g):
        return -1, [], []
    used = [[(c, m) for c, m in g if c >= cov] for g in groups]
    if len(used[0]) < min_a:
        return 1, used[0], used[1]
    if len(used[1]) < min_b:
        return 2, used[0], used[1]
    if sum(c for g in used for c, _ in g) > MAX_TOTAL:
        return 3, used[0], used[1]
    return 0, used[0], used[1]


def rep_deviance(MA: int, CA: int, MB: int, CB: int):
    """D of the contract as a 50-digit decimal."""
    import decimal
    ctx = _rep_context()
    D = decimal.Decimal

    def h(M, C):
        v = D(0)
        for k in (M, C - M):
            if k > 0:
                v = ctx.add(v, ctx.multiply(D(k), ctx.ln(ctx.divide(D(k), D(C)))))
        return v

    d = ctx.multiply(D(2), ctx.subtract(ctx.add(h(MA, CA), h(MB, CB)), h(MA + MB, CA + CB)))
    return max(d, D(0))


@functools.lru_cache(maxsize=1 << 16)
def rep_exact(used_a: tuple, used_b: tuple) -> dict:
    """The test of one tested key from its used replicates ((c, m), ..) of either group -> {'cA', 'mA', 'cB', 'mB', 'nA', 'nB', 'nu', 'equal',
    'D', 'phi', 'p'}: integers, and 50-digit decimals for D, phi and p."""
    import decimal
    from fractions import Fraction
    ctx = _rep_context()
    CA, MA = sum(c for c, _ in used_a), sum(m for _, m in used_a)
    CB, MB = sum(c for c, _ in used_b), sum(m for _, m in used_b)
    nu = len(used_a) + len(used_b) - 2
    out = {'cA': CA, 'mA': MA, 'cB': CB, 'mB': MB, 'nA': len(used_a), 'nB': len(used_b), 'nu': nu, 'equal': MA * CB == MB * CA}
    if out['equal']:
        out.update(D=decimal.Decimal(0), phi=decimal.Decimal(1), p=decimal.Decimal(1))
        return out
    x2 = Fraction(0)
    for used, Cg, Mg in ((used_a, CA, MA), (used_b, CB, MB)):
        if 0 < Mg < Cg:
            x2 += sum(Fraction((m * Cg - c * Mg) ** 2, c * Mg * (Cg - Mg)) for c, m in used)
    phi = max(Fraction(1), x2 / nu)
    phi = ctx.divide(decimal.Decimal(phi.numerator), decimal.Decimal(phi.denominator))
    d = rep_deviance(MA, CA, MB, CB)
    out.update(D=d, phi=phi, p=rep_tail(nu, ctx.divide(d, phi)))
    return out


def rep_exact_p(used_a, used_b) -> float:
    """p of a tested key from its used replicates ((c, m), ..) of either group, rounded once."""
    return float(rep_exact(tuple(map(tuple, used_a)), tuple(map(tuple, used_b)))['p'])


def empty_rep_records() -> Dict[str, np.ndarray]:
    return {k: np.zeros(0, t) for k, t in REP_RECORD_FIELDS}


class RepHostEngine(HostEngine):
    """The semantics of --replicates 1, one contig per run(): integers for the fates and r_i, decimals at 50 digits for ln and the incomplete beta
    (slow and correct: the oracle of every test; standard library and numpy only).  A table is a pair (coverage, modified) of integer arrays."""

    def __init__(self, cov: int = 5, alpha: float = 0.05, min_a: int = 1, min_b: int = 2):
        check_engine_options(cov, alpha)
        if not (1 <= int(min_a) <= MAX_REPS and 1 <= int(min_b) <= MAX_REPS and int(min_a) + int(min_b) >= 3):
            raise DiffmodError('diffmod: --minReps: a,b of 1 to %d each and 3 or more together (got %s,%s)' % (MAX_REPS, min_a, min_b))
        self.cov, self.alpha, self.min_a, self.min_b = int(cov), float(alpha), int(min_a), int(min_b)
        self.reset()

    def run(self, sample, control) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
        """sample, control: [(plus, minus), ..], one pair of tables per replicate -> (counters [2][4] of this contig, the records with p <= alpha in
        key order); hist and counters of the engine grow."""
        n_a, n_b = len(sample), len(control)
        check_rep_counts(n_a, n_b, self.min_a, self.min_b)
        counters = np.zeros((2, len(COUNT_KEYS)), np.int64)
        rows = []
        for s in range(2):
            tabs, n = _padded([rep[s] for rep in list(sample) + list(control)])
            cs, ms = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
            for q in np.nonzero((cs > 0).any(axis=0))[0].tolist():
                c, m = cs[:, q].tolist(), ms[:, q].tolist()
                f, ua, ub = rep_fate(self.cov, self.min_a, self.min_b, c[:n_a], m[:n_a], c[n_a:], m[n_a:])
                counters[s, f] += 1
                if f != 0:
                    continue
                e = rep_exact(tuple(ua), tuple(ub))
                p = float(e['p'])
                self.hist[min(HIST_BINS - 1, int(HIST_BINS * p))] += 1
                if p <= self.alpha:
                    rows.append((q, s, e['cA'], e['mA'], e['cB'], e['mB'], e['nA'], e['nB'], float(e['phi']), p))
        rows.sort(key=lambda r: (r[0], r[1]))
        self.counters += counters
        return counters, {k: np.array([r[j] for r in rows], t) for j, (k, t) in enumerate(REP_RECORD_FIELDS)}


def max_replicates() -> int:
    return _lib.load().dm_diffrep_max_replicates()


def rep_host_routine(cov, alpha, min_a, min_b, sample, control):
    """The run compiled for the host (dm_diffrep_test_host: the routine the kernel runs per key; no GPU needed).  sample, control: [(plus, minus),
    ..] -> (counters [2][4], hist [20], records)."""
    lib = _lib.load()
    reps = list(sample) + list(control)
    tabs, n = _padded([rep[s] for rep in reps for s in range(2)])                        # replicate j: '+' at 2 j, '-' at 2 j + 1
    arrs = [[np.ascontiguousarray(a, np.int32) for a in t] for t in tabs]
    ptrs = [(ctypes.c_void_p * len(reps))(*[arrs[2 * j + s][col].ctypes.data for j in range(len(reps))]) for s in range(2) for col in range(2)]
    counters, hist = np.zeros((2, len(COUNT_KEYS)), np.int64), np.zeros(HIST_BINS, np.int64)
    cap = 2 * n
    rec = {k: np.zeros(max(cap, 1), t) for k, t in REP_RECORD_FIELDS}
    got = ctypes.c_int64(0)
    _lib.check(lib.dm_diffrep_test_host(int(cov), float(alpha), int(min_a), int(min_b), len(sample), len(control), n, *ptrs, counters.ctypes.data, hist.ctypes.data, cap,
                                        *[rec[k].ctypes.data for k, _ in REP_RECORD_FIELDS], ctypes.byref(got)))
    return counters, hist, {k: v[:got.value].copy() for k, v in rec.items()}


class RepDeviceEngine(DeviceEngine):
    """The same on one GPU (dm_diffrep_* of the C ABI): one merge.DeviceMerge per replicate (new_tables with a role per replicate); the sweep reads
    16 bytes per position and replicate.  times(): ms of the counting pass / of the writing pass so far."""
    PREFIX, N_TIMES, FIELDS = 'dm_diffrep', 2, REP_RECORD_FIELDS

    def __init__(self, cov: int = 5, alpha: float = 0.05, min_a: int = 1, min_b: int = 2, device: int = 0):
        self.min_a, self.min_b = int(min_a), int(min_b)
        self._made(device, cov, alpha, self.min_a, self.min_b)

    def run(self, sample, control, fetch_run: int = FETCH_RUN) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
        """sample, control: [(plus, minus), ..] of summary.PositionSummary, one pair per replicate."""
        reps = list(sample) + list(control)
        _to_one_length([t for rep in reps for t in rep])
        plus = (ctypes.c_void_p * max(len(reps), 1))(*[None if rep[0] is None else rep[0]._h for rep in reps])
        minus = (ctypes.c_void_p * max(len(reps), 1))(*[None if rep[1] is None else rep[1]._h for rep in reps])
        return self._run(fetch_run, len(sample), len(control), plus, minus)


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

def _scalar_options(mo: Dict[str, object]) -> Dict[str, object]:
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
    return o


def _contigs(mo: Dict[str, object], base: str, folders: List[str]):
    """-> (contigs, {contig: length or None}) from --Ref and --chr, or from the file names below `folders`."""
    try:
        return tables.contigs(mo.get('Ref'), mo.get('chr'), base, folders)[:2]
    except tables.TableError as exc:
        raise DiffmodError('diffmod: %s' % exc)


def _folders_exist(option: str, folders: List[str]) -> None:
    for f in folders:
        if not os.path.isdir(f):
            raise DiffmodError('diffmod: %s: no folder %s' % (option, f))


def _no_beds(option: str, base: str, below: str) -> DiffmodError:
    return DiffmodError('diffmod: %s: no *.<chr>+.%s.bed / *.<chr>-.%s.bed one to three levels below %s' % (option, base, base, below))


def check_options(mo: Dict[str, object]):
    """What can be refused before a BED file is read or any GPU asked for -> (options dict, contigs, {contig: length or None}, {contig: sample
    files}, {contig: control files})."""
    o = _scalar_options(mo)
    base = o['Base']
    folder = mo.get('predFolder')
    if not folder or not os.path.isdir(folder):
        raise DiffmodError('diffmod: --predFolder: the folder of the sample\'s runs does not exist (%s)' % folder)
    controls = [c for c in (mo.get('control') or []) if c]
    if not controls:
        raise DiffmodError('diffmod: --control: the folder(s) of the control runs are needed (the test is of the sample against them)')
    _folders_exist('--control', controls)
    chrkeys, lengths = _contigs(mo, base, [folder])
    files = {ck: sorted(merge.find_bed_files(folder, ck, base)) for ck in chrkeys}          # (sorted: the order of the notes)
    ctrl_files = {ck: [p for c in controls for p in sorted(merge.find_bed_files(c, ck, base))] for ck in chrkeys}
    if not any(files.values()):
        raise _no_beds('--predFolder', base, folder)
    if not any(ctrl_files.values()):
        raise _no_beds('--control', base, ', '.join(controls))
    return o, chrkeys, lengths, files, ctrl_files


def check_rep_options(mo: Dict[str, object]):
    """The same for --replicates 1 -> (options dict with `replicates` and `minReps`, contigs, lengths, {contig: [files of sample replicate 0, ..]},
    {contig: [files of control replicate 0, ..]})."""
    o = _scalar_options(mo)
    base = o['Base']
    pred = mo.get('predFolder') or []
    samples = [f for f in (pred.split(',') if isinstance(pred, str) else list(pred)) if f]
    controls = [c for c in (mo.get('control') or []) if c]
    if not samples:
        raise DiffmodError('diffmod: --predFolder: the folders of the sample replicates are needed, separated by commas')
    if not controls:
        raise DiffmodError('diffmod: --control: the folder(s) of the control replicates are needed (the test is of the sample against them)')
    min_reps = mo.get('minReps')
    try:
        a, b = (len(samples), len(controls)) if min_reps in (None, '') else (int(v) for v in (min_reps.split(',') if isinstance(min_reps, str) else min_reps))
    except (TypeError, ValueError):
        raise DiffmodError('diffmod: --minReps: two integers a,b (got %r)' % (min_reps,))
    check_rep_counts(len(samples), len(controls), a, b)
    seen = {}
    for option, folders in (('--predFolder', samples), ('--control', controls)):
        for f in folders:
            _folders_exist(option, [f])
            real = os.path.realpath(f)
            if real in seen:
                raise DiffmodError('diffmod: %s: the folder %s is named twice (in %s and in %s): a replicate is one folder of its own' % (option, f, seen[real], option))
            seen[real] = option
    chrkeys, lengths = _contigs(mo, base, samples)
    files = {ck: [sorted(merge.find_bed_files(f, ck, base)) for f in samples] for ck in chrkeys}
    ctrl_files = {ck: [sorted(merge.find_bed_files(c, ck, base)) for c in controls] for ck in chrkeys}
    for option, folders, found in (('--predFolder', samples, files), ('--control', controls, ctrl_files)):
        for j, f in enumerate(folders):
            if not any(found[ck][j] for ck in chrkeys):
                raise _no_beds(option, base, f)
    return dict(o, replicates={'sample': samples, 'control': controls}, minReps=[a, b]), chrkeys, lengths, files, ctrl_files


def _report_text(header: str, rows, middle: str = '') -> str:
    out = [header]
    for ck, pos, s, cA, mA, cB, mB, *rest in rows:
        out.append(('%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.2f\t' + middle + '%.6e\t%.6e') %
                   ((ck, pos, '+-'[s], cA, mA, 100 * mA // cA, cB, mB, 100 * mB // cB, 100.0 * mA / cA - 100.0 * mB / cB) + tuple(rest)))
    return ''.join(r + '\n' for r in out)


def report_text(rows) -> str:
    """rows: (chr, pos, strand 0 / 1, cA, mA, cB, mB, p, q) -> the header and one line per row."""
    return _report_text(HEADER, rows)


def rep_report_text(rows) -> str:
    """rows: (chr, pos, strand 0 / 1, cA, mA, cB, mB, nA, nB, phi, p, q) -> the header and one line per row."""
    return _report_text(REP_HEADER, rows, '%d\t%d\t%.4f\t')


def replicates_option(mo: Dict[str, object]) -> int:
    """--replicates, 0 or 1; --minReps belongs to 1 alone."""
    try:
        rep = int(mo.get('replicates') or 0)
    except (TypeError, ValueError):
        rep = -1
    if rep not in (0, 1):
        raise DiffmodError('diffmod: --replicates: 0 or 1 (got %s)' % (mo.get('replicates'),))
    if not rep and mo.get('minReps') not in (None, ''):
        raise DiffmodError('diffmod: --minReps: only with --replicates 1 (pooled runs have no replicates to count)')
    return rep


# what the two tests word differently, by --replicates: the note of the too_deep keys, the keys of `times` in the document
_TOO_DEEP = ('keys with a pooled coverage above %d were not tested', 'keys whose used replicates sum to a coverage above %d were not tested')
_TIMES = (('select_ms', 'fisher_ms'), ('count_ms', 'write_ms'))


def _engine_for(o: Dict[str, object], rep: int, engine):
    """-> (the engine: the one given, if it was made for these options, else one of the command's own on GPU 0; whether it is the command's own)."""
    made_for = (o['cov'], 1.0 if o['all'] else o['fdr']) + (tuple(o['minReps']) if rep else ())
    if engine is not None:
        has = (engine.cov, engine.alpha) + ((engine.min_a, engine.min_b) if rep else ())
        if has != made_for:
            raise DiffmodError(('diffmod: the engine was made for cov %d alpha %g' + (' minReps %d,%d' if rep else '')) % has)
        return engine, False
    if _lib.load().dm_device_count() < 1:
        raise DiffmodError('no gfx950 GPU visible (this build has no CPU path)')
    if not rep:
        return DeviceEngine(*made_for), True
    try:
        return RepDeviceEngine(*made_for), True
    except _lib.DeepModHipError as exc:
        raise DiffmodError('diffmod: %s' % exc)


def _run_contig(engine, rep: int, ck: str, length: Optional[int], groups: Dict[str, list], pool, notes: List[str]):
    """One contig: the files of every table set into tables of the engine (tables.fill), then its run.  groups: {'sample': [the files of one table
    set, ..], 'control': [..]}, one set per replicate; the pooled test has one set per role, and its entry holds numbers where the replicate test's
    holds a list per replicate.  -> (the contig's entry of the document, the records)"""
    tabs, lines = {}, {}
    for role in ('sample', 'control'):
        tabs[role], lines[role] = [], []
        for j, paths in enumerate(groups[role]):
            t = engine.new_tables('%s%d' % (role, j) if rep else role, ck, length)
            try:
                lines[role].append(tables.fill(t, paths, pool, ck, MAX_LENGTH if length is None else length, notes))
            except (merge.MergeError, tables.TableError) as exc:          # `file:line: reason`; the host tables' refusals
                raise DiffmodError('diffmod: %s' % exc)
            except (ValueError, RuntimeError) as exc:                     # the device tables' own (a coverage sum past int32)
                raise DiffmodError('diffmod: %s: %s' % (exc.path, exc))
            tabs[role].append((t.plus, t.minus))
    counters, rec = engine.run(tabs['sample'], tabs['control']) if rep else engine.run(*tabs['sample'][0], *tabs['control'][0])
    entry = {'length': length, 'files': [len(p) for p in groups['sample']], 'control_files': [len(p) for p in groups['control']],
             'lines_read': lines['sample'], 'control_lines_read': lines['control']}
    if not rep:
        entry = {k: v[0] if isinstance(v, list) else v for k, v in entry.items()}
    for s, strand in enumerate('+-'):
        entry[strand] = dict(zip(COUNT_KEYS, (int(v) for v in counters[s])))
        if counters[s][3]:
            notes.append('%s %s: %d %s' % (ck, strand, int(counters[s][3]), _TOO_DEEP[rep] % MAX_TOTAL))
    return entry, rec


def _list_records(o: Dict[str, object], doc: Dict[str, object], per_contig, fields) -> list:
    """BH over the tested keys of all contigs, then the keep rule: doc gets m, listed (per strand of every contig, and in all), hyper and hypo
    -> the rows of the report, (chr, the record's fields, q)."""
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
            rows.append((ck,) + tuple(rec[k][i].item() for k, _ in fields) + (float(q[i]),))
    doc['m'] = m
    doc['listed'], doc['hyper'], doc['hypo'] = len(rows), hyper, hypo
    return rows


def _write(mo: Dict[str, object], doc: Dict[str, object], text: str) -> None:
    import json
    out_folder = str(mo['outFolder'])
    os.makedirs(out_folder, exist_ok=True)
    prefix = os.path.join(out_folder, doc['inputs']['FileID'])
    with open(prefix + '_diffmod.txt', 'w') as fh:
        fh.write(text)
    with open(prefix + '_diffmod.json', 'w') as fh:
        json.dump(doc, fh, indent=1)
    for ln in doc['notes']:
        print(ln, flush=True)
    print('diffmod: %d keys tested, %d listed (%d above the controls, %d below) -> %s_diffmod.txt' % (doc['m'], doc['listed'], doc['hyper'], doc['hypo'], prefix), flush=True)


def diffmod(mo: Dict[str, object], engine=None) -> Dict[str, object]:
    """The command.  mo: predFolder, control (list of folders), Base, outFolder, FileID, chr (list; None: the contigs of --Ref, or without it those
    the sample's file names hold), Ref (None: the tables grow with the files), cov, fdr, minDelta, all, threads.  replicates 1: the replicate-aware
    test, with predFolder the sample replicates' folders (a list, or one string with commas), control the control replicates' folders and minReps (a,b;
    None: every replicate); on the device it reads 16 bytes per position and replicate of the open contig (its tables hold 24).  engine: an object
    with HostEngine's interface, or RepHostEngine's under replicates 1 (default: DeviceEngine / RepDeviceEngine on GPU 0), made with cov, alpha = fdr
    (1 under all) and minReps.  Writes <outFolder>/<FileID>_diffmod.txt / _diffmod.json -> the JSON document."""
    from concurrent.futures import ThreadPoolExecutor
    rep = replicates_option(mo)
    o, chrkeys, lengths, files, ctrl_files = (check_rep_options if rep else check_options)(mo)
    engine, own = _engine_for(o, rep, engine)
    groups = {ck: {'sample': files[ck], 'control': ctrl_files[ck]} if rep else {'sample': [files[ck]], 'control': [ctrl_files[ck]]} for ck in chrkeys}
    folders = o['replicates'] if rep else {'sample': mo['predFolder'], 'control': [c for c in (mo.get('control') or []) if c]}
    notes: List[str] = []
    doc = {'test': 'quasibinomial-F'} if rep else {}
    doc['inputs'] = dict(o, predFolder=folders['sample'], control=folders['control'], Ref=mo.get('Ref'), chr=chrkeys, FileID=str(mo.get('FileID') or 'mod'),
                         files=[p for ck in chrkeys for g in groups[ck]['sample'] for p in g], control_files=[p for ck in chrkeys for g in groups[ck]['control'] for p in g])
    if rep:
        doc.update(replicates=o['replicates'], minReps=o['minReps'])
    doc['contigs'] = {}
    per_contig = []
    try:
        engine.reset()
        with ThreadPoolExecutor(max(int(mo.get('threads') or 1), 1)) as pool:
            for ck in chrkeys:
                if not any(groups[ck]['sample']) and not any(groups[ck]['control']):
                    continue
                try:
                    doc['contigs'][ck], rec = _run_contig(engine, rep, ck, lengths[ck], groups[ck], pool, notes)
                except _lib.DeepModHipError as exc:                   # device memory that ran out, for one: a line, not a trace
                    if not rep:
                        raise
                    raise DiffmodError('diffmod: %s: %s' % (ck, exc))
                per_contig.append((ck, rec))
        hist = engine.fetch_hist()
        times = engine.times()
    finally:
        if own:
            engine.close()
    rows = _list_records(o, doc, per_contig, REP_RECORD_FIELDS if rep else RECORD_FIELDS)
    if doc['m'] == 0:
        notes.append('no key had --cov %d reads in %s' % (o['cov'], '%d sample and %d control replicates' % tuple(o['minReps']) if rep else 'both the sample and the controls'))
    doc['p_histogram'] = [int(v) for v in hist]
    doc['notes'] = notes
    doc['times'] = dict(zip(_TIMES[rep], (round(t, 4) for t in times)))
    _write(mo, doc, rep_report_text(rows) if rep else report_text(rows))
    return doc
