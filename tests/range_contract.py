"""The input side of the split-f16 range contract (include/deepmod_hip.h, DM_PREC_F16X3 / DM_PREC_F16I8) as a predicate, and the case generators the CPU
self-check (tests/test_range_contract.py) and the GPU tests (tests/test_gpu_range_contract.py) share.

`in_contract` is the header's sentence, written from the header and not from the kernel: no NaN, features 0..5 |x| <= 65504, feature 6 (the event length)
|x| <= 65504 * 2^k with k = DM_INFO_F16_LENGTH_SHIFT.  The kernels test rint(length * 2^-k) <= 65504 and therefore also take lengths up to 65504.5 * 2^k (still
fed exactly): no case here puts a length into the open interval (65504 * 2^k, 65505 * 2^k), so the tests pin neither side of that gap.

A sweep case is (window, row, feature, value): ONE poisoned cell of an otherwise in-contract batch.  The classifier reads a window twice: the forward work item
rows 0..10, the backward work item rows 20..10 - one row per step, prefetched a step ahead, step 0 on a path of its own; a lane holds feature g and feature 4 + g,
the length is cut over lane groups 2 and 3; a wave holds 32 windows as two halves of 16 (the MFMA rows); a tile is 128 windows and the dead lanes of a ragged tile
re-read its last window.  Every one of these is a place where a rewrite can lose the check without changing an output bit, so the sweeps visit all of them."""
import os
import re

import numpy as np

F16_MAX = 65504.0
WIN, NFEAT = 21, 7
LENGTH = 6                      # the feature with the rescaled bound
N_BASE = 129                    # one full tile of 128 windows and a ragged tile of one
S1_WINDOW = 77                  # S1: every cell of this window
S2_CELLS = ((0, 0),             # S2: every window at these cells - forward step 0
            (20, 6),            # backward step 0, on the length
            (10, 5),            # the last step of both directions
            (3, 4), (17, 2))
S2_THIN = (0, 15, 16, 31, 32, 63, 64, 96, 127, 128)

ROWS_FIRST, ROWS_COUNT = 26, 129
ROWS_M = ROWS_FIRST + ROWS_COUNT + 10 + 16          # 16 rows nobody reads on either side of the rows the windows cover
AT_GAP = 32                                         # dm_predict_read_at: the centres jump by this much after the first 64


def in_contract(x, k):
    x = np.asarray(x)
    if np.isnan(x).any():
        return False
    a = np.abs(x.astype(np.float64))
    return bool((a[..., 0:LENGTH] <= F16_MAX).all() and (a[..., LENGTH] <= F16_MAX * 2.0 ** k).all())


def length_limit(k):
    return np.float32(F16_MAX * 2.0 ** k)


def length_beyond(k):
    """The first length the tests require to be refused: 65505 * 2^k (the header refuses from 65504 * 2^k on, the kernels from 65504.5 * 2^k on)."""
    return np.float32(65505.0 * 2.0 ** k)


def poison_kinds(feature, k):
    if feature == LENGTH:
        b = length_beyond(k)
        return (b, -b, np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan))
    return (np.float32(1.0e5), np.float32(-1.0e5), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan))


def s1_cases(k):
    """Every (row, feature) of window S1_WINDOW; the kind of poison rotates so that every feature and every row meets all five."""
    return [(S1_WINDOW, r, f, poison_kinds(f, k)[(r + f) % 5]) for r in range(WIN) for f in range(NFEAT)]


def s2_cases(k, windows=None):
    windows = range(N_BASE) if windows is None else windows
    return [(wi, r, f, poison_kinds(f, k)[(wi + ci) % 5]) for wi in windows for ci, (r, f) in enumerate(S2_CELLS)]


def reader(row):
    """Which work item of a window reads this row."""
    return "forward" if row < WIN // 2 else ("backward" if row > WIN // 2 else "forward+backward")


def describe(case):
    wi, r, f, v = case
    return "window %d (mod 32 = %d: position in the wave, mod 16 = %d: MFMA row) row %d feature %d value %r, read by the %s work item" % (
        wi, wi % 32, wi % 16, r, f, float(v), reader(r))


def poisoned(base, case):
    wi, r, f, v = case
    x = base.copy()
    x[wi, r, f] = v
    return x


def cells_changed(a, b):
    """Number of cells in which two arrays differ, NaN counted as a value."""
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


# ---- boundaries --------------------------------------------------------------------------------------------------------------------------------------

def pass_cases(base, k):
    """name -> batch exactly ON the bounds: each is one call that must succeed (and agree with the oracle)."""
    n = len(base)
    sign = np.where((np.arange(n)[:, None, None] + np.arange(WIN)[None, :, None] + np.arange(NFEAT)[None, None, :]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    out = {}
    x = base.copy()
    x[:, :, 0:LENGTH] = np.float32(F16_MAX) * sign[:, :, 0:LENGTH]
    out["features_pm_65504"] = x
    x = base.copy()
    x[:, :, LENGTH] = length_limit(k) * sign[:, :, LENGTH]
    out["lengths_pm_limit"] = x
    out["negative_zero"] = np.full_like(base, -0.0)
    out["just_inside"] = np.full_like(base, np.nextafter(np.float32(F16_MAX), np.float32(0.0)))
    return out


def raise_boundary_cases(k):
    """One cell each, the first value beyond the bound: the fp32 successor of 65504 on features 0..5 (and its negative), +-65505 * 2^k on the length.  The cells
    are spread over forward-only, backward-only and shared rows, both window halves and the ragged tile."""
    up = np.nextafter(np.float32(F16_MAX), np.float32(np.inf))
    where = ((5, 0), (128, 20), (40, 10), (77, 13), (16, 7), (111, 19))
    cases = []
    for f in range(LENGTH):
        wi, r = where[f]
        cases.append((wi, r, f, up))
        cases.append((wi, WIN - 1 - r, f, -up))
    cases.append((93, 2, LENGTH, length_beyond(k)))
    cases.append((128, 15, LENGTH, -length_beyond(k)))
    return cases


# ---- rows forms --------------------------------------------------------------------------------------------------------------------------------------

def rows_edge_cases(k, at):
    """(row, feature, value, must_raise) for dm_predict_read (at = False: windows centred on ROWS_FIRST .. ROWS_FIRST + ROWS_COUNT - 1) and dm_predict_read_at
    (at = True: the centres of at_centres()).  The first context row is read by the first window's forward step 0 alone, the last one by the last window's
    backward step 0 alone; the rows next to them are read by nobody and may hold anything - NaN included."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    lo = ROWS_FIRST - 10
    hi = (int(at_centres()[-1]) if at else ROWS_FIRST + ROWS_COUNT - 1) + 10
    big = length_beyond(k)
    cases = [(lo, 1, np.float32(-1.0e5), True), (lo, LENGTH, big, True), (hi, 4, nan, True), (hi, LENGTH, -big, True),
             (ROWS_FIRST + 50, 5, inf, True), (ROWS_FIRST + 50, LENGTH, nan, True),
             (lo - 1, 0, nan, False), (lo - 1, LENGTH, big, False), (hi + 1, 3, nan, False), (hi + 1, LENGTH, -inf, False), (0, 2, np.float32(1.0e5), False)]
    if at:
        last_a, first_b = ROWS_FIRST + 63, ROWS_FIRST + 64 + AT_GAP
        cases += [(last_a + 10, 2, np.float32(1.0e5), True), (first_b - 10, LENGTH, big, True),
                  (last_a + 11, 4, nan, False), (first_b - 11, LENGTH, big, False), (last_a + 16, 5, -inf, False)]
    return cases


def rows_m(at):
    return ROWS_M + (AT_GAP if at else 0)


def at_centres():
    """ROWS_COUNT centres: 64 consecutive rows, a jump of AT_GAP (the windows on either side of it leave AT_GAP - 20 rows unread), 65 more."""
    i = np.arange(ROWS_COUNT)
    return (ROWS_FIRST + i + np.where(i >= 64, AT_GAP, 0)).astype(np.int32)


def rows_read(at):
    """Set of the row indices some window of the call reads."""
    centres = at_centres() if at else ROWS_FIRST + np.arange(ROWS_COUNT)
    return set(int(c) + d for c in centres for d in range(-10, 11))


# ---- a model with a small length shift ---------------------------------------------------------------------------------------------------------------

def length_row_scaled(weights, factor):
    """A copy of the weights with the layer-0 kernel row of the event length (both directions) multiplied by `factor` (a power of two: every weight stays
    what it was in f16 terms).  The library stores that row a second time x 2^k with the largest k <= 10 that keeps it an f16, so a large row means a small k."""
    from deepmod_amd import synth
    w = dict(weights)
    for d in ("fw", "bw"):
        name = synth.cell_name(d, 0, "kernel")
        w[name] = w[name].copy()
        w[name][LENGTH] *= np.float32(factor)
    return w


def length_row_factor(weights, k_target):
    """The power of two that length_row_scaled needs for DM_INFO_F16_LENGTH_SHIFT == k_target: the library folds log2(e) (2 log2(e) for the j gate, columns
    100..199) into the row and takes the largest k with max|row| * 2^k <= 32768.  The GPU test asserts the k the model reports, so a change of that rule
    fails loudly there instead of testing another k than it says."""
    from deepmod_amd import synth
    fold = np.where((np.arange(400) >= 100) & (np.arange(400) < 200), 2.8853900817779268, 1.4426950408889634)
    m = max(float(np.abs(weights[synth.cell_name(d, 0, "kernel")][LENGTH].astype(np.float64) * fold).max()) for d in ("fw", "bw"))
    return 2.0 ** (int(np.floor(np.log2(32768.0 / m))) - k_target)


def dm_marks():
    """DM_MARKS of include/deepmod_hip.h (deepmod_amd/_lib.py does not repeat it)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "deepmod_hip.h")) as fh:
        return int(re.search(r"^#define DM_MARKS (\d+)", fh.read(), re.M).group(1))
