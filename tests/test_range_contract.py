"""CPU self-check of tests/range_contract.py: the predicate says what include/deepmod_hip.h says, every "must raise" case of the GPU tests
(tests/test_gpu_range_contract.py) is its in-contract base with exactly ONE cell outside the contract, every "must pass" case is inside it, and no case sits in
the gap between the header's bound on the length (65504 * 2^k) and the first length the kernels refuse (65504.5 * 2^k)."""
import numpy as np
import pytest

import range_contract as rc
from deepmod_amd import synth

KS = (0, 5, 10)


@pytest.fixture(scope="module")
def base():
    x = synth.synthetic_windows(rc.N_BASE, seed=41)
    x.setflags(write=False)
    return x


def test_predicate_is_the_headers_sentence():
    """Literal examples: features 0..5 |x| <= 65504; feature 6 |x| <= 65504 * 2^k (k = 10 for ordinary weights: 67,076,096); no NaN."""
    x = np.zeros((2, 21, 7), np.float32)
    assert rc.in_contract(x, 10) and rc.in_contract(-x, 0)
    for f in range(6):
        for v, ok in ((65504.0, True), (-65504.0, True), (65505.0, False), (-65536.0, False), (1.0e5, False), (np.inf, False), (-np.inf, False), (np.nan, False)):
            y = x.copy()
            y[1, 20, f] = v
            assert rc.in_contract(y, 10) is ok, (f, v)
    for k, limit in ((10, 67076096.0), (5, 2096128.0), (0, 65504.0)):
        assert float(rc.length_limit(k)) == limit
        for v, ok in ((limit, True), (-limit, True), (np.nextafter(np.float32(limit), np.float32(np.inf)), False), (limit * 1.01, False), (-limit * 2.0, False),
                      (np.inf, False), (np.nan, False)):
            y = x.copy()
            y[0, 0, 6] = v
            assert rc.in_contract(y, k) is ok, (k, v)
    y = x.copy()
    y[0, 3, 6] = 70000.0                               # beyond the largest f16, inside the rescaled bound - unless k = 0
    assert rc.in_contract(y, 10) and rc.in_contract(y, 1) and not rc.in_contract(y, 0)
    assert rc.in_contract(np.zeros((0, 21, 7), np.float32), 10)
    assert rc.in_contract(np.full((5, 7), 65504.0, np.float32), 0)          # feature rows [m][7] as well as windows


def _not_in_gap(values, k):
    a = np.abs(np.asarray(values, np.float64))
    a = a[np.isfinite(a)]
    return not ((a > 65504.0 * 2.0 ** k) & (a < 65505.0 * 2.0 ** k)).any()


@pytest.mark.parametrize("k", KS)
def test_must_raise_cases_leave_the_contract_in_exactly_one_cell(base, k):
    assert rc.in_contract(base, k)
    s1, s2, edge = rc.s1_cases(k), rc.s2_cases(k), rc.raise_boundary_cases(k)
    assert len(s1) == 21 * 7 and len(set(c[:3] for c in s1)) == len(s1) and all(c[0] == rc.S1_WINDOW for c in s1)
    assert len(s2) == rc.N_BASE * len(rc.S2_CELLS) and set(c[0] for c in s2) == set(range(rc.N_BASE))
    assert set(rc.S2_THIN) <= set(range(rc.N_BASE)) and repr(rc.s2_cases(k, rc.S2_THIN)) == repr([c for c in s2 if c[0] in rc.S2_THIN])
    for case in s1 + s2 + edge:
        x = rc.poisoned(base, case)
        assert rc.cells_changed(x, base) == 1, rc.describe(case)
        assert not rc.in_contract(x, k), rc.describe(case)
        if case[2] == rc.LENGTH:
            assert _not_in_gap([case[3]], k), rc.describe(case)
    # S1: every feature meets every kind of poison, and so does every row
    for f in range(7):
        got = set(repr(float(c[3])) for c in s1 if c[2] == f)
        assert got == set(repr(float(v)) for v in rc.poison_kinds(f, k)), f
    for r in range(21):
        kinds = set((i for c in s1 if c[1] == r for i, v in enumerate(rc.poison_kinds(c[2], k)) if repr(float(v)) == repr(float(c[3]))))
        assert kinds == set(range(5)), r
    # the boundary list: the fp32 neighbour of 65504 on each of features 0..5, 65505 * 2^k and its negative on the length
    up = np.nextafter(np.float32(65504.0), np.float32(np.inf))
    assert sorted((c[2], float(c[3])) for c in edge) == sorted([(f, s * float(up)) for f in range(6) for s in (1.0, -1.0)] +
                                                                [(6, 65505.0 * 2.0 ** k), (6, -65505.0 * 2.0 ** k)])
    assert {rc.reader(c[1]) for c in edge} == {"forward", "backward", "forward+backward"}


@pytest.mark.parametrize("k", KS)
def test_must_pass_cases_are_inside_the_contract(base, k):
    cases = rc.pass_cases(base, k)
    assert set(cases) == {"features_pm_65504", "lengths_pm_limit", "negative_zero", "just_inside"}
    for name, x in cases.items():
        assert x.shape == base.shape and x.dtype == np.float32 and rc.in_contract(x, k), name
        assert _not_in_gap(x[..., 6], k), name
    x = cases["features_pm_65504"]
    assert (np.abs(x[..., 0:6]) == 65504.0).all() and (x[..., 0:6] > 0).any() and (x[..., 0:6] < 0).any() and np.array_equal(x[..., 6], base[..., 6])
    x = cases["lengths_pm_limit"]
    assert (np.abs(x[..., 6]) == 65504.0 * 2.0 ** k).all() and (x[..., 6] > 0).any() and (x[..., 6] < 0).any() and np.array_equal(x[..., 0:6], base[..., 0:6])
    assert np.signbit(cases["negative_zero"]).all() and not cases["negative_zero"].any()
    assert (cases["just_inside"] < 65504.0).all() and (cases["just_inside"] > 65503.99).all()


@pytest.mark.parametrize("at", [False, True], ids=["predict_read", "predict_read_at"])
@pytest.mark.parametrize("k", KS)
def test_rows_form_cases_raise_exactly_where_a_window_reads(k, at):
    m = rc.rows_m(at)
    rows = synth.synthetic_windows(m, seed=43)[:, 10, :].copy()
    assert rc.in_contract(rows, k)
    read = rc.rows_read(at)
    centres = rc.at_centres() if at else rc.ROWS_FIRST + np.arange(rc.ROWS_COUNT)
    assert len(centres) == rc.ROWS_COUNT == 129 and rc.ROWS_FIRST >= 26 and (np.diff(centres) > 0).all()
    assert min(read) == rc.ROWS_FIRST - 10 >= 16 and max(read) == m - 1 - 16          # unread rows on both sides
    if at:
        assert np.diff(centres).max() == rc.AT_GAP + 1 > 21
    cases = rc.rows_edge_cases(k, at)
    for row, f, v, must_raise in cases:
        assert 0 <= row < m and must_raise is (row in read), (row, f, v)
        y = rows.copy()
        y[row, f] = v
        assert rc.cells_changed(y, rows) == 1 and not rc.in_contract(y, k)
        if f == rc.LENGTH:
            assert _not_in_gap([v], k)
    raising = [c[0] for c in cases if c[3]]
    quiet = [c[0] for c in cases if not c[3]]
    # the first and the last context row, their unread neighbours (one of them holding a NaN), a mid row
    assert min(read) in raising and max(read) in raising and min(read) - 1 in quiet and max(read) + 1 in quiet
    assert any(np.isnan(c[2]) for c in cases if not c[3]) and any(min(read) + 20 < r < max(read) - 20 for r in raising)
    if at:
        gap = [r for r in range(min(read), max(read)) if r not in read]
        assert len(gap) == rc.AT_GAP - 20 and set(gap) & set(quiet) and gap[0] - 1 in raising and gap[-1] + 1 in raising


def test_length_row_scale_is_a_power_of_two():
    w = synth.synthetic_weights(22, 4.0)
    for k in KS:
        f = rc.length_row_factor(w, k)
        assert f >= 1.0 and np.log2(f) == int(np.log2(f))
        w2 = rc.length_row_scaled(w, f)
        for d in ("fw", "bw"):
            name = synth.cell_name(d, 0, "kernel")
            assert np.array_equal(w2[name][6], w[name][6] * np.float32(f)) and np.array_equal(np.delete(w2[name], 6, 0), np.delete(w[name], 6, 0))
            # the row times the gate fold (<= 2.886) times 2^k is what the library stores: at most 32768, so an f16, and more than half of that
            top = float(np.abs(w2[name][6]).max()) * 2.0 ** k
            assert top * 2.8853900817779268 <= 65504.0
    assert rc.dm_marks() >= 2
