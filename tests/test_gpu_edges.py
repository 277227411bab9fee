"""GPU (-m gpu): the split-f16 classifier kernels give the bits of the library BEFORE the edge work on the classifier (profiles/edges/README.md):
the MFMA order inside a k32-step changed there (the snake order is the only one), and whatever else is done to launch and super-tile edges may
move time, never a bit.

tests/golden/edges_parent_bits.npz was written by tests/golden/make_golden_edges.py on the parent commit's library: uint32 views of `prob` and
`cls` for the calls of tests/edges_cases.py, for f16x3 and f16i8, on synth.synthetic_weights(26, 4.0) and on the trained-like weights.  Every
comparison here is exact equality; there is no tolerance.

Cases: n = 1, 127, 128, 129, 385 through materialised windows; two calls through dm_predict_read_at (the widx addressing) under
DM_OPT_RESERVED_CUS at its maximum in which workgroups run three items - the premise is asserted from the launch geometry the library reports
(tests/work_items.py), once on an even grid (a workgroup keeps its direction) and once on an odd one (a workgroup alternates, and the two items of
the tile at a round boundary run in different rounds); three consecutive launches of different n on one model; `prob` only and `cls` only; an input
outside the f16 range, which is still refused with DM_ERANGE and leaves the next call's bits alone.

One case of the edge work's plan cannot be set up through the public options: both directions of ONE tile on the SAME workgroup.  Items 2 t and
2 t + 1 land on workgroups (2 t) % g and (2 t + 1) % g, equal only for a grid of g = 1, and DM_OPT_RESERVED_CUS leaves at least half the CUs
(launches of one tile run on two workgroups).  The odd-grid case above is the nearest a call can get."""
import numpy as np
import pytest

import edges_cases as ec
import work_items as wi
from deepmod_amd import _lib, model

pytestmark = pytest.mark.gpu

_MODELS = {}


@pytest.fixture(scope="module")
def parent():
    z = np.load(ec.FIXTURE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module", params=[(w, p) for w in ec.WEIGHTS for p in ec.PRECISIONS], ids=lambda wp: "%s-%s" % wp)
def held(request, gpu_device, hip_lib, parent):
    """One model per (weights, precision) for the whole module, and what the parent's library gave for it."""
    wname, precision = request.param
    if request.param not in _MODELS:
        _MODELS[request.param] = model.BiLSTMModel(ec.weights(wname), device=gpu_device, precision=precision)
    m = _MODELS[request.param]

    def want(case):
        return parent[ec.key(wname, precision, case, "prob")], parent[ec.key(wname, precision, case, "cls")]
    return m, want, "%s %s" % request.param


def teardown_module(module):
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()


def _differs(prob, cls, want_prob, want_cls):
    """Findings of one call against the parent's bits (empty: equal)."""
    out = []
    got = ec.bits(prob)
    if got.shape != want_prob.shape or len(cls) != len(want_cls):
        return ["shapes %s / %s against the parent's %s / %s" % (got.shape, cls.shape, want_prob.shape, want_cls.shape)]
    d = np.flatnonzero((got != want_prob).any(axis=1))
    if d.size:
        i = int(d[0])
        out.append("%d of %d windows differ in prob, first at %d (tile %d, lane %d): %r against the parent's %r" %
                   (d.size, len(got), i, i // ec.TILE, i % ec.TILE, prob[i].tolist(), want_prob[i].view(np.float32).tolist()))
    d = np.flatnonzero(np.asarray(cls) != want_cls)
    if d.size:
        out.append("%d windows differ in cls, first at %d" % (d.size, int(d[0])))
    return out


@pytest.mark.parametrize("n", ec.SIZES)
def test_same_bits_as_the_parent(n, held):
    m, want, what = held
    prob, cls, _ = ec.run(m, "n%d" % n)
    failed = _differs(prob, cls, *want("n%d" % n))
    assert not failed, "%s n = %d: %s" % (what, n, "; ".join(failed))


@pytest.mark.parametrize("case", sorted(ec.ROUNDS3))
def test_same_bits_when_workgroups_run_three_items(case, held):
    """dm_predict_read_at (widx) under the reserved grid: at least three rounds, so that workgroups run a third item; on the odd grid every workgroup
    alternates directions and a tile's two items lie in different rounds at a round boundary."""
    m, want, what = held
    prob, cls, (cap, grid) = ec.run(m, case)
    geo = wi.Geometry(ec.ROUNDS3[case], grid, cap)
    print("[edges] %s %s: %s" % (what, case, geo.describe()))
    if not (geo.rounds >= 3 and geo.items_per_group().max() >= 3 and geo.grid % 2 == (1 if case.endswith("odd") else 0)):
        raise AssertionError("PREMISE BROKEN (no workgroup runs three items, or the grid's parity is not the case's): " + geo.describe())
    if case.endswith("odd"):
        ir = geo.item_round()
        assert (ir[0::2] != ir[1::2]).any(), "PREMISE BROKEN: no tile has its two items in different rounds: " + geo.describe()
    failed = _differs(prob, cls, *want(case))
    assert not failed, "%s %s: %s" % (what, case, "; ".join(failed))


def test_consecutive_launches_of_different_size_on_one_model(held):
    """385, then 129, then 1 window, then 385 again, back to back on one model: nothing a launch leaves behind on the model (partial logits, any
    per-tile state) reaches the next one."""
    m, want, what = held
    failed = []
    for n in (385, 129, 1, 385):
        prob, cls, _ = ec.run(m, "n%d" % n)
        failed += ["n = %d: %s" % (n, f) for f in _differs(prob, cls, *want("n%d" % n))]
    assert not failed, "%s: %s" % (what, "; ".join(failed))


def test_prob_only_and_cls_only(held):
    """A null `cls` or a null `prob` (dm_predict_windows takes either): the one that is asked for holds the parent's bits."""
    m, want, what = held
    want_prob, want_cls = want("n385")
    x = np.ascontiguousarray(ec.windows()[:385], np.float32)
    prob = np.full((385, 2), np.nan, np.float32)
    _lib.check(m._lib.dm_predict_windows(m._h, x.ctypes.data, 385, prob.ctypes.data, None))
    cls = np.full(385, 7, np.uint8)
    _lib.check(m._lib.dm_predict_windows(m._h, x.ctypes.data, 385, None, cls.ctypes.data))
    failed = _differs(prob, cls, want_prob, want_cls)
    assert not failed, "%s: %s" % (what, "; ".join(failed))


def test_an_input_outside_the_f16_range_is_still_refused(held):
    m, want, what = held
    x = np.array(ec.windows()[:129], np.float32)
    x[128, 10, 0] = 1.0e6                      # the lone window of the ragged tile, a row both directions read
    with pytest.raises(_lib.DeepModRangeError):
        m.predict_windows(x)
    prob, cls, _ = ec.run(m, "n129")           # the flag does not stick
    failed = _differs(prob, cls, *want("n129"))
    assert not failed, "%s after the refusal: %s" % (what, "; ".join(failed))
