"""GPU (-m gpu): the classifier kernels held to the oracle in HIDDEN-STATE space, through probe heads (tests/hidden_probe.py).

Every other parity test compares probabilities after the two-logit softmax, under heads that saturate it on most windows (p1 (1 - p1) < 1e-3 on
half of the 10^6-window fixture's windows and on two thirds of the trained-like ones): a kernel that dropped the low f16 half of a whole layer's
weights stays below 3e-5 there (tests/test_hidden_probe.py shows both numbers side by side).  The head is an input of the ABI, so with a gain-1
dense head, or a one-hot head on one unit, the probabilities are an invertible read-out of the last layer's centre-step output at EVERY window:

    err = max |recover_z(prob_kernel) - z_64|  <=  R[precision] * yard + 2 * floor

over all windows, none exempted.  yard is the fp32 C oracle's own distance from the float64 value of the graph, floor what the fp32 head and the
read-out cost the reference itself; R is measured (hidden_probe.R).  The float64 and C references are computed once per (weights, inputs) pair
and shared by every head and every precision."""
import os

import numpy as np
import pytest

import hidden_probe as hp
from conftest import GOLDEN, trained_like_weights
from deepmod_amd import model, synth

pytestmark = pytest.mark.gpu

HEAD_SEEDS = (1, 2, 3, 4)
# tile edges of the 16-unit MFMA tiles and the four units of the mixed k-step (96..99), in both directions
EDGE_UNITS = (0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 97, 98, 99)
# A probe is a model of its own: 11 ms to create, ~30 ms per unit and precision with the call and the read-out.  All 200 units x 2 weight sets x 3
# precisions were run once to measure hidden_probe.R["unit"] (38 s, a sixth of the GPU suite); the suite keeps the 34 edge units (6 s).
UNITS = EDGE_UNITS


def _weights(name):
    return trained_like_weights() if name == "trained" else synth.synthetic_weights(*name)


def _inputs(name):
    if name == "windows20000":
        return synth.synthetic_windows(20000, seed=131)
    if name == "ragged129":
        return synth.synthetic_windows(129, seed=132)
    if name == "windows2048":
        return synth.synthetic_windows(2048, seed=133)
    if name == "windows1024":
        return synth.synthetic_windows(1024, seed=134)
    if name == "read_shaped_tail":        # make_golden_tail.py: means on the +-5 clip, lengths up to 27,000 samples
        return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "trained_like_tail_case.npz"))["X"], np.float32)
    raise KeyError(name)


_WEIGHTS, _REFS = {}, {}


def weights(wname):
    if wname not in _WEIGHTS:
        _WEIGHTS[wname] = _weights(wname)
    return _WEIGHTS[wname]


def reference(wname, xname, x=None):
    """One Reference per (weights, inputs): hcat does not depend on the head, nor on the precision under test."""
    key = (wname, xname)
    if key not in _REFS:
        _REFS[key] = hp.Reference(weights(wname), _inputs(xname) if x is None else x)
    return _REFS[key]


@pytest.fixture(scope="module", params=["f32", "f16x3", "f16i8"])
def kernel(gpu_device, hip_lib, request):
    """Every test runs for every precision mode of the library (as test_gpu_parity.py::models): exact-fp32 MFMA, the split-f16 default and the
    opt-in int8-cross-term variant, which has its own allowance (under DEEPMOD_PRECISION=auto it runs only where the calibration gate lets it in).
    The head is part of the weights a model is created from, so a probe is a model of its own."""
    def run(w, head, x):
        m = model.BiLSTMModel(hp.probe_weights(w, head), device=gpu_device, precision=request.param)
        try:
            return m.predict_windows(x)[0]
        finally:
            m.close()
    run.precision = request.param
    return run


def _held(kernel, ref, w, head, what):
    r = hp.report(ref, kernel(w, head, ref.x), head)
    bound = hp.allowance(kernel.precision, r["yard"], r["floor"])
    print("[hidden] %-5s %s: yard %.3g floor %.3g err %.3g ratio %.2f (bound %.3g)" % (kernel.precision, what, r["yard"], r["floor"], r["err"], r["ratio"], bound))
    r["bound"] = bound
    return r


@pytest.mark.parametrize("head_seed", HEAD_SEEDS)
@pytest.mark.parametrize("wname", ["trained", (17, 4.0), (21, 1.0)], ids=str)
def test_dense_probe_against_the_float64_oracle(wname, head_seed, kernel):
    """Gain-1 dense heads (every unit of both directions weighs in): 20,000 synthetic windows, the read-shaped tail inputs and a ragged call."""
    w, head = weights(wname), hp.dense_head(head_seed)
    failed = []
    for xname in ("windows20000", "read_shaped_tail", "ragged129"):
        r = _held(kernel, reference(wname, xname), w, head, "%s dense head %d %s" % (wname, head_seed, xname))
        if not r["err"] <= r["bound"]:
            failed.append((xname, r))
    assert not failed, failed


@pytest.mark.parametrize("direction", ["fw", "bw"])
@pytest.mark.parametrize("wname", ["trained", (17, 4.0)], ids=str)
def test_one_hot_probe_per_unit(wname, direction, kernel):
    """p1 = sigmoid(2 h_u): one unit of one direction alone, 2,048 windows per unit, the same assertion per unit with the allowance measured per
    unit (hidden_probe.R["unit"]).  A failure names the direction, the unit and where in the tile the worst window sits (window index mod 128: the
    work item; mod 16: the MFMA row)."""
    w, ref = weights(wname), reference(wname, "windows2048")
    failed, worst = [], None
    for u in UNITS:
        head = hp.one_hot_head(u + (hp.HID if direction == "bw" else 0))
        r = hp.report(ref, kernel(w, head, ref.x), head)
        bound = hp.allowance(kernel.precision, r["yard"], r["floor"], "unit")
        if worst is None or r["ratio"] > worst[1]["ratio"]:
            worst = (u, r)
        if not r["err"] <= bound:
            failed.append("%s unit %d: err %.3g > %.3g (yard %.3g, floor %.3g) at window %d (mod 128: %d, mod 16: %d)" %
                          (direction, u, r["err"], bound, r["yard"], r["floor"], r["worst"], r["worst"] % 128, r["worst"] % 16))
    print("[hidden] %-5s %s one-hot %s: worst unit %d ratio %.2f (yard %.3g floor %.3g err %.3g), %d units" %
          (kernel.precision, wname, direction, worst[0], worst[1]["ratio"], worst[1]["yard"], worst[1]["floor"], worst[1]["err"], len(UNITS)))
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("wname", ["trained", (17, 4.0)], ids=str)
def test_rows_a_direction_never_reads_do_not_move_a_bit(wname, kernel):
    """LIVE = 11: the forward direction reads rows 0..10 of a window, the backward one rows 20..10 (oracle_np.predict_windows_np's row indexing).
    Under a head that is zero on the other direction's units, replacing the rows this direction never reads by other finite in-range rows leaves
    the output bit-identical."""
    w = weights(wname)
    x = synth.synthetic_windows(1000, seed=135)
    other = np.roll(x, 1, axis=0)
    for side, dead in (("fw", slice(11, 21)), ("bw", slice(0, 10))):
        head = (hp.fw_only if side == "fw" else hp.bw_only)(hp.dense_head(2))
        x2 = x.copy()
        x2[:, dead, :] = other[:, dead, :]
        assert not np.array_equal(x2, x)
        a, b = kernel(w, head, x), kernel(w, head, x2)
        diff = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))
        assert diff.size == 0, "%s-only head: %d windows moved by rows the direction never reads, first at %d" % (side, diff.size, diff[0])


@pytest.mark.parametrize("side,rows", [("fw", (0, 1, 9, 10)), ("bw", (20, 19, 11, 10))])
def test_row_influence_matches_the_float64_oracle(side, rows, kernel):
    """What ONE row contributes: row r replaced by another window's row, the change of z in the kernel against the change in float64, within twice
    the bound of a single evaluation.  Rows 0 (fw) and 20 (bw) enter at step 0 - the kernels' special case without a previous state - and reach the
    output only through ten more steps of three layers; this is where that step is held to the reference on its own.  Not vacuous: on the
    trained-like weights the float64 |dz| of the earliest rows exceeds 100 x the bound on more than a tenth of the windows (asserted below; measured
    with the oracles alone: 0.95 of the windows for the fp32-class allowance, 0.7 for the int8 mode's)."""
    wname = "trained"
    w = weights(wname)
    base = reference(wname, "windows1024")
    head = (hp.fw_only if side == "fw" else hp.bw_only)(hp.dense_head(1))
    z_base = hp.recover_z(kernel(w, head, base.x))
    failed = []
    for r in rows:
        x2 = base.x.copy()
        x2[:, r, :] = np.roll(base.x[:, r, :], 1, axis=0)
        ref2 = reference(wname, "windows1024 row %d" % r, x2)
        yard, floor = max(base.yard(head), ref2.yard(head)), max(base.floor(head), ref2.floor(head))
        bound = 2.0 * hp.allowance(kernel.precision, yard, floor)
        dz64 = ref2.z64(head) - base.z64(head)
        moved = float((np.abs(dz64) > 100.0 * bound).mean())
        dzk = hp.recover_z(kernel(w, head, x2)) - z_base
        err = np.abs(dzk - dz64)
        print("[hidden] %-5s row influence %s row %d: |dz64| > 100 x bound on %.2f of the windows, err %.3g (bound %.3g)" %
              (kernel.precision, side, r, moved, float(err.max()), bound))
        assert moved >= 0.1, (side, r, moved)
        if not err.max() <= bound:
            failed.append((side, r, float(err.max()), bound, int(np.argmax(err))))
    assert not failed, failed


@pytest.mark.parametrize("head_seed", HEAD_SEEDS)
def test_the_yardstick_sees_a_dropped_low_half(head_seed, kernel):
    """The kernel gets the trained-like weights with forward layer 2 rounded to f16 (what a split-f16 kernel that lost the `lo` half of that layer
    computes), the oracle the clean ones: the dense-probe check must FAIL.  On the CPU the defect is ~120 x yard against an allowance below 1,
    and 1.4e-5 in probability space under the weights' own head - inside the 3e-5 the probability tests assert."""
    w = weights("trained")
    head = hp.dense_head(head_seed)
    ref = reference("trained", "windows20000")
    r = hp.report(ref, kernel(hp.round_to_f16(w, "fw", 2), head, ref.x), head)
    bound = hp.allowance(kernel.precision, r["yard"], r["floor"])
    print("[hidden] %-5s dropped low half, head %d: err %.3g = %.0f x yard, bound %.3g" % (kernel.precision, head_seed, r["err"], r["err"] / r["yard"], bound))
    assert r["err"] > bound, (r, bound)
