"""CPU self-check of the hidden-state yardstick (tests/hidden_probe.py) that tests/test_gpu_hidden_parity.py holds the HIP kernels to.  The
stand-in for "kernel" is the fp32 numpy oracle: on clean weights it must sit inside yard + floor, on weights whose low f16 half was dropped
(what a subtly wrong split-f16 kernel computes) it must stand out in hidden space - while the suite's own probability-space check lets the
same defect pass.  That second half is the documented reason the probe module exists."""
import numpy as np
import pytest

import hidden_probe as hp
from conftest import trained_like_weights
from deepmod_amd import synth
from oracle import oracle_np

HEAD_SEEDS = (1, 2, 3, 4)
N_CLEAN, N_DAMAGED = 1024, 2048


def _weights(name):
    if name == "trained":
        return trained_like_weights()
    seed, scale = name
    return synth.synthetic_weights(seed, scale)


def _np32(w, x):
    """(prob under the weights' own head, hcat) of the fp32 numpy oracle."""
    prob, _, hcat = oracle_np.predict_windows_np(w, x, np.float32)
    return prob, hcat


def test_probe_heads_and_readout():
    w = synth.synthetic_weights(21, 1.0)
    head = hp.dense_head(3)
    pw = hp.probe_weights(w, head)
    assert pw is not w and np.array_equal(pw[hp.HEAD_W], head) and not pw[hp.HEAD_B].any() and w[hp.HEAD_B].any()
    assert all(pw[k] is w[k] for k in w if k not in (hp.HEAD_W, hp.HEAD_B))
    assert head.dtype == np.float32 and abs(float((hp.head_vector(head) ** 2).sum()) - 2.0) < 0.5        # gain 1 per logit
    assert np.array_equal(hp.dense_head(3), head) and not np.array_equal(hp.dense_head(4), head)
    for u in (0, 99, 100, 199):
        v = hp.head_vector(hp.one_hot_head(u))
        assert v[u] == 2.0 and np.count_nonzero(v) == 1
    assert not hp.fw_only(head)[100:].any() and np.array_equal(hp.fw_only(head)[:100], head[:100])
    assert not hp.bw_only(head)[:100].any() and np.array_equal(hp.bw_only(head)[100:], head[100:])
    # the read-out inverts the two-logit softmax: float64 probabilities of known z, rounded to fp32
    z = np.linspace(-2.0, 2.0, 4001)
    p1 = 1.0 / (1.0 + np.exp(-z))
    prob = np.stack([1.0 - p1, p1], axis=1).astype(np.float32)
    assert np.abs(hp.recover_z(prob) - z).max() < 4e-7                    # two fp32 roundings of p at |z| <= 2: (1 + e^2) 2^-24 each at most
    # head_prob_np is the oracle's own head + softmax (bit for bit), so a damaged-weight case needs ONE evaluation of the cells for all its heads
    x = synth.synthetic_windows(200, seed=5)
    hcat = _np32(w, x)[1]
    for h in (head, hp.one_hot_head(137)):
        assert np.array_equal(hp.head_prob_np(hcat, h).view(np.uint32), _np32(hp.probe_weights(w, h), x)[0].view(np.uint32))
    # c_head_prob gives the C oracle's probabilities under a probe head from the hcat of ONE C-oracle run: p to one fp32 ulp (2^-24 below 1), so
    # `floor` within 2^-24 / (p1 (1 - p1)) of the one a full run under that head gives
    ref = hp.Reference(w, x)
    for h in (head, hp.dense_head(1), hp.one_hot_head(3), hp.one_hot_head(150)):
        full = oracle_np.predict_windows_c(hp.probe_weights(w, h), x)[0]
        assert np.abs(full - ref.prob_c32(h)).max() <= 2.0 ** -24
        floor_full = float(np.abs(hp.recover_z(full) - ref.z32(h)).max())
        assert abs(ref.floor(h) - floor_full) <= 2.0 ** -24 / 0.1, (ref.floor(h), floor_full)
    # the chunked float64 evaluation is the oracle's own
    assert np.array_equal(hp.hcat64(w, x), oracle_np.predict_windows_np(w, x, np.float64)[2])
    z64, z32 = hp.reference_z(w, x, head)
    assert z64.dtype == np.float64 and z64.shape == (200,) and 0 < np.abs(z64 - z32).max() < 1e-5


@pytest.mark.parametrize("name", ["trained", (17, 4.0), (21, 4.0), (22, 4.0), (26, 4.0), (21, 1.0)], ids=str)
def test_clean_weights_sit_inside_the_yardstick_and_the_softmax_stays_linear(name):
    """On clean weights the fp32 numpy oracle (the C oracle's arithmetic in another summation order) is inside the GPU tests' bound under every
    dense head, and the gain-1 head keeps p1 (1 - p1) >= 0.1 on EVERY window of every weight set the suite uses -
    where the suite's own heads leave it below 1e-3 on half of them."""
    w = _weights(name)
    x = synth.synthetic_windows(N_CLEAN, seed=77)
    ref = hp.Reference(w, x)
    hcat32 = _np32(w, x)[1]
    for hs in HEAD_SEEDS:
        head = hp.dense_head(hs)
        r = hp.report(ref, hp.head_prob_np(hcat32, head), head)
        sens = float(hp.sensitivity(ref.z64(head)).min())
        print("%s head %d: yard %.3g floor %.3g err %.3g  min p1(1-p1) %.3f" % (name, hs, r["yard"], r["floor"], r["err"], sens))
        assert sens >= 0.1, (name, hs, sens)
        assert 0 < r["floor"] < 1.5e-6 and 0 < r["yard"] < 1e-5, r
        # a CORRECT fp32 evaluation in another summation order (a second draw of `yard`) passes the bound the GPU kernels are held to
        assert r["err"] <= hp.allowance("f32", r["yard"], r["floor"]), (name, hs, r)


def test_the_suites_own_heads_saturate_the_softmax():
    """Why probability space is not enough: under the heads the parity tests use, most windows of the 10^6-window fixture's weights (seed 17 x 4)
    and of the trained-like weights have p1 (1 - p1) < 1e-3."""
    x = synth.synthetic_windows(N_CLEAN, seed=77)
    for name in ("trained", (17, 4.0)):
        p1 = oracle_np.predict_windows_c(_weights(name), x)[0][:, 1].astype(np.float64)
        assert (p1 * (1.0 - p1) < 1e-3).mean() > 0.4, name


# (direction, layer, rows, columns) rounded to f16; the err / yard the dense probe must show (measured on 20,000 windows with the oracles alone, before
# any kernel was probed: 121, 6.4, 65 - asserted a little below, on 2,048 windows); whether the defect must stay
# below 3e-5 in probability space under the suite's own head
DAMAGE = [
    ("fw layer 2, whole kernel", ("fw", 2, slice(None), slice(None)), 100.0, True),
    ("bw layer 1, rows 196:200 (units 96..99, the mixed k-step)", ("bw", 1, slice(196, 200), slice(None)), 6.0, True),
    ("fw layer 0, gate-j columns 100:116", ("fw", 0, slice(None), slice(100, 116)), 50.0, False),
]


@pytest.fixture(scope="module")
def trained_ref():
    w = trained_like_weights()
    x = synth.synthetic_windows(N_DAMAGED, seed=77)
    return w, x, hp.Reference(w, x), oracle_np.predict_windows_c(w, x)[0]


@pytest.mark.parametrize("label,where,least,hidden_in_prob", DAMAGE, ids=[d[0].split(",")[0] + d[0].split(",")[1][:8] for d in DAMAGE])
def test_dropped_low_half_passes_probability_space_and_fails_hidden_space(label, where, least, hidden_in_prob, trained_ref):
    """The trained-like weights with part of one kernel rounded to f16, evaluated by the fp32 numpy oracle, against the CLEAN references.
    Probability space (the suite's own head, the C oracle: what test_gpu_parity asserts at 3e-5 on these weights) next to hidden space."""
    w, x, ref, prob_clean = trained_ref
    wd = hp.round_to_f16(w, *where)
    assert not np.array_equal(wd[oracle_np.cell_name(where[0], where[1], "kernel")], w[oracle_np.cell_name(where[0], where[1], "kernel")])
    prob_d, hcat_d = _np32(wd, x)
    dp = float(np.abs(prob_d - prob_clean).max())
    worst_over_yard, exceeded = [], 0
    for hs in HEAD_SEEDS:
        head = hp.dense_head(hs)
        r = hp.report(ref, hp.head_prob_np(hcat_d, head), head)
        bound = max(hp.allowance("f32", r["yard"], r["floor"]), hp.allowance("f16x3", r["yard"], r["floor"]))
        print("%s | head %d: probability space max|dp| %.3g (asserted there: 3e-5) | hidden space err %.3g = %.1f x yard %.3g, bound %.3g" %
              (label, hs, dp, r["err"], r["err"] / r["yard"], r["yard"], bound))
        worst_over_yard.append(r["err"] / r["yard"])
        exceeded += r["err"] > bound
    # the unit the defect moves most, through the one-hot probe of that unit - the per-unit pass of the GPU module
    dh = np.abs(hcat_d.astype(np.float64) - ref.h64).max(axis=0)
    unit = int(np.argmax(dh))
    head = hp.one_hot_head(unit)
    r1 = hp.report(ref, hp.head_prob_np(hcat_d, head), head)
    bound1 = max(hp.allowance("f32", r1["yard"], r1["floor"], "unit"), hp.allowance("f16x3", r1["yard"], r1["floor"], "unit"))
    print("%s | one-hot unit %d: err %.3g = %.1f x yard %.3g, bound %.3g" % (label, unit, r1["err"], r1["err"] / r1["yard"], r1["yard"], bound1))
    if hidden_in_prob:
        assert dp < 3e-5, dp                                   # today's suite lets this defect pass ...
    else:
        assert dp < 1e-4, dp                                   # ... and this one passes the path's tolerance
    assert max(worst_over_yard) >= least, worst_over_yard      # ... hidden space does not
    assert exceeded == len(HEAD_SEEDS) and r1["err"] > bound1, (exceeded, r1, bound1)      # beyond the GPU tests' bound under every head
    assert r1["err"] / r1["yard"] >= least
