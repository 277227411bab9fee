"""GPU: the trainer (csrc/train.hip.inc behind dm_trainer_*) against torch-CPU float64 autograd of the exact architecture (tests/train_oracle.py).

The acceptance rule of the gradients: for each of the 14 tensors T, e(T) = max|g - g64| / max|g64|, and

        e_gpu(T) <= R * e32(T) + 2^-23

where e32 is torch-CPU float32 autograd against the same float64 result (what a correct fp32 implementation with another summation order
loses) and 2^-23 one unit round-off.  The loss is held by the same rule.

R   = 18    measured 2026-10-18 on one MI355X: the worst (e_gpu - 2^-23) / e32 over the cases below (and a second n = 2,049 case) was 11.86
            (trained-like weights, n = 2,049, unbalanced, bw1/kernel: e_gpu 1.81e-6 against e32 1.43e-7; at n = 1, fw1/bias: 10.3), x 1.5 box-to-box
            and compiler margin = 17.8, rounded up.  The loss alone: 1.55.
R_L = 266   measured 2026-10-18: the worst (|loss_gpu - loss64| - 2^-23 loss64) / |loss32 - loss64| over the 40 steps of the learning test was
            176.8 (step 7: 3.1e-6 against 1.7e-8), x 1.5 = 265.2, rounded up.  The absolute figures: the GPU trajectory stays within 5.6e-6 of the
            float64 one, the float32 one within 1.4e-7 - the float32 run lies within the resolution of a float32 loss at most steps, which is what
            makes the ratio large.  The first Adam steps divide by sqrt(v) + eps with v ~ g^2: where |g| is near eps / sqrt(1 - beta2) = 3e-7 the
            update has slope lr (1 - beta1) / eps = 1e4 in g, so an absolute gradient error of 1e-8 moves a weight by 1e-4.

A tensor's maximum is set by its largest rows (the event-length row of a layer-0 kernel carries gradients 30 to 1,000 times those of the other
rows), so the rule above holds a small row group, gate or the partial unit tile 96..99 only to per cent of its own scale.  The block rule holds
each of the 195 blocks B of train_oracle.BLOCKS (row group x gate x unit group) to its own scale:

        e_gpu(B) <= R_B * e32*(B) + 2^-23

where e32*(B) is the largest e32 of the block over three float32 evaluations of the oracle in three summation orders (the batch as given,
reversed, in two halves): one evaluation's error of a 4-element block can be luckily small.  tests/test_train_host.py checks on the CPU that
every case gives every block a float64 gradient and a yardstick above zero, and that the rule rejects what the tensor rule accepts.

R_B = 41    measured 2026-10-19 on one MI355X: the worst (e_gpu(B) - 2^-23) / e32*(B) over all blocks of all cases below was 26.87 (trained-like
            weights, synthetic windows, n = 2,049, unbalanced, bw2/bias[o,u96-99]: e_gpu 5.07e-6 against e32* 1.84e-7; absolute error 4.35e-9 on a
            block maximum of 8.6e-4, in a tensor whose maximum is 0.77), x 1.5 = 40.3, rounded up.  At n = 2,049 the median block ratio is 2.9
            (dw_kernel adds the 2,049 windows on one accumulator chain of 513 MFMAs, torch sums in blocks; at n <= 129 the median is at most 1.2),
            the four terms of this block cancel to a tenth of sum|term| (6 to 12 per unit, from the float64 oracle), and the next blocks are 13.4,
            12.1 (the same gate's units 0..95) and 12.1.  The second (the smaller call on a used handle, n = 1, bw0/kernel[mean,f,u96-99]): 22.57,
            e_gpu 4.91e-7 - four units round-off - against e32* 1.65e-8, a single draw at n = 1 where the three evaluations coincide; that call's
            median block ratio is 0.9.  Over all cases units 96..99 and units 0..95, the four gates and the row groups have the same median e_gpu
            (2.7e-7 and 2.8e-7 for the unit groups): no operand segment, gate or tile edge stands out.  The yardstick is the CPU's: with the
            float32 oracle run on 8 threads in place of 16 the same GPU gradients give 37.3 at n = 2,049 (fw0/bias[i,u96-99]) and 6.3 on
            the n = 1 call, at most 12.4 elsewhere.  Worst per family: synthetic windows
            n <= 129 10.29, n = 2,049 26.87, read-shaped 11.08, saturating weights 4.19, one class 7.44, shrinking batches 22.57, Session 2.96.
prob        max|prob - prob64| <= R max|prob32 - prob64| + 2^-23 with the R above: the worst (max|prob - prob64| - 2^-23) / max|prob32 - prob64|
            measured 2026-10-19 was 1.84 (read-shaped windows, n = 129: 7.7e-7 against 3.5e-7).
"""
import importlib.util
import os

import numpy as np
import pytest

import train_oracle as oracle
from conftest import GOLDEN, ROOT, trained_like_weights
from deepmod_amd import model, synth, train

pytestmark = pytest.mark.gpu

R = 18
R_L = 266
R_B = 41
U = 2.0 ** -23
TOL = 1e-4                 # the project's probability tolerance (tests/test_gpu_parity.py)
MAX_BATCH = 2049

GRAD_NS = (1, 15, 16, 17, 33, 129)      # row-tile edges; 11 n off a multiple of 4; and one n = 2,049 below (one past the nominal batch)
assert GRAD_NS == oracle.GRAD_NS and oracle.BIG_CASE == ("synth", "trained", MAX_BATCH, True)


def _weights(which):
    return model.flatten_weights(synth.synthetic_weights(5, 1.0) if which == "synthetic" else trained_like_weights())


def _batch(n, seed):
    x = synth.synthetic_windows(n, seed=seed)
    lab = np.random.default_rng(seed + 1).integers(0, 2, n)
    return x, np.eye(2, dtype=np.float32)[lab]


@pytest.fixture(scope="module")
def trainers(gpu_device):
    made = {}

    def get(which):
        if which not in made:
            made[which] = train.Trainer(_weights(which), device=gpu_device, max_batch=MAX_BATCH)
        return made[which]
    yield get
    for t in made.values():
        t.close()


def gradient_case(tr, which, n, unbalanced):
    """-> (e_gpu, e32) dicts over the 14 tensors plus 'loss'."""
    ref = oracle.reference(("synth", which, n, unbalanced))
    l64, g64, l32 = ref["l64"], ref["g64"], ref["l32"]
    loss, _, g = tr.grad(ref["x"], ref["y"], unbalanced, want_prob=False)
    e_gpu = oracle.tensor_errors(g.astype(np.float64), g64)
    e_32 = oracle.tensor_errors(ref["g32"].astype(np.float64), g64)
    e_gpu["loss"] = abs(loss - l64) / abs(l64)
    e_32["loss"] = abs(l32 - l64) / abs(l64)
    return e_gpu, e_32


def blocks_and_prob(case, prob, g):
    """The block rule and the prob rule of one call against the case's reference: prints the worst block, then asserts every block and prob."""
    ref = oracle.reference(case)
    e_gpu, e_32 = oracle.block_errors(g, ref["g64"]), ref["e32_blocks"]
    ratio, name = max(((e_gpu[k] - U) / e_32[k], k) for k in e_gpu)
    a = np.abs(ref["g64"])
    idx = next(i for k, _, i in oracle.BLOCKS if k == name)
    print("blocks %s worst %s e_gpu=%.3g e32*=%.3g ratio=%.3g (abs err %.3g, block max|g64| %.3g, tensor max|g64| %.3g)" %
          (oracle.case_id(case), name, e_gpu[name], e_32[name], ratio, e_gpu[name] * a[idx].max(), a[idx].max(),
           max(a[lo:hi].max() for t, lo, hi, _ in oracle.SLICES if t == name.split("[")[0])))
    dp, dp32 = float(np.abs(prob - ref["p64"]).max()), ref["e32_prob"]
    print("prob   %s max|p - p64|=%.3g max|p32 - p64|=%.3g ratio=%.3g" % (oracle.case_id(case), dp, dp32, (dp - U) / max(dp32, 1e-300)))
    assert prob.shape == ref["p64"].shape and prob.dtype == np.float32
    for k in e_gpu:
        assert e_gpu[k] <= R_B * e_32[k] + U, k
    assert dp <= R * dp32 + U


def held_to_the_oracle(case, loss, prob, g):
    """Every rule on one call: loss and the 14 tensors by R, the 195 blocks by R_B, prob by R."""
    ref = oracle.reference(case)
    e_gpu = oracle.tensor_errors(g.astype(np.float64), ref["g64"])
    e_32 = oracle.tensor_errors(ref["g32"].astype(np.float64), ref["g64"])
    e_gpu["loss"] = abs(loss - ref["l64"]) / abs(ref["l64"])
    e_32["loss"] = abs(ref["l32"] - ref["l64"]) / abs(ref["l64"])
    ratio, name = max(((e_gpu[k] - U) / max(e_32[k], 1e-300), k) for k in e_gpu)
    print("grad   %s worst %s e_gpu=%.3g e32=%.3g ratio=%.3g" % (oracle.case_id(case), name, e_gpu[name], e_32[name], ratio))
    for name in e_gpu:
        assert e_gpu[name] <= R * e_32[name] + U, name
    blocks_and_prob(case, prob, g)


@pytest.mark.parametrize("n", (1, 17, 129))
def test_forward_equals_the_fp32_inference_kernel(trainers, gpu_device, n):
    for which in ("synthetic", "trained"):
        flat = _weights(which)
        x, y = _batch(n, 50 + n)
        m = model.BiLSTMModel(train.unflatten_weights(flat), device=gpu_device, precision="f32")
        want, _ = m.predict_windows(x)
        m.close()
        for unbalanced in (False, True):          # the class weights live in the loss only: predictions stay softmax(z)
            _, prob, _ = trainers(which).grad(x, y, unbalanced, want_grad=False)
            err = float(np.abs(prob - want).max())
            print("forward %s n=%d unbalanced=%d max|dp|=%.3g" % (which, n, unbalanced, err))
            assert err <= TOL


@pytest.mark.parametrize("unbalanced", (False, True))
@pytest.mark.parametrize("which", ("synthetic", "trained"))
@pytest.mark.parametrize("n", GRAD_NS)
def test_gradients_and_loss_against_float64_autograd(trainers, which, n, unbalanced):
    e_gpu, e_32 = gradient_case(trainers(which), which, n, unbalanced)
    for name in e_gpu:
        print("grad %s n=%d unbalanced=%d %-10s e_gpu=%.3g e32=%.3g ratio=%.3g" %
              (which, n, unbalanced, name, e_gpu[name], e_32[name], (e_gpu[name] - U) / max(e_32[name], 1e-300)))
    for name in e_gpu:
        assert e_gpu[name] <= R * e_32[name] + U, name


def test_gradients_one_past_the_nominal_batch(trainers):
    e_gpu, e_32 = gradient_case(trainers("trained"), "trained", 2049, True)
    for name in e_gpu:
        print("grad trained n=2049 unbalanced=1 %-10s e_gpu=%.3g e32=%.3g ratio=%.3g" %
              (name, e_gpu[name], e_32[name], (e_gpu[name] - U) / max(e_32[name], 1e-300)))
    for name in e_gpu:
        assert e_gpu[name] <= R * e_32[name] + U, name


@pytest.mark.parametrize("unbalanced", (False, True))
@pytest.mark.parametrize("which", ("synthetic", "trained"))
@pytest.mark.parametrize("n", GRAD_NS)
def test_gradient_blocks_and_prob_against_float64_autograd(trainers, which, n, unbalanced):
    case = ("synth", which, n, unbalanced)
    ref = oracle.reference(case)
    _, prob, g = trainers(which).grad(ref["x"], ref["y"], unbalanced)
    blocks_and_prob(case, prob, g)


def test_gradient_blocks_and_prob_one_past_the_nominal_batch(trainers):
    ref = oracle.reference(oracle.BIG_CASE)
    _, prob, g = trainers("trained").grad(ref["x"], ref["y"], ref["unbalanced"])
    blocks_and_prob(oracle.BIG_CASE, prob, g)


@pytest.mark.parametrize("case", oracle.TAIL_CASES, ids=oracle.case_id)
def test_read_shaped_gradients_against_float64_autograd(gpu_device, case):
    """Windows of tests/golden/trained_like_tail_case.npz (event lengths up to 26,984, means on the +-5 clip) with seeded labels: trained-like
    weights unbalanced at n = 1, 17, 129; saturating weights (scale 4) balanced at n = 33; 16 windows of one class, each class."""
    ref = oracle.reference(case)
    tr = train.Trainer(ref["flat"], device=gpu_device, max_batch=len(ref["x"]))
    try:
        loss, prob, g = tr.grad(ref["x"], ref["y"], ref["unbalanced"])
    finally:
        tr.close()
    held_to_the_oracle(case, loss, prob, g)


def test_smaller_batches_after_a_larger_one_on_one_handle(gpu_device):
    """n = 129, 1, 17, 16, 129 on one Trainer(max_batch=129), each call with other windows, other labels and the other `unbalanced`: what the
    larger call left in the tape, dh and dc is wrong for the smaller one, so a stale entry that is read shows against the float64 oracle."""
    ref0 = oracle.reference(oracle.SHRINK_CASES[0])
    tr = train.Trainer(ref0["flat"], device=gpu_device, max_batch=max(oracle.SHRINK_NS))
    try:
        got = []
        for case in oracle.SHRINK_CASES:
            ref = oracle.reference(case)
            assert len(ref["x"]) == oracle.SHRINK_NS[case[1]] and np.array_equal(ref["flat"], ref0["flat"])
            got.append(tr.grad(ref["x"], ref["y"], ref["unbalanced"]))
    finally:
        tr.close()
    for case, (loss, prob, g) in zip(oracle.SHRINK_CASES, got):
        held_to_the_oracle(case, loss, prob, g)


def test_session_fetch_after_a_larger_one_is_held_to_the_oracle(gpu_device):
    """model.Session with a tape of 16 windows: a 40-window fetch makes the trainer grow, the 9-window fetch after it is held to float64 - loss and
    prob as the session returns them, the gradient from the session's own trainer."""
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        model.mCreateSession(7, 100, 21, {"outputlayer": "", "unbalanced": 0, "seed": oracle.SESSION_SEED, "max_batch": 16})
    sess = model.new_session(gpu_device)
    try:
        sess.run(init)
        for case in oracle.SESSION_CASES:
            ref = oracle.reference(case)
            loss, prob = sess.run([loss_op, sess.graph.prediction], feed_dict={X: ref["x"], Y: ref["y"]})
            tr = sess._train.trainer
            assert tr.max_batch >= max(oracle.SESSION_NS[:case[1] + 1])
            assert np.array_equal(tr.get_state()[0], ref["flat"])
            loss2, prob2, g = tr.grad(ref["x"], ref["y"], False)
            assert np.float32(loss).tobytes() == np.float32(loss2).tobytes() and np.array_equal(prob, prob2)
            held_to_the_oracle(case, float(loss), prob, g)
    finally:
        sess.close()


def test_unbalanced_reaches_the_kernel_through_the_session(gpu_device):
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        model.mCreateSession(7, 100, 21, {"outputlayer": "", "unbalanced": 1, "seed": 2, "max_batch": 16})
    sess = model.new_session(gpu_device)
    weighted, plain = (train.Trainer(train.initial_weights(2), device=gpu_device, max_batch=16) for _ in range(2))
    bits = lambda v: np.float32(v).tobytes()
    try:
        sess.run(init)
        x, y = _batch(16, 410)
        got = sess.run([train_op, loss_op], feed_dict={X: x, Y: y})
        assert bits(got[1]) == bits(weighted.step(x, y, unbalanced=True))
        assert bits(got[1]) != bits(plain.step(x, y, unbalanced=False))
        assert _same_state(sess._train.trainer.get_state(), weighted.get_state())
        assert not np.array_equal(sess._train.trainer.get_state()[0], plain.get_state()[0])
        plain.set_state(*weighted.get_state())
        x, y = _batch(9, 411)
        loss = sess.run(loss_op, feed_dict={X: x, Y: y})              # the loss-only fetch: dm_trainer_grad
        assert bits(loss) == bits(weighted.grad(x, y, True, want_grad=False)[0])
        assert bits(loss) != bits(plain.grad(x, y, False, want_grad=False)[0])
    finally:
        sess.close()
        weighted.close()
        plain.close()


def test_a_loss_that_is_not_finite_is_refused_and_the_state_kept(gpu_device):
    """out/W of +-3e38 on hidden states of order 1: the logits overflow, the loss is NaN or Inf.  step and grad refuse, Adam does not run."""
    from deepmod_amd import _lib
    tr = train.Trainer(_weights("trained"), device=gpu_device, max_batch=32)
    try:
        x, y = _batch(20, 9)
        tr.step(x, y)
        good = tr.get_state()
        bad = good[0].copy()
        a, b = oracle.SLICES[12][1:3]
        bad[a:b] = np.float32(3e38) * np.random.default_rng(5).choice([-1.0, 1.0], b - a).astype(np.float32)
        tr.set_state(bad, good[1], good[2], good[3])
        before = tr.get_state()
        assert _same_state(before, (bad, good[1], good[2], good[3]))
        for unbalanced in (False, True):
            with pytest.raises(_lib.DeepModHipError) as exc:
                tr.step(x, y, unbalanced)
            assert "not finite" in str(exc.value)
            with pytest.raises(_lib.DeepModHipError) as exc:
                tr.grad(x, y, unbalanced)
            assert "not finite" in str(exc.value)
            assert _same_state(before, tr.get_state())
        tr.set_state(*good)
        tr.step(x, y)
        after = tr.get_state()
        assert after[3] == 2 and np.isfinite(after[0]).all() and not np.array_equal(after[0], good[0])
    finally:
        tr.close()


def test_an_empty_batch_gives_a_zero_gradient(gpu_device):
    tr = train.Trainer(_weights("synthetic"), device=gpu_device, max_batch=16)
    try:
        x, y = _batch(4, 3)
        tr.step(x, y)
        before = tr.get_state()
        for _ in range(2):                                    # np.empty would hand back the freed gradient of the call before
            big = tr.grad(x, y)[2]
            assert np.abs(big).max() > 0
            del big
            loss, prob, g = tr.grad(x[:0], y[:0])
            assert loss == 0.0 and prob.shape == (0, 2) and prob.dtype == np.float32
            assert g.shape == (oracle.NW,) and g.dtype == np.float32 and not g.any()
        assert tr.grad(x[:0], y[:0], want_prob=False, want_grad=False) == (0.0, None, None)
        assert _same_state(before, tr.get_state())
    finally:
        tr.close()


def _adam_blobs(rng):
    g = rng.standard_normal(oracle.NW).astype(np.float32) * np.float32(1e-2)
    g[::7] = 0.0
    g[1::11] = np.float32(1e-41) * rng.integers(-9, 10, g[1::11].size).astype(np.float32)       # denormals
    g[2::13] = np.float32(1e15) * rng.choice([-1.0, 1.0], g[2::13].size).astype(np.float32)     # large
    g[3::1001] = np.float32(3e19) * rng.choice([-1.0, 1.0], g[3::1001].size).astype(np.float32)  # g * g overflows: v = inf, the update is 0
    return g


def test_adam_is_bit_equal_to_the_numpy_statement(gpu_device):
    rng = np.random.default_rng(77)
    w = _weights("synthetic")
    m, v = np.zeros_like(w), np.zeros_like(w)
    tr = train.Trainer(w, device=gpu_device, max_batch=16)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for t in (1, 2, 3):
            g = _adam_blobs(rng)
            tr.adam(g)
            w, m, v = oracle.adam_numpy_f32(w, m, v, g, t)
            gw, gm, gv, gt = tr.get_state()
            assert gt == t
            for name, a, b in (("w", gw, w), ("m", gm, m), ("v", gv, v)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
        # t = 1,000 through set_state, from a state with its own zeros / denormals / large entries
        w = _weights("trained")
        m = _adam_blobs(rng)
        v = np.abs(_adam_blobs(rng))
        v[3::1001] = np.float32(1e30)
        g = _adam_blobs(rng)
        tr.set_state(w, m, v, 999)
        tr.adam(g)
        w, m, v = oracle.adam_numpy_f32(w, m, v, g, 1000)
        gw, gm, gv, gt = tr.get_state()
        assert gt == 1000
        for name, a, b in (("w", gw, w), ("m", gm, m), ("v", gv, v)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (1000, name)
    tr.close()


def _same_state(a, b):
    return a[3] == b[3] and all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a[:3], b[:3]))


def test_step_is_grad_then_adam_and_runs_are_bit_identical(gpu_device):
    flat = _weights("trained")
    a, b, c = (train.Trainer(flat, device=gpu_device, max_batch=200) for _ in range(3))
    for i, n in enumerate((129, 200, 17)):
        x, y = _batch(n, 7000 + i)
        la = a.step(x, y, unbalanced=bool(i & 1))
        lb, _, g = b.grad(x, y, unbalanced=bool(i & 1))
        b.adam(g)
        lc = c.step(x, y, unbalanced=bool(i & 1))
        assert np.float32(la).tobytes() == np.float32(lb).tobytes() == np.float32(lc).tobytes()
    sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
    assert sa[3] == 3
    assert _same_state(sa, sb)         # composition
    assert _same_state(sa, sc)         # determinism: two trainers, the same three batches
    assert not np.array_equal(sa[0], flat)
    for t in (a, b, c):
        t.close()


def test_refusals_leave_the_state_unchanged(gpu_device):
    from deepmod_amd import _lib
    tr = train.Trainer(_weights("synthetic"), device=gpu_device, max_batch=32)
    x, y = _batch(20, 9)
    tr.step(x, y)
    before = tr.get_state()
    assert tr.step(x[:0], y[:0]) == 0.0                      # n = 0: a no-op
    assert _same_state(before, tr.get_state())
    xb, yb = _batch(33, 10)
    with pytest.raises(_lib.DeepModHipError) as exc:
        tr.step(xb, yb)
    assert "max_batch" in str(exc.value)
    assert _same_state(before, tr.get_state())
    for bad in (np.nan, np.inf):
        xn = x.copy()
        xn[7, 3, 4] = bad
        with pytest.raises(_lib.DeepModHipError) as exc:
            tr.step(xn, y)
        assert "NaN or Inf" in str(exc.value)
        with pytest.raises(_lib.DeepModHipError):
            tr.grad(xn, y)
        assert _same_state(before, tr.get_state())
    yn = y.copy()
    yn[0, 0] = np.nan
    with pytest.raises(_lib.DeepModHipError):
        tr.step(x, yn)
    assert _same_state(before, tr.get_state())
    tr.step(x, y)                                            # and the trainer still works
    assert tr.get_state()[3] == 2
    tr.close()


LEARN_SEED, LEARN_STEPS, LEARN_N = 3, 40, 256


def planted_batches():
    spec = importlib.util.spec_from_file_location("_make_trained_like", os.path.join(GOLDEN, "make_trained_like.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(LEARN_SEED)
    tables = (rng.normal(0.0, 1.2, 4 ** 5), rng.normal(0.0, 0.8, 4 ** 5))
    out = []
    for _ in range(LEARN_STEPS):
        x, lab = mod.planted_windows(LEARN_N, rng, tables)
        out.append((x, np.eye(2, dtype=np.float32)[lab]))
    return out


def test_learning_follows_the_float64_trajectory(gpu_device):
    """40 Adam steps of n = 256 on planted-signal windows from the seeded initialisation.  LEARN_SEED was chosen on the CPU: the float64 oracle
    alone drops from 0.537 to 0.317 (by 0.22, measured on the CPU) over these batches."""
    flat = model.flatten_weights(train.initial_weights(LEARN_SEED))
    batches = planted_batches()
    l64 = oracle.train_trajectory(flat, batches, oracle.torch.float64)
    l32 = oracle.train_trajectory(flat, batches, oracle.torch.float32)
    tr = train.Trainer(flat, device=gpu_device, max_batch=LEARN_N)
    lg = np.array([tr.step(x, y) for x, y in batches], np.float64)
    tr.close()
    d_gpu, d_32 = np.abs(lg - l64), np.abs(l32 - l64)
    for i in range(LEARN_STEPS):
        print("learn step %2d loss64=%.6f gpu-64=%.3g f32-64=%.3g ratio=%.3g" % (i, l64[i], d_gpu[i], d_32[i], (d_gpu[i] - U * l64[i]) / max(d_32[i], 1e-300)))
    drop = l64[0] - l64[-1]
    assert drop > 0.1
    assert np.all(d_gpu <= R_L * d_32 + U * np.abs(l64))
    assert lg[0] - lg[-1] >= 0.5 * drop


def test_model_session_trains_and_saves(gpu_device, tmp_path):
    """The seam the reference's train_save_model uses: model.mCreateSession's tuple on a model.Session - sess.run([train_op, loss_op], feed) steps
    the trainer, a batch beyond the tape makes it grow with its state kept, saver.save writes a bundle detect's loader reads back."""
    from deepmod_amd import tfbundle
    init, init_l, loss_op, accuracy, train_op, X, Y, saver, auc_op, mpre, mspf, mfpred = \
        model.mCreateSession(7, 100, 21, {"outputlayer": "", "unbalanced": 0, "seed": 2, "max_batch": 16})
    sess = model.new_session(gpu_device)
    ref = train.Trainer(train.initial_weights(2), device=gpu_device, max_batch=40)
    try:
        sess.run(init)
        sess.run(init_l)
        for n in (16, 40):                                    # 40 > the tape of 16 windows
            x, y = _batch(n, 300 + n)
            got = sess.run([train_op, loss_op], feed_dict={X: x, Y: y})
            assert got[0] is None and np.float32(got[1]).tobytes() == np.float32(ref.step(x, y)).tobytes()
        assert sess._train.trainer.max_batch >= 40
        assert _same_state(sess._train.trainer.get_state(), ref.get_state())
        x, y = _batch(9, 77)
        loss, auc, acc, p, r = sess.run([loss_op, auc_op[1], accuracy, mpre[1], mspf[1]], feed_dict={X: x, Y: y})
        want_loss, prob, _ = ref.grad(x, y, want_grad=False)
        assert np.float32(loss).tobytes() == np.float32(want_loss).tobytes()
        assert acc == np.float32((np.argmax(prob, 1) == np.argmax(y, 1)).mean()) and 0.0 <= auc <= 1.0 and 0.0 <= p <= 1.0 and 0.0 <= r <= 1.0
        assert _same_state(sess._train.trainer.get_state(), ref.get_state())      # a fetch without train_op changes nothing
        prefix = str(tmp_path / "ck" / "m")
        os.makedirs(os.path.dirname(prefix))
        saver.save(sess, prefix)
        w = ref.get_state()[0]
        back = tfbundle.load_bundle(prefix)
        assert np.array_equal(model.flatten_weights(back), w)
        assert back["beta1_power"] == np.float32(0.9 ** 3) and len(back) == 44
    finally:
        sess.close()
        ref.close()


def test_train_command_writes_checkpoints_detect_can_run(gpu_device, tmp_path):
    """bin/DeepMod.py train on the fixture folders (small batchsize): the checkpoint folders, the bundle's names and shapes, and a detect run on
    the new --modfile."""
    import glob
    import json
    import subprocess
    import sys
    from deepmod_amd import predstore, synth_reads, tfbundle
    out = str(tmp_path / "trained") + "/"
    fix = os.path.join(GOLDEN, "train")
    cmd = [sys.executable, os.path.join(ROOT, "bin", "DeepMod.py"), "train", "--wrkBase", "%s;%s" % (os.path.join(fix, "neg"), os.path.join(fix, "pos")),
           "--FileID", "mod_train", "--outFolder", out, "--batchsize", "8", "--seed", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Training Finished!" in r.stdout
    # the real saver wrote exactly the checkpoints the reference's schedule asks for on these folders (the two_groups recording)
    saves = [str(p) for p in np.load(os.path.join(fix, "schedule.npz"))["two_groups|saves"]]
    assert {"0.50/mod_train", "4/mod_train"} <= set(saves)
    written = sorted(os.path.relpath(p, out)[:-len(".index")] for p in glob.glob(os.path.join(out, "*", "*.index")))
    assert written == sorted(saves)
    for s in saves:
        assert os.path.isfile(os.path.join(out, os.path.dirname(s), "checkpoint")), s
    prefix = os.path.join(out + "4", "mod_train")
    assert tfbundle.latest_checkpoint(out + "4") == prefix
    want = json.load(open(os.path.join(GOLDEN, "index_tables.json")))["rnn_conmodC_P100wd21_f7ne1u0_4"]["entries"]
    got = tfbundle.read_index(prefix + ".index")
    assert sorted(got) == sorted(want)
    for name, e in want.items():
        assert tuple(got[name].shape) == tuple(e["shape"]), name
    # detect with the new model = the trainer's own forward on the same windows
    tensors = tfbundle.load_bundle(prefix, names=[n for n, _ in train.blob_names()])
    files = synth_reads.write_synthetic_run(str(tmp_path / "reads"), n_reads=3, reads_per_file=3, genome_len=4000, seed=5, min_len=200, max_len=400)
    det = str(tmp_path / "det")
    cmd = [sys.executable, os.path.join(ROOT, "bin", "DeepMod.py"), "detect", "--wrkBase", str(tmp_path / "reads"), "--modfile", prefix, "--FileID", "d",
           "--outFolder", det, "--threads", "1", "--gpus", "1", "--storePred", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, DEEPMOD_PRECISION="f32"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    stores = glob.glob(os.path.join(det, "**", "rnn.pred.detail.npz.*"), recursive=True)
    assert stores
    got_pred = {}
    for path in stores:
        st = predstore.load_pred_store(path)
        assert st["format"] == 2
        for key, attrs in st["attrs"].items():
            lo, hi = predstore.pred_rows(st, key)
            got_pred[attrs["readk"]] = st["mod_pred"][lo:hi]
    tr = train.Trainer(tensors, device=gpu_device, max_batch=4096)
    checked = 0
    for f in files:
        for rd in predstore.load_feature_container(f):
            tx = rd["mfeatures"][:, 3:].astype(np.float32)                    # detect.mPredict1: window k is centred on row 100 + k
            n = len(rd["events"]) - rd["start_clip"] - rd["end_clip"]
            x = np.stack([tx[100 + k - 10:100 + k + 11] for k in range(n)])
            _, prob, _ = tr.grad(x, np.tile(np.float32([1, 0]), (n, 1)), want_grad=False)
            aligned = np.flatnonzero(rd["base_map_info"]["readbase"] != "-")[:n]
            decided = np.abs(prob[:, 1] - 0.5) > TOL
            assert np.array_equal(got_pred[rd["readk"]][aligned][decided], np.argmax(prob, 1)[decided].astype(np.int8)), rd["readk"]
            checked += int(decided.sum())
    tr.close()
    assert checked > 500
