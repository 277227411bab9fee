"""GPU: training of the CpG-cluster model (csrc/cluster_train.hip.inc behind dm_cluster_trainer_*) against torch-CPU float64 autograd of the
reference's training graph with explicit masks (tests/cluster_train_oracle.py, tied to the graph by tests/test_cluster_train_host.py).

Batch sizes, by the tiles of grad_kernel: a v_mfma_f32_16x16x4_f32 k-step takes 4 rows, a wave 64 rows, and a block is one wave:
    1;  3, 4, 5 (k-step);  63, 64, 65 (wave = block);  199 = three blocks and a ragged tail of 7;  max_batch + 1 = 257, which is refused.

The acceptance rule of the gradients is tests/test_gpu_train.py's: for each of the six tensors T, e(T) = max|g - g64| / max|g64|, and

        e_gpu(T) <= R * e32(T) + 2^-23

with e32 torch-CPU float32 autograd against the same float64 result and 2^-23 one unit round-off; a tensor whose float64 gradient is identically
zero must be exactly zero.  The loss and `out` are held by the same rule.

R   = 3     measured 2026-10-19 on one MI355X: the worst (e_gpu - 2^-23) / e32 over all cases below (both weight sets, every n, the fixture's,
            all-ones, two dropout draws' and the row-dropped masks, the loss and `out` included, and the smaller call on a used handle) was 1.89
            (real weights, all-ones mask, n = 63, b_1: e_gpu 2.54e-7 against e32 7.11e-8), x 1.5 run-to-run and compiler margin = 2.83, rounded
            up.  No case had e32 = 0.  The ratio depends on the draw of the masks: a small n leaves few terms and a small e32 (under another
            mask stream a single case, n = 3 with one row dropped, reached 5.94 on b_1 with e_gpu 3.85e-7), so a change of dropout_keep or of the
            cases means measuring again (print the figures: -s).
R_L = 50    measured 2026-10-19: the worst (|loss_gpu - loss64| - 2^-23 loss64) / |loss32 - loss64| over the 40 steps of the two learning runs was
            33.02 (keep_prob 1, step 8: 1.38e-7 against 3.5e-9 - the float32 run lies within the resolution of a float32 loss there), x 1.5 = 49.5,
            rounded up; keep_prob 0.7: 6.25 (step 11).  In absolute figures the GPU trajectory stays within 1.2e-6 (keep_prob 1) and 3.3e-6
            (keep_prob 0.7) of the float64 one; the losses fall from 0.2290 to 0.0811 and from 0.2867 to 0.2499.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cluster_train_oracle as oracle
from conftest import GOLDEN, ROOT
from deepmod_amd import _lib, cluster, cluster_train, tfbundle

pytestmark = pytest.mark.gpu

R = 3
R_L = 50
U = 2.0 ** -23

NS = (1, 3, 4, 5, 63, 64, 65, 199)      # see above
MAX_BATCH = 256
CASE = np.load(os.path.join(GOLDEN, "cluster_train_case.npz"))
XALL = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "cluster_case.npz"))["X"], np.float32)          # 915 feature rows of the synthetic contig
YALL = np.round(np.random.default_rng(11).random(len(XALL)), 3).astype(np.float32)
WEIGHTS = {"real": cluster.flatten_cluster_weights(dict(np.load(os.path.join(GOLDEN, "cluster_weights.npz")))),
           "initial": cluster.flatten_cluster_weights(cluster_train.initial_weights(1))}                # stddev-1 values, large pre-activations
WORST = {"R": (0.0, None), "R_L": (0.0, None)}                                                           # what the measuring job prints


def rows(n, offset=0):
    idx = (offset + 7 * np.arange(n)) % len(XALL)
    return XALL[idx], YALL[idx]


def mask_of(kind, n):
    if kind == "ones":
        return np.ones((n, 120), np.uint8), 1.0
    keep = cluster_train.dropout_keep(5 if kind == "dropout2" else 21, n, n, 0.7)
    if kind == "rowdropped":
        keep[n // 2] = 0
    return keep, 0.7


def fixture_case(n, kp10):
    tag = "_n%d_kp%d" % (n, kp10)
    kp = np.float32(CASE["keep_prob" + tag])
    keep = np.floor(kp + np.concatenate([CASE["u1" + tag], CASE["u2" + tag]], axis=1).astype(np.float32)).astype(np.uint8)
    return CASE["X" + tag], CASE["Y" + tag], keep, float(kp)


GRAD_CASES = [(w, kind, n) for w in ("real", "initial") for kind in ("ones", "dropout", "dropout2", "rowdropped") for n in NS] + \
             [("real", "fixture%d" % kp10, n) for kp10 in (7, 10) for n in (1, 37)]


def case_inputs(case):
    w, kind, n = case
    if kind.startswith("fixture"):
        x, y, keep, kp = fixture_case(n, int(kind[7:]))
    else:
        x, y = rows(n, offset=3 * n)
        keep, kp = mask_of(kind, n)
    return WEIGHTS[w], x, y, keep, kp


def hold_to_oracle(tr, case, flat, x, y, keep, kp):
    """One dm_cluster_trainer_grad call against the float64 oracle by the rule above; prints each figure before it asserts."""
    loss, out, g = tr.grad(x, y, kp, keep)
    l64, g64, o64 = oracle.loss_and_grad(flat, x, y, keep, kp)
    l32, g32, o32 = oracle.loss_and_grad(flat, x, y, keep, kp, dtype=torch.float32)
    e_gpu, e_32 = oracle.tensor_errors(g.astype(np.float64), g64), oracle.tensor_errors(g32, g64)
    e_gpu["loss"], e_32["loss"] = abs(loss - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    e_gpu["out"], e_32["out"] = float(np.abs(out - o64).max()), float(np.abs(o32 - o64).max())
    for k in e_gpu:
        ratio = (e_gpu[k] - U) / e_32[k] if e_32[k] > 0 else (0.0 if e_gpu[k] <= U else float("inf"))
        print("%s %-5s e_gpu=%.3e e32=%.3e ratio=%.2f" % (case, k, e_gpu[k], e_32[k], ratio))
        if ratio > WORST["R"][0]:
            WORST["R"] = (ratio, (case, k, e_gpu[k], e_32[k]))
    for k in e_gpu:
        assert e_gpu[k] <= R * e_32[k] + U, (case, k, e_gpu[k], e_32[k])


@pytest.fixture(scope="module")
def trainers(gpu_device):
    made = {k: cluster_train.ClusterTrainer(w, gpu_device, max_batch=MAX_BATCH) for k, w in WEIGHTS.items()}
    yield made
    for t in made.values():
        t.close()


def fresh(gpu_device, which="real"):
    return cluster_train.ClusterTrainer(WEIGHTS[which], gpu_device, max_batch=MAX_BATCH)


def states_equal(a, b):
    return a[3] == b[3] and all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("which", ["real", "initial"])
def test_forward_at_keep_prob_1_is_the_scoring_kernel_bit_for_bit(trainers, gpu_device, which):
    model = cluster.ClusterModel(cluster_train.unflatten_cluster_weights(WEIGHTS[which]), gpu_device)
    for n in NS:
        x, y = rows(n, offset=n)
        _, out, _ = trainers[which].grad(x, y, 1.0, np.ones((n, 120), np.uint8), want_grad=False)
        assert out.tobytes() == model.predict(x).tobytes(), n
        _, out2, _ = trainers[which].grad(x, y, 1.0, None, seed=5, step=n, want_grad=False)        # the generated mask at keep_prob 1: all ones
        assert out2.tobytes() == out.tobytes(), n
    model.close()


@pytest.mark.parametrize("which", ["real", "initial"])
def test_gradients_loss_and_out_against_float64_autograd(trainers, which):
    """R = see the module docstring.  Fixture masks, all-ones masks, dropout masks and a mask with one row fully dropped, at every n."""
    for case in [c for c in GRAD_CASES if c[0] == which]:
        hold_to_oracle(trainers[which], case, *case_inputs(case))
    print("worst ratio so far:", WORST["R"])


def test_generated_mask_is_dropout_keep_and_null_mask_is_that_mask(trainers):
    tr = trainers["initial"]
    for n in NS:
        keep = tr.mask(17, n + 2, n, 0.7)
        assert keep.tobytes() == cluster_train.dropout_keep(17, n + 2, n, 0.7).tobytes(), n
        x, y = rows(n, offset=5)
        a, b = tr.grad(x, y, 0.7, None, seed=17, step=n + 2), tr.grad(x, y, 0.7, keep)
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), n
    assert tr.mask(2 ** 63 + 5, 0, 3, 0.7).tobytes() == cluster_train.dropout_keep(2 ** 63 + 5, 0, 3, 0.7).tobytes()
    assert tr.mask(1, 0, 64, 1.0).all()


def test_adam_is_bit_equal_to_the_numpy_statement(gpu_device):
    rng = np.random.default_rng(3)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-38, 1e18, -1e18, 3e-7, -3e-7, 1.0, -1.0], np.float32)
    g = rng.standard_normal(oracle.NW).astype(np.float32) * np.float32(1e-3)
    g[:600] = np.tile(special, 50)
    w = rng.standard_normal(oracle.NW).astype(np.float32)
    m = rng.standard_normal(oracle.NW).astype(np.float32) * np.float32(1e-3)
    v = (rng.standard_normal(oracle.NW).astype(np.float32) * np.float32(1e-3)) ** 2
    m[:1200] = np.repeat(np.array([0.0, 1e-40], np.float32), 600)
    v[:1200] = np.repeat(np.array([0.0, 1e-41], np.float32), 600)
    tr = fresh(gpu_device)
    with np.errstate(all="ignore"):
        for t in (1, 2, 3, 1000):
            tr.set_state(w, m, v, t - 1)
            tr.adam(g)
            got = tr.get_state()
            want = oracle.adam_numpy_f32(w, m, v, g, t)
            assert got[3] == t
            for a, b, name in zip(got[:3], want, "wmv"):
                assert a.tobytes() == b.astype(np.float32).tobytes(), (t, name)
    tr.close()


def test_step_is_grad_plus_adam_and_runs_are_bit_identical(gpu_device):
    n = 199
    ids = np.concatenate([[0, len(XALL) - 1, 5, 5, 5], np.arange(150, 50, -1), np.random.default_rng(2).integers(0, len(XALL), n - 105)]).astype(np.int64)
    assert len(ids) == n
    a, b = fresh(gpu_device, "initial"), fresh(gpu_device, "initial")
    a.set_data(XALL, YALL)
    for step, batch in enumerate((ids, ids[::-1][:65], ids[:1])):                   # the mask follows the handle's step count; a smaller batch after a larger
        a.step(batch, 0.7, seed=9)
        keep = b.mask(9, step, len(batch), 0.7)
        loss, _, g = b.grad(XALL[batch], YALL[batch], 0.7, keep)
        b.adam(g)
        assert states_equal(a.get_state(), b.get_state()), step
        assert a.losses(step, 1)[0] == np.float32(loss), step
    assert a.get_state()[3] == 3 and a.losses(0, 3).shape == (3,)
    # the smaller batch after the larger ones is still held to the oracle, on the weights the handle has now
    x, y = rows(5, offset=40)
    keep, kp = mask_of("dropout", 5)
    hold_to_oracle(a, ("initial+3 steps", "dropout", 5), a.get_state()[0], x, y, keep, kp)
    # two handles, 20 steps each
    c, d = fresh(gpu_device, "initial"), fresh(gpu_device, "initial")
    for h in (c, d):
        h.set_data(XALL, YALL)
        for step in range(20):
            h.step(np.random.default_rng([4, step]).integers(0, len(XALL), 64 + step), 0.7, seed=1)
    assert states_equal(c.get_state(), d.get_state()) and c.losses(0, 20).tobytes() == d.losses(0, 20).tobytes()
    assert not states_equal(c.get_state(), a.get_state())
    for h in (a, b, c, d):
        h.close()


def test_refusals_leave_the_state_unchanged(gpu_device):
    tr = fresh(gpu_device)
    lib = _lib.load()
    x, y = rows(9)
    tr.adam(np.full(oracle.NW, 1e-3, np.float32))                                   # a state with m, v and t set
    before = tr.get_state()

    def refused(call, *args):
        with pytest.raises(_lib.DeepModHipError) as exc:
            call(*args)
        assert exc.value.code == _lib.DM_EINVAL and lib.dm_last_error()
        assert states_equal(tr.get_state(), before)
        return str(exc.value)

    assert "no data" in refused(tr.step, np.arange(4), 0.7, 0)                       # step before set_data
    ynan = y.copy()
    ynan[3] = np.nan
    assert "NaN or Inf in y" in refused(tr.grad, x, ynan, 0.7)
    assert "NaN or Inf in y" in refused(tr.set_data, x, ynan)
    xinf = x.copy()
    xinf[2, 7] = np.inf
    assert "NaN or Inf in x" in refused(tr.grad, xinf, y, 0.7)
    tr.set_data(x, y)
    assert "outside [0, 9)" in refused(tr.step, np.array([0, 9]), 0.7, 0)
    assert "outside [0, 9)" in refused(tr.step, np.array([-1]), 0.7, 0)
    assert "keep_prob" in refused(tr.step, np.array([0]), 0.0, 0)
    big_x, big_y = rows(MAX_BATCH + 1)
    assert "exceed max_batch" in refused(tr.grad, big_x, big_y, 0.7)                 # max_batch + 1 is refused, nothing grows
    assert "exceed max_batch" in refused(tr.step, np.zeros(MAX_BATCH + 1, np.int64), 0.7, 0)
    assert "not all among the recorded steps" in refused(tr.losses, 0, 1)
    tr.step(np.arange(9), 0.7, 0)                                                   # and the handle still works
    assert tr.get_state()[3] == before[3] + 1 and np.isfinite(tr.losses(before[3], 1)).all()
    tr.close()


# ---------------------------------------------------------------------------------------------
# learning: a student fits the shipped model's outputs
# ---------------------------------------------------------------------------------------------
def learning_case():
    """2,048 rows (the 915 feature rows tiled, the fractions perturbed within [0, 1]), the teacher's outputs (the real weights at keep_prob 1,
    float64 oracle) as truth, 40 batches of 256 consecutive rows."""
    rng = np.random.default_rng(2026)
    x = XALL[np.arange(2048) % len(XALL)].astype(np.float64)
    frac = [0, 1] + list(range(3, 14))
    x[:, frac] = np.clip(x[:, frac] + rng.uniform(-0.05, 0.05, (2048, len(frac))), 0.0, 1.0)
    x = np.ascontiguousarray(x, np.float32)
    ones = np.ones((2048, 120), np.uint8)
    _, _, y = oracle.loss_and_grad(WEIGHTS["real"], x, np.zeros(2048, np.float32), ones, 1.0)
    ids = [np.arange(256 * (s % 8), 256 * (s % 8) + 256, dtype=np.int64) for s in range(40)]
    return x, y.astype(np.float32), ids


@pytest.mark.parametrize("kp", [1.0, 0.7])
def test_learning_follows_the_float64_trajectory(gpu_device, kp):
    """R_L = see the module docstring."""
    x, y, ids = learning_case()
    start = cluster.flatten_cluster_weights(cluster_train.initial_weights(0))
    batches = [(x[b], y[b], cluster_train.dropout_keep(0, s, 256, kp)) for s, b in enumerate(ids)]
    l64 = oracle.train_trajectory(start, batches, kp, torch.float64)
    l32 = oracle.train_trajectory(start, batches, kp, torch.float32)
    tr = cluster_train.ClusterTrainer(start, gpu_device, max_batch=256)
    tr.set_data(x, y)
    for b in ids:
        tr.step(b, kp, seed=0)
    got = tr.losses(0, 40).astype(np.float64)
    tr.close()
    d_gpu, d_32 = np.abs(got - l64), np.abs(l32 - l64)
    ratio = np.where(d_32 > 0, (d_gpu - U * np.abs(l64)) / np.where(d_32 > 0, d_32, 1.0), np.where(d_gpu <= U * np.abs(l64), 0.0, np.inf))
    s = int(np.argmax(ratio))
    print("keep_prob %.1f: loss %.6f -> %.6f (float64 %.6f -> %.6f); worst ratio %.2f at step %d: |gpu - 64| = %.3e, |32 - 64| = %.3e; max |gpu - 64| = %.3e" %
          (kp, got[0], got[-1], l64[0], l64[-1], ratio[s], s, d_gpu[s], d_32[s], d_gpu.max()))
    if ratio[s] > WORST["R_L"][0]:
        WORST["R_L"] = (float(ratio[s]), (kp, s, float(d_gpu[s]), float(d_32[s])))
    assert l64[-1] < l64[0]
    assert got[-1] < got[0]
    assert np.all(d_gpu <= R_L * d_32 + U * np.abs(l64))


# ---------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------
def synthetic_contig(rng, chrom, length=6000):
    """Motif table, DeepMod BED and planted bedMethyl truth of one contig (the shape of tests/golden/make_golden_cluster.py's generator, every
    row with coverage): the truth of a site is its own fraction pulled half way toward the mean of its neighbourhood."""
    seq = rng.choice(list("ACGT"), length, p=[.2, .3, .3, .2])
    motif, bed = [], []
    for p in range(length - 1):
        if seq[p] == "C" and seq[p + 1] == "G":
            motif += ["%s %d + C\n" % (chrom, p), "%s %d - C\n" % (chrom, p + 1)]
    for line in motif:
        c, p, s, _ = line.split()
        if rng.random() < 0.85:
            cov = int(rng.integers(1, 40))
            mod = int(rng.integers(0, cov + 1))
            bed.append("%s %s %d C %d %s %s %d 0,0,0 %d %d %d\n" % (c, p, int(p) + 1, cov, s, p, int(p) + 1, cov, int(100 * mod / cov), mod))
    return "".join(motif), "".join(bed)


def planted_truth(pred_path, motif_path, chrom):
    pred = cluster.read_pred(pred_path, chrom, cluster.read_motif(motif_path))
    x, _ = cluster.cluster_features(pred)
    mean = np.where(x[:, 2] > 0, x[:, 3:] @ (np.arange(11) / 10.0), x[:, 0])
    pct = np.rint(100 * (0.5 * x[:, 0] + 0.5 * mean)).astype(int)
    keys = [(s, int(p)) for s in "+-" for p in pred[s][0]]
    return "".join("%s %d %d . 10 %s %d %d 0,0,0 10 %d\n" % (chrom, p, p + 1, s, p, p + 1, v) for (s, p), v in zip(keys, pct))


def test_traincluster_command(tmp_path, gpu_device):
    os.makedirs(tmp_path / "motif")
    truth = "track name=planted\n"
    for i, chrom in enumerate(("chr1", "chr2")):
        motif, bed = synthetic_contig(np.random.default_rng(100 + i), chrom)
        (tmp_path / "motif" / ("motif_%s_C.bed" % chrom)).write_text(motif)
        (tmp_path / ("pred.%s.C.bed" % chrom)).write_text(bed)
        truth += planted_truth(str(tmp_path / ("pred.%s.C.bed" % chrom)), str(tmp_path / "motif" / ("motif_%s_C.bed" % chrom)), chrom)
    (tmp_path / "truth.bed").write_text(truth)
    argv = ["--predFile", str(tmp_path / "pred"), "--motifFolder", str(tmp_path / "motif"), "--truth", str(tmp_path / "truth.bed"), "--chr", "chr1",
            "--heldout", "chr2", "--epochs", "2", "--batchsize", "256", "--seed", "3", "--FileID", "fit"]
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "DeepMod.py"), "traincluster"] + argv + ["--outFolder", str(tmp_path / "a")],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["Cg.cov5.nb25-%d.%s" % (e, ext) for e in (1, 2) for ext in ("index", "data-00000-of-00001")] + ["checkpoint", "fit_cluster_train.json"])
    report = json.load(open(tmp_path / "a" / "fit_cluster_train.json"))
    n = report["sites"]["with_truth"]
    assert n > 500 and report["sites"]["without_truth"] == 0 and report["heldout_sites"]["with_truth"] > 500
    assert [e["steps"] for e in report["epochs"]] == [-(-n // 256)] * 2 and report["epochs"][1]["t"] == 2 * -(-n // 256)
    assert all(np.isfinite([e["train_mse"], e["heldout_mse"]]).all() for e in report["epochs"]) and report["best_epoch"] in (1, 2)
    assert tfbundle.latest_checkpoint(str(tmp_path / "a")) == str(tmp_path / "a" / "Cg.cov5.nb25-2")
    last = str(tmp_path / "a" / "Cg.cov5.nb25-2")
    entries = tfbundle.read_index(last + ".index")
    assert sorted(entries) == sorted([k + s for k in cluster.WEIGHT_ORDER for s in ("", "/Adam", "/Adam_1")] + ["beta1_power", "beta2_power"])
    model = cluster.ClusterModel.from_checkpoint(last, gpu_device)
    assert model.predict(XALL[:5]).shape == (5,)
    model.close()
    written = cluster.hm_cluster_predict(str(tmp_path / "pred"), str(tmp_path / "motif"), last, chrkeys=["chr2"], device=gpu_device)
    assert written == [str(tmp_path / "pred_clusterCpG.chr2.C.bed")]
    got = open(written[0]).read().splitlines()
    src = [ln.strip() for ln in open(tmp_path / "pred.chr2.C.bed")]
    assert sorted(ln.rsplit(" ", 1)[0] for ln in got) == sorted(src)
    assert all(0 <= int(ln.rsplit(" ", 1)[1]) <= 100 for ln in got)
    # the same seed writes the same bytes (this time through the module, in this process)
    mo = dict(outLevel=3, FileID="fit", outFolder=str(tmp_path / "b"), predFile=str(tmp_path / "pred"), motifFolder=str(tmp_path / "motif"), cov=5,
              keep_prob=0.7, epochs=2, batchsize=256, seed=3, truth=[str(tmp_path / "truth.bed")], chr=["chr1"], heldout=["chr2"])
    cluster_train.train_cluster(mo, gpu_device)
    for name in names:
        if name.startswith("Cg."):
            assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read(), name
