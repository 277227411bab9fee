"""CPU: training of the CpG-cluster model (deepmod_amd/cluster_train.py) - the oracle tied to the reference's training graph, the oracle's teeth,
the truth reader against the reference's readBed, the dropout mask's definition, the data-set assembly and the command's refusals."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_train_oracle as oracle
from conftest import GOLDEN, ROOT
from deepmod_amd import cluster, cluster_train

CASE = np.load(os.path.join(GOLDEN, "cluster_train_case.npz"))
TRUTH = json.load(open(os.path.join(GOLDEN, "cluster_truth_case.json")))
SITES = json.load(open(os.path.join(GOLDEN, "cluster_case.json")))
REAL = cluster.flatten_cluster_weights(dict(np.load(os.path.join(GOLDEN, "cluster_weights.npz"))))


def fixture_case(n, kp10):
    """(x, y, keep uint8 [n,120], keep_prob float32, output [n], Mean) of the reference graph's run; keep = floor(keep_prob + u) in float32."""
    tag = "_n%d_kp%d" % (n, kp10)
    kp = np.float32(CASE["keep_prob" + tag])
    keep = np.floor(kp + np.concatenate([CASE["u1" + tag], CASE["u2" + tag]], axis=1).astype(np.float32)).astype(np.uint8)
    return CASE["X" + tag], CASE["Y" + tag], keep, kp, CASE["output" + tag].ravel(), float(CASE["Mean" + tag])


@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("kp10", [7, 10])
def test_float64_oracle_reproduces_the_reference_graph(n, kp10):
    """Ties the oracle's dropout and loss to the reference: within 1e-6, the bound tests/test_cluster.py:42 uses for this network against this
    interpreter."""
    x, y, keep, kp, output, mean = fixture_case(n, kp10)
    assert keep.min() >= 0 and keep.max() == 1 and (kp10 == 10) == bool(keep.all())
    loss, _, out = oracle.loss_and_grad(REAL, x, y, keep, kp)
    print("n=%d keep_prob=%.1f max|out - output|=%.3g |loss - Mean|=%.3g" % (n, kp, np.abs(out - output).max(), abs(loss - mean)))
    assert np.abs(out - output).max() <= 1e-6
    assert abs(loss - mean) <= 1e-6


@pytest.mark.parametrize("variant", ["noscale", "mask1only", "sumloss"])
def test_the_oracle_has_teeth(variant):
    """No scaling by keep_prob, a mask on layer 1 only, a summed loss: each moves at least one of the six gradient tensors by more than 100 x the
    float32-vs-float64 distance of the unbroken oracle at n = 37."""
    import torch
    x, y, keep, kp, _, _ = fixture_case(37, 7)
    _, g64, _ = oracle.loss_and_grad(REAL, x, y, keep, kp)
    _, g32, _ = oracle.loss_and_grad(REAL, x, y, keep, kp, dtype=torch.float32)
    _, gbad, _ = oracle.loss_and_grad(REAL, x, y, keep, kp, variant=variant)
    e32, ebad = oracle.tensor_errors(g32, g64), oracle.tensor_errors(gbad, g64)
    print(variant, {k: "%.3g / %.3g" % (ebad[k], e32[k]) for k in e32})
    assert all(v > 0 for v in e32.values())
    assert any(ebad[k] > 100 * e32[k] for k in e32)


def test_read_truth_equals_the_reference_reader(tmp_path):
    path = tmp_path / "truth.bed"
    path.write_text(TRUTH["text"])
    got = cluster_train.read_truth(str(path))
    want = {(c, s, p): v for c, s, p, v in TRUTH["truth"]}
    assert got == want and list(got) == list(want)
    assert cluster_train.read_truth(str(path), chrom="chr2") == {k: v for k, v in want.items() if k[0] == "chr2"}
    assert cluster_train.read_truth(str(path), start=101, end=207) == {k: v for k, v in want.items() if 101 <= k[2] <= 207}
    assert ("chr1", "+", 205) in cluster_train.read_truth(str(path), cov=4)
    bad = tmp_path / "bad.bed"
    bad.write_text("header\nchr1 100 101 . 12 + 100 101 0,255,0 12 83\nchr1 101 102 . 9 - 101 102 0,255,0 9\n")
    with pytest.raises(ValueError, match=r"bad\.bed:3: expected 11 fields"):
        cluster_train.read_truth(str(bad))


def test_dropout_keep():
    assert cluster_train.dropout_keep(3, 5, 64, 1.0).all()
    a = cluster_train.dropout_keep(3, 5, 64, 0.7)
    assert a.shape == (64, 120) and a.dtype == np.uint8 and set(np.unique(a)) == {0, 1}
    assert np.array_equal(a, cluster_train.dropout_keep(3, 5, 64, 0.7))
    assert np.array_equal(a[:9], cluster_train.dropout_keep(3, 5, 9, 0.7))            # a row's mask does not depend on the batch size
    for other in ((3, 6), (4, 5), (5, 3)):
        assert not np.array_equal(a, cluster_train.dropout_keep(other[0], other[1], 64, 0.7))
    share = cluster_train.dropout_keep(0, 0, 8334, 0.7).mean()                         # 1,000,080 draws
    print("kept share %.5f" % share)
    assert abs(share - 0.7) <= 0.002                                                   # about 4 sigma of a binomial share


def _write_sites(tmp_path, chrom="chr1"):
    os.makedirs(tmp_path / "motif", exist_ok=True)
    (tmp_path / "motif" / ("motif_%s_C.bed" % chrom)).write_text(SITES["motif"].replace("chr1", chrom))
    (tmp_path / ("pred.%s.C.bed" % chrom)).write_text(SITES["pred_bed"].replace("chr1", chrom))
    return str(tmp_path / "pred"), str(tmp_path / "motif")


def test_dataset_rows_are_the_feature_rows_at_the_truth_keys(tmp_path):
    pred_prefix, motif_folder = _write_sites(tmp_path)
    pred = cluster.read_pred(pred_prefix + ".chr1.C.bed", "chr1", cluster.read_motif(motif_folder + "/motif_chr1_C.bed"))
    x_all, _ = cluster.cluster_features(pred)
    keys = [("chr1", s, int(p)) for s in "+-" for p in pred[s][0]]
    rng = np.random.default_rng(7)
    chosen = sorted(rng.choice(len(keys), len(keys) // 3, replace=False).tolist())
    truth = {keys[i]: round(float(rng.integers(0, 101)) / 100.0, 3) for i in reversed(chosen)}      # the dictionary's order must not matter
    truth[("chr1", "+", 10 ** 7)] = 0.5                                                             # truth without a site
    truth[("chr9",) + keys[0][1:]] = 0.5
    x, y, counts = cluster_train.build_dataset(pred_prefix, motif_folder, truth, ["chr1"])
    assert x.dtype == np.float32 and y.dtype == np.float32
    assert np.array_equal(x, x_all[chosen].astype(np.float32))
    assert np.array_equal(y, np.array([truth[keys[i]] for i in chosen], np.float32))
    assert counts == {"with_truth": len(chosen), "without_truth": len(keys) - len(chosen), "per_contig": {"chr1": [len(chosen), len(keys) - len(chosen)]}}
    # a site without truth is no row, but still a neighbour: the rows count more neighbours than the truth sites alone would give
    only = {}
    for s in "+-":
        idx = [i for i, p in enumerate(pred[s][0]) if ("chr1", s, int(p)) in truth]
        only[s] = (pred[s][0][idx], pred[s][1][idx], [pred[s][2][i] for i in idx])
    x_only, _ = cluster.cluster_features(only)
    assert x_only.shape == x.shape and (x[:, 2] >= x_only[:, 2]).all() and (x[:, 2] > x_only[:, 2]).any()


def test_initial_weights_and_checkpoint_tensors():
    w = cluster_train.initial_weights(0)
    assert [w[k].shape for k in cluster.WEIGHT_ORDER] == [(14, 100), (100,), (100, 20), (20,), (20, 1), (1,)]
    assert all(not w[k].any() for k in ("b_1", "b_2", "b_O")) and all(np.abs(w[k]).max() <= 2.0 for k in w)
    assert 0.8 < w["W_2"].std() < 0.95                                                 # a standard normal cut at 2 sigma: 0.88
    flat = cluster.flatten_cluster_weights(w)
    assert np.array_equal(flat, cluster.flatten_cluster_weights(cluster_train.initial_weights(0)))
    assert not np.array_equal(flat, cluster.flatten_cluster_weights(cluster_train.initial_weights(1)))
    t = cluster_train.checkpoint_tensors(flat, flat * 0, flat * 0 + 1, 3)
    assert sorted(t) == sorted([k + s for k in cluster.WEIGHT_ORDER for s in ("", "/Adam", "/Adam_1")] + ["beta1_power", "beta2_power"])
    assert t["W_O/Adam_1"].shape == (20, 1) and t["beta1_power"].shape == () and t["beta1_power"] == np.float32(0.9 ** 4)


# ---------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------
def _deepmod():
    spec = importlib.util.spec_from_file_location("_deepmod_cli", os.path.join(ROOT, "bin", "DeepMod.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _refusal(argv):
    cli = _deepmod()
    args = cli.build_parser().parse_args(["traincluster"] + argv)
    with pytest.raises(SystemExit) as exc:
        args.func(args)
    msg = str(exc.value)
    assert msg.startswith("Error: ") and "\n" not in msg
    return msg


def test_cli_refusals(tmp_path):
    pred_prefix, motif_folder = _write_sites(tmp_path)
    _write_sites(tmp_path, "chr2")
    truth = tmp_path / "truth.bed"
    truth.write_text(TRUTH["text"])                                                    # none of its positions is a site of the synthetic contig
    base = ["--predFile", pred_prefix, "--motifFolder", motif_folder, "--truth", str(truth), "--outFolder", str(tmp_path / "out")]
    assert "--keep_prob 0 outside (0, 1]" in _refusal(base + ["--keep_prob", "0"])
    assert "--keep_prob 1.5 outside (0, 1]" in _refusal(base + ["--keep_prob", "1.5"])
    assert "contig chr2 is named in both --chr and --heldout" in _refusal(base + ["--chr", "chr1,chr2", "--heldout", "chr2"])
    assert "no file %s" % (tmp_path / "nothing.bed") in _refusal(base[:4] + ["--truth", str(tmp_path / "nothing.bed")])
    assert "no file %s.chr3.C.bed" % pred_prefix in _refusal(base + ["--chr", "chr3"])
    assert "no file %s/motif_chr1_C.bed" % (tmp_path / "nomotif") in _refusal(base[:2] + ["--motifFolder", str(tmp_path / "nomotif")] + base[4:])
    assert "no site of chr1 has truth" in _refusal(base)
    short = tmp_path / "short.bed"
    short.write_text("header\nchr1 101 102 . 9 - 101 102 0,255,0 9\n")
    assert "short.bed:2: expected 11 fields" in _refusal(base[:4] + ["--truth", str(short)])
    assert not os.path.exists(tmp_path / "out")


def test_cli_help_and_no_gpu(tmp_path):
    script = os.path.join(ROOT, "bin", "DeepMod.py")
    text = subprocess.run([sys.executable, script, "traincluster", "--help"], capture_output=True, text=True, check=True).stdout
    for flag in ("--predFile", "--motifFolder", "--truth", "--chr", "--heldout", "--cov", "--keep_prob", "--epochs", "--batchsize", "--seed",
                 "--outFolder", "--FileID", "--outLevel"):
        assert flag in text, flag
    assert "project's own" in text
    # with truth on the sites and no device visible the command ends with its one line and writes nothing
    pred_prefix, motif_folder = _write_sites(tmp_path)
    rows = [ln.split() for ln in SITES["pred_bed"].splitlines()[:200]]
    truth = tmp_path / "truth.bed"
    truth.write_text("header\n" + "".join("%s %s %s . 9 %s %s %s 0,0,0 9 50\n" % (r[0], r[1], r[2], r[5], r[1], r[2]) for r in rows))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    run = subprocess.run([sys.executable, script, "traincluster", "--predFile", pred_prefix, "--motifFolder", motif_folder, "--truth", str(truth),
                          "--outFolder", str(tmp_path / "out")], capture_output=True, text=True, env=env)
    assert run.returncode != 0
    assert run.stderr.strip().splitlines()[-1] == "Error: no gfx950 GPU visible (this build has no CPU path)"
    assert not os.path.exists(tmp_path / "out")
