"""Test helper: torch-CPU autograd of the CpG-cluster training graph (the reference's Cg.cov5.nb25.meta) with explicit dropout masks, in float64
and float32.  layer_1 = relu(X W_1 + b_1); d_1 = layer_1 / keep_prob * keep_1; layer_2 = relu(d_1 W_2 + b_2); d_2 = layer_2 / keep_prob * keep_2;
output = sigmoid(d_2 W_O + b_O); loss = mean((output - Y)^2).  The blob is cluster.flatten_cluster_weights' (W_1 b_1 W_2 b_2 W_O b_O); a mask is
[n, 120]: units 0..99 of layer 1, then the 20 of layer 2.  Adam is tests/train_oracle.py's."""
import numpy as np
import torch

from train_oracle import BETA1, BETA2, EPS, adam_numpy_f32, lr_t  # noqa: F401  (adam_numpy_f32: what the GPU Adam is held bit-equal to)

NW = 3541
SLICES = [("W_1", 0, 1400, (14, 100)), ("b_1", 1400, 1500, (100,)), ("W_2", 1500, 3500, (100, 20)), ("b_2", 3500, 3520, (20,)),
          ("W_O", 3520, 3540, (20, 1)), ("b_O", 3540, 3541, (1,))]
VARIANTS = ("graph", "noscale", "mask1only", "sumloss")      # the graph, and three deliberately broken forms (the oracle's teeth)


def _t(blob, i):
    _, a, b, shape = SLICES[i]
    return blob[a:b].reshape(shape)


def forward(blob, x, keep, kp, variant="graph"):
    """output [n] of blob (torch) on rows x [n,14] with mask keep [n,120] (torch, the same dtype)."""
    k1, k2 = keep[:, :100], keep[:, 100:]
    l1 = torch.relu(x @ _t(blob, 0) + _t(blob, 1))
    d1 = l1 * k1 if variant == "noscale" else l1 / kp * k1
    l2 = torch.relu(d1 @ _t(blob, 2) + _t(blob, 3))
    if variant == "mask1only":
        d2 = l2
    else:
        d2 = l2 * k2 if variant == "noscale" else l2 / kp * k2
    return torch.sigmoid(d2 @ _t(blob, 4) + _t(blob, 5))[:, 0]


def loss_of(out, y, variant="graph"):
    sq = (out - y) ** 2
    return sq.sum() if variant == "sumloss" else sq.mean()


def loss_and_grad(flat, x, y, keep, kp, dtype=torch.float64, variant="graph"):
    """-> (loss float, grad float64 ndarray [3541] in blob layout, output float64 ndarray [n]) computed in `dtype`."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    blob = torch.tensor(np.asarray(flat, np.float32), dtype=dtype, requires_grad=True)
    xt = torch.tensor(np.asarray(x, np.float32), dtype=dtype)
    yt = torch.tensor(np.asarray(y, np.float32), dtype=dtype)
    kt = torch.tensor(np.asarray(keep, np.float32), dtype=dtype)
    out = forward(blob, xt, kt, torch.tensor(np.float32(kp), dtype=dtype), variant)
    loss = loss_of(out, yt, variant)
    (g,) = torch.autograd.grad(loss, blob)
    return float(loss.detach()), g.detach().double().numpy(), out.detach().double().numpy()


def tensor_errors(g, g64):
    """e(T) = max|g - g64| / max|g64| of the six tensors; a tensor whose float64 gradient is identically zero: 0.0 if g is exactly zero, else inf."""
    out = {}
    for name, a, b, _ in SLICES:
        top = float(np.abs(g64[a:b]).max())
        if top == 0.0:
            out[name] = 0.0 if not np.any(g[a:b]) else float("inf")
        else:
            out[name] = float(np.abs(g[a:b] - g64[a:b]).max() / top)
    return out


def train_trajectory(flat, batches, kp, dtype):
    """Adam (TF1 form) on the batches [(x, y, keep), ...] in `dtype` -> loss before each update."""
    w = torch.tensor(np.asarray(flat, np.float32), dtype=dtype)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    kpt = torch.tensor(np.float32(kp), dtype=dtype)
    losses = []
    for t, (x, y, keep) in enumerate(batches, 1):
        wr = w.clone().requires_grad_(True)
        out = forward(wr, torch.tensor(np.asarray(x, np.float32), dtype=dtype), torch.tensor(np.asarray(keep, np.float32), dtype=dtype), kpt)
        loss = loss_of(out, torch.tensor(np.asarray(y, np.float32), dtype=dtype))
        (g,) = torch.autograd.grad(loss, wr)
        m = BETA1 * m + (1 - BETA1) * g
        v = BETA2 * v + (1 - BETA2) * g * g
        w = w - torch.tensor(lr_t(t), dtype=dtype) * m / (torch.sqrt(v) + EPS)
        losses.append(float(loss.detach()))
    return np.array(losses)
