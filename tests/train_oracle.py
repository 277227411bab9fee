"""Training oracle of the tests: torch-CPU autograd of the exact architecture (bin/DeepMod_scripts/myMultiBiRNN.py:21-91 of the reference: two
stacks of three BasicLSTMCell(100, forget_bias=1), gates i, j, f, o, forward stack over rows 0..10, backward stack over rows 20..10, head on
concat(h_fw[10], h_bw[10]), mean softmax cross entropy, class weights [0.1, 0.9] inside the loss's softmax when unbalanced) on the
canonical weight blob of deepmod_amd.model.flatten_weights.  float64 is the reference; the same code in float32 gives the error a correct
fp32 implementation has (the yardstick of tests/test_gpu_train.py).  Only tests import this module (torch is not a dependency of the package).

`forget_bias` and `bw_rows` exist for the tests that show the oracle has teeth: the wrong architecture must miss by a wide margin."""
import numpy as np
import torch

NFEAT, HID, WIN, LIVE = 7, 100, 21, 11
NW = 408402
BETA1, BETA2, EPS, LR = 0.9, 0.999, 1e-8, 1e-3


def tensor_slices():
    """(name, start, stop, shape) of the 14 tensors of the blob, in blob order."""
    out, off = [], 0
    for d in ("fw", "bw"):
        for layer in range(3):
            k = (NFEAT if layer == 0 else HID) + HID
            out.append(("%s%d/kernel" % (d, layer), off, off + k * 400, (k, 400)))
            off += k * 400
            out.append(("%s%d/bias" % (d, layer), off, off + 400, (400,)))
            off += 400
    out.append(("out/W", off, off + 400, (200, 2)))
    off += 400
    out.append(("out/b", off, off + 2, (2,)))
    assert off + 2 == NW
    return out


SLICES = tensor_slices()


def _stack(blob, base, x_rows, forget_bias):
    """x_rows: list of 11 [n,7] tensors in the order the stack sees them -> h of the top cell after the last one."""
    n = x_rows[0].shape[0]
    seq = x_rows
    for layer in range(3):
        _, k0, k1, kshape = SLICES[base + 2 * layer]
        _, b0, b1, _ = SLICES[base + 2 * layer + 1]
        kern, bias = blob[k0:k1].reshape(kshape), blob[b0:b1]
        h = torch.zeros(n, HID, dtype=blob.dtype)
        c = torch.zeros(n, HID, dtype=blob.dtype)
        outs = []
        for inp in seq:
            g = torch.cat([inp, h], 1) @ kern + bias
            i, j, f, o = g[:, :HID], g[:, HID:2 * HID], g[:, 2 * HID:3 * HID], g[:, 3 * HID:]
            c = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
            h = torch.tanh(c) * torch.sigmoid(o)
            outs.append(h)
        seq = outs
    return seq[-1]


def forward(blob, x, forget_bias=1.0, bw_rows=None):
    """logits [n,2] of blob (torch, any float dtype) on windows x [n,21,7] (torch, the same dtype)."""
    fw = [x[:, r, :] for r in range(LIVE)]
    bw = [x[:, r, :] for r in (bw_rows if bw_rows is not None else range(WIN - 1, WIN - 1 - LIVE, -1))]
    hcat = torch.cat([_stack(blob, 0, fw, forget_bias), _stack(blob, 6, bw, forget_bias)], 1)
    _, w0, w1, wshape = SLICES[12]
    _, b0, b1, _ = SLICES[13]
    return hcat @ blob[w0:w1].reshape(wshape) + blob[b0:b1]


def loss_of(logits, y, unbalanced):
    z = logits * torch.tensor([0.1, 0.9], dtype=logits.dtype) if unbalanced else logits
    return (-(y * torch.log_softmax(z, 1)).sum(1)).mean()


def loss_and_grad(flat, x, y, unbalanced=False, dtype=torch.float64, forget_bias=1.0, bw_rows=None):
    """-> (loss float, grad float64 ndarray [408402] in blob layout, prob float64 ndarray [n,2]) computed in `dtype`."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    blob = torch.tensor(np.asarray(flat, np.float32), dtype=dtype, requires_grad=True)
    xt = torch.tensor(np.asarray(x, np.float32), dtype=dtype)
    yt = torch.tensor(np.asarray(y, np.float32), dtype=dtype)
    logits = forward(blob, xt, forget_bias, bw_rows)
    loss = loss_of(logits, yt, unbalanced)
    (g,) = torch.autograd.grad(loss, blob)
    return float(loss.detach()), g.detach().double().numpy(), torch.softmax(logits.detach(), 1).double().numpy()


def tensor_errors(g, g64):
    """e(T) = max|g - g64| / max|g64| of the 14 tensors."""
    return {name: float(np.abs(g[a:b] - g64[a:b]).max() / np.abs(g64[a:b]).max()) for name, a, b, _ in SLICES}


def lr_t(t):
    return LR * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t)


def adam_numpy_f32(w, m, v, g, t):
    """The float32 statement dm_trainer_adam is held bit-equal to: one rounding per operation, in this order."""
    f = np.float32
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    lr = f(lr_t(t))
    m = b1 * m + omb1 * g
    v = b2 * v + omb2 * (g * g)
    w = w - (lr * m) / (np.sqrt(v) + eps)
    return w, m, v


def train_trajectory(flat, batches, dtype, unbalanced=False):
    """Adam (TF1 form) on the given batches [(x, y), ...] in `dtype` -> loss before each update."""
    w = torch.tensor(np.asarray(flat, np.float32), dtype=dtype)
    m, v = torch.zeros_like(w), torch.zeros_like(w)
    losses = []
    for t, (x, y) in enumerate(batches, 1):
        wr = w.clone().requires_grad_(True)
        loss = loss_of(forward(wr, torch.tensor(x, dtype=dtype)), torch.tensor(y, dtype=dtype), unbalanced)
        (g,) = torch.autograd.grad(loss, wr)
        m = BETA1 * m + (1 - BETA1) * g
        v = BETA2 * v + (1 - BETA2) * g * g
        w = w - torch.tensor(lr_t(t), dtype=dtype) * m / (torch.sqrt(v) + EPS)
        losses.append(float(loss.detach()))
    return np.array(losses)
