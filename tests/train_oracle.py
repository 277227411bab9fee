"""Training oracle of the tests: torch-CPU autograd of the exact architecture (bin/DeepMod_scripts/myMultiBiRNN.py:21-91 of the reference: two
stacks of three BasicLSTMCell(100, forget_bias=1), gates i, j, f, o, forward stack over rows 0..10, backward stack over rows 20..10, head on
concat(h_fw[10], h_bw[10]), mean softmax cross entropy, class weights [0.1, 0.9] inside the loss's softmax when unbalanced) on the
canonical weight blob of deepmod_amd.model.flatten_weights.  float64 is the reference; the same code in float32 gives the error a correct
fp32 implementation has (the yardstick of tests/test_gpu_train.py).  Only tests import this module (torch is not a dependency of the package).

BLOCKS resolves the blob by row group, gate and unit group; `reference` holds the inputs and the float64 / float32 results of every gradient
case, computed once per process.

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


# ---------------------------------------------------------------------------------------------
# the gradient resolved by block: row group x gate x unit group
# ---------------------------------------------------------------------------------------------
GATES = ("i", "j", "f", "o")
UNIT_GROUPS = (("u0-95", 0, 96), ("u96-99", 96, HID))                 # units 96..99: the partial 16-unit tile of the 100 -> 112 padding
ROWS_L0 = (("onehot", 0, 4), ("mean", 4, 5), ("stdv", 5, 6), ("length", 6, 7), ("recurrent", NFEAT, NFEAT + HID))
ROWS_L12 = (("input", 0, HID), ("recurrent", HID, 2 * HID))


def block_table():
    """(name, tensor, index array into the blob) of the 195 blocks: kernels by row group x gate x unit group, biases by gate x unit group,
    out/W by direction, out/b whole."""
    out = []
    for name, a, b, shape in SLICES:
        idx = np.arange(a, b).reshape(shape)
        if name.endswith("kernel"):
            for rname, r0, r1 in (ROWS_L0 if shape[0] == NFEAT + HID else ROWS_L12):
                for gi, gate in enumerate(GATES):
                    for uname, u0, u1 in UNIT_GROUPS:
                        out.append(("%s[%s,%s,%s]" % (name, rname, gate, uname), name, idx[r0:r1, gi * HID + u0:gi * HID + u1].ravel()))
        elif name.endswith("bias"):
            for gi, gate in enumerate(GATES):
                for uname, u0, u1 in UNIT_GROUPS:
                    out.append(("%s[%s,%s]" % (name, gate, uname), name, idx[gi * HID + u0:gi * HID + u1]))
        elif name == "out/W":
            out.append(("out/W[fw]", name, idx[:HID].ravel()))
            out.append(("out/W[bw]", name, idx[HID:].ravel()))
        else:
            out.append((name, name, idx))
    return out


BLOCKS = block_table()


def block_errors(g, g64):
    """e(B) = max|g - g64| / max|g64| of the 195 blocks (inf where a block of g64 is all zero)."""
    d = np.abs(np.asarray(g, np.float64) - g64)
    a = np.abs(g64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {name: float(np.float64(d[idx].max()) / a[idx].max()) for name, _, idx in BLOCKS}


def float32_evaluations(flat, x, y, unbalanced):
    """The float32 oracle three times, in three summation orders over the batch: as given, reversed, and in two halves combined with weights
    n1 / n and n2 / n (at n = 1 the first again) -> [(loss, grad, prob in the order of x)] * 3."""
    f32 = torch.float32
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    n = len(x)
    given = loss_and_grad(flat, x, y, unbalanced, f32)
    if n == 1:
        return [given, given, given]
    lr, gr, pr = loss_and_grad(flat, x[::-1].copy(), y[::-1].copy(), unbalanced, f32)
    n1 = n // 2
    (l1, g1, p1), (l2, g2, p2) = (loss_and_grad(flat, x[s], y[s], unbalanced, f32) for s in (slice(0, n1), slice(n1, n)))
    w1, w2 = np.float32(n1) / np.float32(n), np.float32(n - n1) / np.float32(n)
    gh = (w1 * g1.astype(np.float32) + w2 * g2.astype(np.float32)).astype(np.float64)
    lh = float(w1 * np.float32(l1) + w2 * np.float32(l2))
    return [given, (lr, gr, pr[::-1]), (lh, gh, np.concatenate([p1, p2]))]


def block_yardstick(evals, g64):
    """e32*(B): the largest e32 of block B over the float32 evaluations - one evaluation's round-off can be luckily small."""
    errs = [block_errors(g, g64) for _, g, _ in evals]
    return {name: max(e[name] for e in errs) for name in errs[0]}


# ---------------------------------------------------------------------------------------------
# the gradient cases of tests/test_gpu_train.py: their inputs, and their references computed once per process
# ---------------------------------------------------------------------------------------------
GRAD_NS = (1, 15, 16, 17, 33, 129)      # row-tile edges; 11 n off a multiple of 4
SHRINK_NS = (129, 1, 17, 16, 129)       # one handle: a large batch, three smaller ones, the large size again
SESSION_SEED, SESSION_NS = 2, (40, 9)   # model.Session with max_batch 16: the first fetch grows the tape, the second is held to the oracle

SYNTH_CASES = [("synth", which, n, unb) for n in GRAD_NS for which in ("synthetic", "trained") for unb in (False, True)]
BIG_CASE = ("synth", "trained", 2049, True)
TAIL_CASES = [("tail", n) for n in (1, 17, 129)] + [("saturated", 33), ("oneclass", 1), ("oneclass", 0)]
SHRINK_CASES = [("shrink", i) for i in range(len(SHRINK_NS))]
SESSION_CASES = [("session", i) for i in range(len(SESSION_NS))]
ALL_CASES = SYNTH_CASES + [BIG_CASE] + TAIL_CASES + SHRINK_CASES + SESSION_CASES


def case_id(case):
    return "-".join(str(int(c)) if isinstance(c, bool) else str(c) for c in case)


def _tail_windows(n, seed):
    """n of the 192 read-shaped windows of tests/golden/trained_like_tail_case.npz (event lengths up to 26,984, means on the +-5 clip),
    drawn without replacement, with seeded random one-hot labels."""
    from conftest import GOLDEN
    import os
    X = np.load(os.path.join(GOLDEN, "trained_like_tail_case.npz"))["X"]
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(X[rng.permutation(len(X))[:n]], dtype=np.float32)
    return x, np.eye(2, dtype=np.float32)[rng.integers(0, 2, n)]


def case_inputs(case):
    """-> (weight blob, x, y, unbalanced) of a case."""
    from conftest import trained_like_weights
    from deepmod_amd import model, synth, train
    kind = case[0]
    if kind == "synth":                                   # the cases the suite had first: synth.synthetic_windows
        _, which, n, unbalanced = case
        flat = model.flatten_weights(synth.synthetic_weights(5, 1.0) if which == "synthetic" else trained_like_weights())
        x = synth.synthetic_windows(n, seed=1000 + n)
        lab = np.random.default_rng(1000 + n + 1).integers(0, 2, n)
        return flat, x, np.eye(2, dtype=np.float32)[lab], unbalanced
    if kind == "tail":
        x, y = _tail_windows(case[1], 4000 + case[1])
        return model.flatten_weights(trained_like_weights()), x, y, True
    if kind == "saturated":                               # weights of scale 4: layer-0 gates saturate on read-shaped inputs
        x, y = _tail_windows(case[1], 4100)
        return model.flatten_weights(synth.synthetic_weights(5, 4.0)), x, y, False
    if kind == "oneclass":                                # the training files are one class each: a batch can be too
        x, _ = _tail_windows(16, 4200 + case[1])
        return model.flatten_weights(trained_like_weights()), x, np.tile(np.eye(2, dtype=np.float32)[case[1]], (16, 1)), True
    if kind == "shrink":                                  # every call: other windows, other labels, unbalanced alternating
        i = case[1]
        x, y = _tail_windows(SHRINK_NS[i], 4300 + i)
        return model.flatten_weights(trained_like_weights()), x, y, bool(i & 1)
    if kind == "session":
        x, y = _tail_windows(SESSION_NS[case[1]], 4400 + case[1])
        return model.flatten_weights(train.initial_weights(SESSION_SEED)), x, y, False
    raise ValueError(case)


_references = {}


def reference(case):
    """The float64 result and the three float32 evaluations of a case, computed once per process and shared (read-only) by every test:
    flat, x, y, unbalanced, l64, g64, p64, l32, g32 (as float32), p32 (the float32 evaluation of the batch as given), e32_blocks (the yardstick:
    the largest of the three) and e32_prob = max|p32 - p64|."""
    if case not in _references:
        flat, x, y, unbalanced = case_inputs(case)
        l64, g64, p64 = loss_and_grad(flat, x, y, unbalanced, torch.float64)
        evals = float32_evaluations(flat, x, y, unbalanced)
        ref = dict(flat=flat, x=x, y=y, unbalanced=unbalanced, l64=l64, g64=g64, p64=p64, l32=evals[0][0], g32=evals[0][1].astype(np.float32),
                   p32=evals[0][2], e32_blocks=block_yardstick(evals, g64), e32_prob=float(np.abs(evals[0][2] - p64).max()))
        for a in (flat, x, y, g64, p64):
            a.setflags(write=False)
        _references[case] = ref
    return _references[case]
