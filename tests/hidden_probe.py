"""TEST INFRASTRUCTURE: probe heads that turn the classifier's two probabilities into an invertible read-out of the last layer's centre-step
output h (hcat[n, 200]: units 0..99 forward, 100..199 backward).  Never imported by the product.

The kernels fuse the head product, so h never reaches memory - but the head W[200][2], b[2] is an INPUT.  The suite's own heads (standard
normal, or the trained-like one) saturate the two-logit softmax on most windows: dp1/dz = p1 (1 - p1) is below 1e-3 there, and a hidden-state
error has to be thousands of fp32 ulps before 3e-5 in probability notices it.  With a head the test chooses the softmax stays in its linear
part on every window, and

    z = l1 - l0 = hcat . (W[:, 1] - W[:, 0])          (b = 0)

is recovered from the fp32 probabilities as log p1 - log p0 to a few 1e-7:

* dense, gain 1:  W = G / sqrt(200), G standard normal (seeded) - every unit of both directions weighs in, |z| stays below ~2;
* one-hot:        W[u, 1] = 2, zero elsewhere - p1 = sigmoid(2 h_u), h_u = z / 2: one unit of one direction, alone;
* fw_only / bw_only of a dense head: the other direction's rows zeroed - that direction's partial logit is exactly 0.

Three figures per case, over ALL windows (no class is compared, so nothing is exempted as a near tie):

    yard  = max |z_c32 - z_64|                  how far the fp32 C oracle itself is from the exact (float64) value of the graph
    floor = max |recover_z(prob_c32) - z_c32|   what the fp32 head product and the softmax read-out cost the reference itself
    err   = max |recover_z(prob_kernel) - z_64|

and the assertion of tests/test_gpu_hidden_parity.py is err <= R * yard + 2 * floor.

A call that repeats K distinct windows n times over (tests/test_gpu_work_items.py: enough tiles for every workgroup to run three or four work
items) is reported through Reference.view(index): the oracles cost K windows, and yard and floor are those of the windows the call uses.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional

import numpy as np

from oracle import oracle_np

HID = oracle_np.HID
HEAD_W, HEAD_B = oracle_np.HEAD_W, oracle_np.HEAD_B


# -- heads ------------------------------------------------------------------------------------------------------------------------------
def dense_head(seed: int) -> np.ndarray:
    """G / sqrt(200), G standard normal: z = hcat . (W1 - W0) has gain 1 (|h| < 1 and the weights' squares sum to 2)."""
    g = np.random.default_rng(seed).standard_normal((2 * HID, 2))
    return (g / np.sqrt(2.0 * HID)).astype(np.float32)


def one_hot_head(unit: int) -> np.ndarray:
    """p1 = sigmoid(2 h_unit); unit 0..99 forward, 100..199 backward.  (2 is exact in every operand format of the kernels.)"""
    w = np.zeros((2 * HID, 2), np.float32)
    w[unit, 1] = 2.0
    return w


def fw_only(head: np.ndarray) -> np.ndarray:
    out = np.array(head, np.float32, copy=True)
    out[HID:] = 0.0
    return out


def bw_only(head: np.ndarray) -> np.ndarray:
    out = np.array(head, np.float32, copy=True)
    out[:HID] = 0.0
    return out


def probe_weights(w: Dict[str, np.ndarray], head: np.ndarray) -> Dict[str, np.ndarray]:
    """A copy of the weights with HEAD_W replaced by `head` and HEAD_B = 0."""
    head = np.ascontiguousarray(head, np.float32)
    assert head.shape == (2 * HID, 2), head.shape
    out = {k: v for k, v in w.items()}
    out[HEAD_W] = head.copy()
    out[HEAD_B] = np.zeros(2, np.float32)
    return out


def head_vector(head: np.ndarray) -> np.ndarray:
    """W[:, 1] - W[:, 0] in float64 (exact: both are fp32)."""
    head = np.asarray(head, np.float32).astype(np.float64)
    return head[:, 1] - head[:, 0]


# -- read-out ---------------------------------------------------------------------------------------------------------------------------
def recover_z(prob: np.ndarray) -> np.ndarray:
    """l1 - l0 = log p1 - log p0, float64, from the fp32 probabilities."""
    p = np.asarray(prob, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.log(p[:, 1]) - np.log(p[:, 0])


def sensitivity(z: np.ndarray) -> np.ndarray:
    """p1 (1 - p1) at logit difference z."""
    p1 = 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))
    return p1 * (1.0 - p1)


# -- references -------------------------------------------------------------------------------------------------------------------------
_CHUNK = 1024


def hcat64(w: Dict[str, np.ndarray], x: np.ndarray, threads: Optional[int] = None) -> np.ndarray:
    """hcat of oracle_np.predict_windows_np(..., np.float64): the exact value of the graph on the fp32 weights and inputs.  Windows are
    independent, so the batch is evaluated in chunks on a few threads (numpy releases the GIL in its loops) - same values, less wall time."""
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[0]
    if n == 0:
        return np.zeros((0, 2 * HID), np.float64)
    chunks = [(i, min(n, i + _CHUNK)) for i in range(0, n, _CHUNK)]
    threads = threads or max(1, min(len(chunks), oracle_np.usable_cores()))
    run = lambda lohi: oracle_np.predict_windows_np(w, x[lohi[0]:lohi[1]], np.float64)[2]
    if threads == 1:
        parts = [run(c) for c in chunks]
    else:
        with ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(run, chunks))
    out = np.concatenate(parts, axis=0)
    assert out.dtype == np.float64 and out.shape == (n, 2 * HID)
    return out


class Reference:
    """The two references of one (weights, inputs) pair.  hcat does not depend on the head, so one Reference serves every probe head."""

    def __init__(self, w: Dict[str, np.ndarray], x: np.ndarray):
        self.w = w
        self.x = np.ascontiguousarray(x, np.float32)
        self.h64 = hcat64(w, self.x)
        self.h32f = oracle_np.predict_windows_c(w, self.x, want_hcat=True)[2]
        self.h32 = self.h32f.astype(np.float64)
        self._figures = {}                 # yard and floor per head: the same for every precision under test

    def z64(self, head: np.ndarray) -> np.ndarray:
        return self.h64 @ head_vector(head)

    def z32(self, head: np.ndarray) -> np.ndarray:
        return self.h32 @ head_vector(head)

    def prob_c32(self, head: np.ndarray) -> np.ndarray:
        """The C oracle's probabilities under the probe head, from its own hcat (c_head_prob): the C oracle is not run again for every head."""
        return c_head_prob(self.h32f, head)

    def _cached(self, what: str, head: np.ndarray, compute):
        key = (what, np.ascontiguousarray(head, np.float32).tobytes())
        if key not in self._figures:
            self._figures[key] = compute()
        return self._figures[key]

    def yards(self, head: np.ndarray) -> np.ndarray:
        """|z_c32 - z_64| per window."""
        return self._cached("yards", head, lambda: np.abs(self.z32(head) - self.z64(head)))

    def floors(self, head: np.ndarray) -> np.ndarray:
        """|recover_z(prob_c32) - z_c32| per window."""
        return self._cached("floors", head, lambda: np.abs(recover_z(self.prob_c32(head)) - self.z32(head)))

    def yard(self, head: np.ndarray) -> float:
        return self._cached("yard", head, lambda: float(self.yards(head).max()))

    def floor(self, head: np.ndarray) -> float:
        return self._cached("floor", head, lambda: float(self.floors(head).max()))

    def err(self, prob: np.ndarray, head: np.ndarray) -> np.ndarray:
        """|recover_z(prob) - z_64| per window."""
        return np.abs(recover_z(prob) - self.z64(head))

    def view(self, index: np.ndarray) -> "IndexedReference":
        return IndexedReference(self, index)


class IndexedReference:
    """A Reference over K distinct windows seen through an index map [n] -> [0, K): what report() needs for a kernel call whose window i is
    window index[i] of the Reference.  A window's arithmetic does not depend on where in a call it sits, so a call of n windows that repeats
    K distinct ones costs the CPU oracles K windows; yard and floor are taken over the distinct windows the call USES, so windows of the
    Reference that the call leaves out lend it no allowance.  view(arange(K)) reports what the Reference itself reports."""

    def __init__(self, ref: Reference, index: np.ndarray):
        index = np.ascontiguousarray(index, np.int64)
        k = ref.x.shape[0]
        assert index.ndim == 1 and index.size > 0 and int(index.min()) >= 0 and int(index.max()) < k, (index.shape, k)
        self.ref, self.index, self.used = ref, index, np.unique(index)
        self.w = ref.w

    @property
    def x(self) -> np.ndarray:
        """The call's windows, materialised: float32 [n, 21, 7]."""
        return np.ascontiguousarray(self.ref.x[self.index])

    def z64(self, head: np.ndarray) -> np.ndarray:
        return self.ref.z64(head)[self.index]

    def z32(self, head: np.ndarray) -> np.ndarray:
        return self.ref.z32(head)[self.index]

    def prob_c32(self, head: np.ndarray) -> np.ndarray:
        return self.ref.prob_c32(head)[self.index]

    def yard(self, head: np.ndarray) -> float:
        return float(self.ref.yards(head)[self.used].max())

    def floor(self, head: np.ndarray) -> float:
        return float(self.ref.floors(head)[self.used].max())

    def err(self, prob: np.ndarray, head: np.ndarray) -> np.ndarray:
        prob = np.asarray(prob)
        assert prob.shape == (self.index.size, 2), (prob.shape, self.index.size)
        return np.abs(recover_z(prob) - self.z64(head))


def reference_z(w: Dict[str, np.ndarray], x: np.ndarray, head: np.ndarray):
    """(z_64, z_c32): hcat of the float64 numpy oracle and of the fp32 C oracle, each turned into z in float64."""
    ref = Reference(w, x)
    return ref.z64(head), ref.z32(head)


def report(ref, prob: np.ndarray, head: np.ndarray) -> Dict[str, float]:
    """yard, floor and err of one case; ratio = (err - 2 floor) / yard is what the allowance R is measured as.  ref: a Reference, or an
    IndexedReference (Reference.view(index)) for a kernel output of n windows that are windows index[0..n) of the Reference."""
    yard, floor = ref.yard(head), ref.floor(head)
    e = ref.err(prob, head)
    worst = int(np.argmax(e)) if len(e) else -1
    err = float(e.max()) if len(e) else 0.0
    return {"yard": yard, "floor": floor, "err": err, "worst": worst, "ratio": (err - 2.0 * floor) / yard if yard > 0 else float("inf")}


def head_prob_np(hcat: np.ndarray, head: np.ndarray) -> np.ndarray:
    """The head and softmax lines of oracle_np.predict_windows_np in fp32 on a given fp32 hcat (b = 0): the probabilities the fp32 numpy oracle
    gives under probe_weights(w, head), without evaluating the six cells again for every head (tests/test_hidden_probe.py pins the identity)."""
    F = np.float32
    logits = (np.asarray(hcat, F) @ np.asarray(head, F)).astype(F) + np.zeros(2, F)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F)


def c_head_prob(hcat: np.ndarray, head: np.ndarray) -> np.ndarray:
    """The head lines of oracle/deepmod_oracle.c restated on a given fp32 hcat (b = 0): the two logits summed serially in fp32 over fw units 0..99,
    then bw units 0..99, every product and sum rounded (the C oracle is built with contraction off), then its two-exponential softmax.  hcat does
    not depend on the head, and a C-oracle pass over 20,000 windows costs seconds: this gives that pass's probabilities for any head from ONE run
    (tests/test_hidden_probe.py: the same logits, p the same to one fp32 ulp - libm's expf is not always correctly rounded)."""
    F = np.float32
    h = np.ascontiguousarray(hcat, F)
    wout = np.ascontiguousarray(head, F)
    lg0, lg1 = np.zeros(len(h), F), np.zeros(len(h), F)
    for u in range(2 * HID):
        lg0 = lg0 + h[:, u] * wout[u, 0]
        lg1 = lg1 + h[:, u] * wout[u, 1]
    assert lg0.dtype == F and lg1.dtype == F
    m = np.maximum(lg0, lg1)
    d0, d1 = lg0 - m, lg1 - m
    e0, e1 = np.exp(d0.astype(np.float64)).astype(F), np.exp(d1.astype(np.float64)).astype(F)
    return np.stack([e0 / (e0 + e1), e1 / (e0 + e1)], axis=1).astype(F)


# -- the allowance ------------------------------------------------------------------------------------------------------------------------
# err <= R * yard + 2 * floor.  R is MEASURED against the reference, not chosen: the worst (err - 2 floor) / yard of each kernel on an MI355X, x 1.5
# (the maximum of this error over 20,000 windows moves by tens of percent between seeds), rounded up to one significant digit.
#
# "dense": the dense-probe cases of tests/test_gpu_hidden_parity.py (trained-like, seed 17 x 4, seed 21 x 1) and three more weight seeds at scale 4
# (21, 22, 26), 4 head seeds each, 20,000 synthetic windows + the read-shaped tail inputs + a ragged 129-window call.  Measured 2026-10-17:
#     fp32 kernel 0.53 (seed 17 x 4; trained-like -0.24: err below 2 floor), split-f16 0.54 (seed 17 x 4; trained-like -0.05),
#     int8 cross terms 38.2 (seed 21 x 4; trained-like 25.2, seed 21 x 1 11.7).
# "unit": the one-hot pass, all 200 units x (trained-like, seed 17 x 4), 2,048 windows per unit.  Measured 2026-10-17:
#     fp32 kernel 2.67 (seed 17 x 4, bw unit 88; trained-like 1.05, bw unit 71), split-f16 1.93 (seed 17 x 4, fw unit 47; trained-like 0.98, bw unit 71),
#     int8 46.9 (seed 17 x 4, bw unit 97; trained-like 40.7, fw unit 19).
#   A unit's yard is the maximum of ONE unit's fp32 round-off over 2,048 windows - a single draw with a heavy tail, where the dense yard pools 200 units
#   over 20,000 windows - so two CORRECT fp32 evaluations spread wider against each other per unit: the numpy fp32 oracle against the C oracle, same
#   windows, per-unit max |dh| ratios up to 2.1 one way and 2.8 the other at seed 17 x 4 (1.9 / 1.8 trained-like), 0.8 .. 1.15 under the dense heads.
#   The worst units of the fp32-class kernels (88, 71, 47, 16, 73, 40 over the eight passes) follow no direction, tile or lane group, and none is in the
#   mixed k-step 96..99: their ratios are of the size two correct fp32 evaluations show against each other.
# Both fp32-class kernels stay below 4, the figure above which a ratio is a finding to locate and fix rather than a number to write down; the
# opt-in int8 mode keeps its documented reduced precision (its operands carry 19 bits, not 22) and its own allowance.
R_MEASURED = {"dense": {"f32": 0.53, "f16x3": 0.54, "f16i8": 38.2}, "unit": {"f32": 2.67, "f16x3": 1.93, "f16i8": 46.9}}
R = {"dense": {"f32": 0.8, "f16x3": 0.9, "f16i8": 60.0}, "unit": {"f32": 4.0, "f16x3": 3.0, "f16i8": 80.0}}


def allowance(precision: str, yard: float, floor: float, probe: str = "dense") -> float:
    return R[probe][precision] * yard + 2.0 * floor


# -- damaged weights: stand-ins for a subtly wrong kernel ---------------------------------------------------------------------------------
def round_to_f16(w: Dict[str, np.ndarray], direction: str, layer: int, rows=slice(None), cols=slice(None)) -> Dict[str, np.ndarray]:
    """A copy of the weights with part of one cell's kernel rounded to f16: what a split-f16 kernel computes when it drops the `lo` half."""
    name = oracle_np.cell_name(direction, layer, "kernel")
    out = {k: v for k, v in w.items()}
    k = np.array(w[name], np.float32, copy=True)
    k[rows, cols] = k[rows, cols].astype(np.float16).astype(np.float32)
    out[name] = k
    return out
