"""TEST INFRASTRUCTURE: the calls whose output bits tests/golden/edges_parent_bits.npz records (written by tests/golden/make_golden_edges.py on the
library of the commit BEFORE the classifier's edge work) and tests/test_gpu_edges.py holds every later library to.  Never imported by the product.

A case is a name and one call on a model: the same inputs, bit for bit, whoever runs it.  A window's output does not depend on the launch geometry
(tests/test_gpu_work_items.py), so the recorded bits hold on any number of CUs; the geometry premises of the two three-round cases are asserted by
the test from what the library reports, not recorded.

The three-round cases go through dm_predict_read_at on a row matrix of POOL distinct windows, walked with a stride coprime to POOL: 16,000 windows
per call whose outputs repeat with period POOL, which is what keeps the compressed fixture small."""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "edges_parent_bits.npz")

TILE, WIN, NFEAT = 128, 21, 7
PRECISIONS = ["f16x3", "f16i8"]
WEIGHTS = ["synthetic", "trained"]
SIZES = [1, 127, 128, 129, 385]          # one lane, a tile less one, a full tile, a tile and one, three tiles and one
POOL = 300
# under DM_OPT_RESERVED_CUS at its maximum on 256 CUs (cap 128): 129 tiles = 258 items -> 3 rounds on 86 workgroups (even: a workgroup keeps its
# direction), 130 tiles = 260 items -> 3 rounds on 87 (odd: a workgroup alternates, and the two items of a tile can lie in different rounds)
ROUNDS3 = {"rounds3_even": 129, "rounds3_odd": 130}
CASES = ["n%d" % n for n in SIZES] + sorted(ROUNDS3)

_CACHE = {}


def weights(name):
    from deepmod_amd import synth
    if name == "synthetic":
        return synth.synthetic_weights(26, 4.0)
    z = np.load(os.path.join(GOLDEN, "trained_like_weights.npz"))
    return {k.replace("|", "/"): np.ascontiguousarray(z[k], dtype=np.float32) for k in z.files}


def windows():
    from deepmod_amd import synth
    if "x" not in _CACHE:
        _CACHE["x"] = synth.synthetic_windows(max(SIZES), seed=77)
        _CACHE["x"].setflags(write=False)
    return _CACHE["x"]


def pool_rows():
    """POOL windows as one row matrix: block k (rows 21 k .. 21 k + 20) is window k."""
    from deepmod_amd import synth
    if "rows" not in _CACHE:
        _CACHE["rows"] = np.ascontiguousarray(synth.synthetic_windows(POOL, seed=78).reshape(-1, NFEAT))
        _CACHE["rows"].setflags(write=False)
    return _CACHE["rows"]


def centres(ntiles):
    n = TILE * (ntiles - 1) + 5           # a ragged last tile
    index = (np.arange(n, dtype=np.int64) * 7 + 3) % POOL
    return (WIN * index + WIN // 2).astype(np.int32)


def run(m, case):
    """-> (prob float32 [n, 2], cls uint8 [n], (grid cap, workgroups) of the call)."""
    from deepmod_amd import _lib
    if case in ROUNDS3:
        full_cap = m.get_info(_lib.DM_INFO_GRID_CAP)
        m.set_option(_lib.DM_OPT_RESERVED_CUS, full_cap // 2)
        try:
            prob, cls = m.predict_read_at(pool_rows(), centres(ROUNDS3[case]))
            geo = m.launch_geometry()
        finally:
            m.set_option(_lib.DM_OPT_RESERVED_CUS, 0)
        return prob, cls, geo
    n = int(case[1:])
    prob, cls = m.predict_windows(windows()[:n])
    return prob, cls, m.launch_geometry()


def key(wname, precision, case, what):
    return "%s|%s|%s|%s" % (wname, precision, case, what)


def bits(prob):
    return np.ascontiguousarray(prob, np.float32).view(np.uint32)
