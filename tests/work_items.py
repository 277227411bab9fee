"""TEST INFRASTRUCTURE: the work items of a persistent classifier launch, and inputs that put chosen windows into chosen items.  Never imported
by the product.  Host-side only (tests/test_work_items_host.py checks it without a GPU); tests/test_gpu_work_items.py feeds it the launch
geometry the library REPORTS (DM_INFO_GRID_CAP, DM_INFO_LAST_GRID) - nothing here knows how the library sizes its grid.

What include/deepmod_hip.h documents about a launch of T = ceil(n / 128) tiles on g workgroups: workgroup b runs the items b, b + g, b + 2 g, ...
below 2 T, item w is tile w // 2 in direction w % 2 (0 forward, 1 backward).  The ROUND of an item is how many items its workgroup ran before
it (w // g).  With an even g a workgroup keeps one direction, with an odd g it alternates.

The windows come from one pool of K = 2,304 distinct ones, so that the CPU oracles cost K windows whatever the call's size
(hidden_probe.Reference.view): the 192 read-shaped windows of tests/golden/trained_like_tail_case.npz (HOT: means on the +-5 clip, events up to
26,984 samples) and 2,112 of synth.synthetic_windows (QUIET) - the two input sets hidden_probe.R was measured on."""
from __future__ import annotations

import os
from typing import Callable, Dict, Iterable, List, Tuple

import numpy as np

TILE = 128
N_HOT, N_QUIET = 192, 2112
K = N_HOT + N_QUIET
QUIET_BLOCKS = N_QUIET // TILE          # 16 tiles' worth of distinct quiet windows (the last 64 quiet windows belong to no block)
N_MIXED = K - 2                         # mixed_index draws from pool windows [0, N_MIXED): the last two are kept out of every mixed call
LONE, UNREAD = K - 2, K - 1             # ... for the range-flag case: a window placed exactly once, and one no call selects
WIN, NFEAT = 21, 7


def pool(golden_dir: str) -> np.ndarray:
    from deepmod_amd import synth
    hot = np.ascontiguousarray(np.load(os.path.join(golden_dir, "trained_like_tail_case.npz"))["X"], np.float32)
    assert hot.shape == (N_HOT, WIN, NFEAT), hot.shape
    x = np.concatenate([hot, synth.synthetic_windows(N_QUIET, seed=136)], axis=0)
    x.setflags(write=False)
    return x


def pool_rows(x: np.ndarray) -> np.ndarray:
    """The pool as ONE feature-row matrix [K * 21, 7]: block k (rows 21 k .. 21 k + 20) is window k, so the window centred on row 21 k + 10 is
    window k exactly and a centre list picks pool windows through the kernels' widx addressing."""
    return np.ascontiguousarray(x.reshape(-1, NFEAT))


def centres(index: np.ndarray) -> np.ndarray:
    return (WIN * np.asarray(index, np.int64) + WIN // 2).astype(np.int32)


# -- geometry ---------------------------------------------------------------------------------------------------------------------------
class Geometry:
    """T tiles on a grid of g workgroups under a cap (both as the library reported them)."""

    def __init__(self, ntiles: int, grid: int, cap: int):
        self.ntiles, self.grid, self.cap = int(ntiles), int(grid), int(cap)
        self.items = 2 * self.ntiles
        if not (self.ntiles >= 1 and 1 <= self.grid <= self.cap and self.grid <= self.items):
            raise AssertionError("PREMISE BROKEN: a launch of %d tiles reports %d workgroups under a cap of %d" % (self.ntiles, self.grid, self.cap))
        self.rounds = -(-self.items // self.grid)

    def group_items(self, b: int) -> np.ndarray:
        return np.arange(b, self.items, self.grid)

    def item_round(self) -> np.ndarray:
        """[2 T]: the round of every item."""
        return np.arange(self.items) // self.grid

    def tile_round(self) -> np.ndarray:
        """[T]: the round of a tile's FORWARD item.  The backward item is in the same round, except for at most one tile per round boundary of
        an odd grid, whose backward item opens the next round on workgroup 0."""
        return self.item_round()[0::2]

    def items_per_group(self) -> np.ndarray:
        return np.array([len(self.group_items(b)) for b in range(self.grid)])

    def patterns(self) -> Dict[str, int]:
        """direction pattern of a workgroup ('fbf': forward, backward, forward) -> how many workgroups run it."""
        out: Dict[str, int] = {}
        for b in range(self.grid):
            p = "".join("fb"[w & 1] for w in self.group_items(b))
            out[p] = out.get(p, 0) + 1
        return out

    def describe(self) -> str:
        return "%d tiles = %d items on %d workgroups (cap %d): %d rounds, patterns %s" % (
            self.ntiles, self.items, self.grid, self.cap, self.rounds, " ".join("%s x %d" % kv for kv in sorted(self.patterns().items())))


def require(geo: Geometry, rounds: int, parity: str, exact: bool = False) -> Geometry:
    """The premise of a case, asserted from the reported geometry: `rounds` rounds; parity 'even': every workgroup keeps ONE direction,
    'odd': every workgroup alternates, both starting directions occur; exact: every workgroup runs exactly `rounds` items, else every workgroup
    runs `rounds` or `rounds - 1` and at most `rounds - 1` of them the fewer (so the later items are the rule, not the exception).
    An AssertionError that says which premise the launch no longer meets - never a pass on a geometry that does not exercise the case."""
    what = "PREMISE BROKEN (the library's grid rule no longer gives this case its launch geometry; choose the tile count anew): " + geo.describe()
    if geo.rounds != rounds:
        raise AssertionError("%s - wanted %d rounds" % (what, rounds))
    if geo.grid % 2 != (0 if parity == "even" else 1):
        raise AssertionError("%s - wanted an %s grid" % (what, parity))
    per = geo.items_per_group()
    short = int((per < rounds).sum())
    if per.max() != rounds or per.min() < rounds - 1 or short > (0 if exact else rounds - 1):
        raise AssertionError("%s - wanted %s %d items per workgroup, %d workgroups run fewer (least %d)" % (what, "exactly" if exact else "nearly always", rounds, short, per.min()))
    pats = geo.patterns()
    full = {p for p in pats if len(p) == rounds}
    want = {"f" * rounds, "b" * rounds} if parity == "even" else {("fb" * rounds)[:rounds], ("bf" * rounds)[:rounds]}
    if full != want:
        raise AssertionError("%s - wanted the direction patterns %s" % (what, sorted(want)))
    return geo


def search(grid_of: Callable[[int], int], cap: int, rounds: int, parity: str, exact: bool = False) -> Geometry:
    """The fewest tiles T whose launch - grid_of(T): what the library reports for it - meets require(rounds, parity, exact).  The walk starts at
    the fewest tiles that cannot fit into rounds - 1 rounds of `cap` workgroups and ends where `rounds` rounds of them are full."""
    lo, hi = (rounds - 1) * cap // 2 + 1, rounds * cap // 2
    seen = []
    for t in range(lo, hi + 1):
        geo = Geometry(t, grid_of(t), cap)
        try:
            return require(geo, rounds, parity, exact)
        except AssertionError:
            seen.append("T=%d: g=%d, %d rounds" % (t, geo.grid, geo.rounds))
    raise AssertionError("PREMISE BROKEN: no tile count in [%d, %d] gives %d rounds on an %s grid%s under a cap of %d workgroups; the library reported %s"
                         % (lo, hi, rounds, parity, " filled exactly" if exact else "", cap, "; ".join(seen[:8]) + (" ..." if len(seen) > 8 else "")))


# -- index maps: window i of a call is pool window index[i] -----------------------------------------------------------------------------------
def mixed_index(n: int, offset: int = 7) -> np.ndarray:
    """Hot and quiet windows mixed within every tile: the pool windows [0, N_MIXED) walked with a stride coprime to N_MIXED (2,302 = 2 x 1,151),
    so each of them comes up every 2,302 windows, at another lane of another tile each time (2,302 is no multiple of 16)."""
    return ((np.arange(n, dtype=np.int64) * 935 + offset) % N_MIXED).astype(np.int64)


def quiet_block(q: int) -> np.ndarray:
    """The pool windows of quiet block q: one tile's worth."""
    assert 0 <= q < QUIET_BLOCKS
    return N_HOT + TILE * q + np.arange(TILE, dtype=np.int64)


def poisoned_index(geo: Geometry, hot_parity: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Full tiles; the tiles whose round has parity hot_parity hold hot windows only, the others quiet blocks (round robin).
    -> (index [128 T], hot [T] bool, block [T]: the quiet block of a quiet tile, -1 for a hot one)."""
    rnd = geo.tile_round()
    hot = (rnd % 2) == hot_parity
    block = np.full(geo.ntiles, -1, np.int64)
    index = np.empty(geo.ntiles * TILE, np.int64)
    q = 0
    for t in range(geo.ntiles):
        if hot[t]:
            index[t * TILE:(t + 1) * TILE] = (np.arange(TILE) + 37 * t) % N_HOT
        else:
            block[t] = q % QUIET_BLOCKS
            index[t * TILE:(t + 1) * TILE] = quiet_block(block[t])
            q += 1
    return index, hot, block


def poisoned_premise(geo: Geometry, hot: np.ndarray) -> Tuple[int, int]:
    """(later items whose workgroup ran a tile of the OTHER kind right before, later items whose predecessor was of the same kind).  The second
    number is 0 on an even grid and at most rounds - 1 on an odd one (Geometry.tile_round)."""
    w = np.arange(geo.grid, geo.items)
    other = hot[w // 2] != hot[(w - geo.grid) // 2]
    return int(other.sum()), int((~other).sum())


def require_poisoned(geo: Geometry, hot: np.ndarray) -> Tuple[int, int]:
    other, same = poisoned_premise(geo, hot)
    if not (other > 0 and same <= (0 if geo.grid % 2 == 0 else geo.rounds - 1) and hot.any() and not hot.all()):
        raise AssertionError("PREMISE BROKEN: %d later items follow a tile of the other kind, %d one of their own kind: %s" % (other, same, geo.describe()))
    return other, same


def pieces(ntiles: int, tiles_per_piece: int) -> List[Tuple[int, int]]:
    """[lo, hi) window ranges that cut a call at tile boundaries (the last piece keeps the call's ragged tile; the caller clips hi to n)."""
    assert tiles_per_piece >= 1
    return [(t * TILE, min(ntiles, t + tiles_per_piece) * TILE) for t in range(0, ntiles, tiles_per_piece)]


def last_round_windows(geo: Geometry, n: int) -> Iterable[int]:
    """Windows both of whose items are in the last round."""
    ir = geo.item_round()
    for t in range(geo.ntiles):
        if ir[2 * t] == geo.rounds - 1 and ir[2 * t + 1] == geo.rounds - 1:
            for i in range(t * TILE, min(n, (t + 1) * TILE)):
                yield i
