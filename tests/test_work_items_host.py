"""CPU: the host side of tests/test_gpu_work_items.py - the indexed view of hidden_probe.Reference and the case builders of tests/work_items.py.

The GPU module takes a launch's geometry from what the library reports.  Here a stand-in plays the library: PRESENT_RULE restates how
launch_bilstm sizes its grid today (deepmod_amd/csrc/deepmod_hip.hip), for the grid caps of a 208-, 256-, 304- and 512-CU device with half the
CUs reserved.  It is the stand-in of THIS module only: the GPU tests do not contain it, and a library that sizes its grid otherwise fails their
premises (shown below with the rule from before the grid was sized to whole rounds) instead of passing on a launch that no longer exercises the
case."""
import numpy as np
import pytest

import hidden_probe as hp
import work_items as wi
from conftest import GOLDEN
from deepmod_amd import synth

CAPS = (104, 128, 152, 256)


def PRESENT_RULE(cap):
    def grid_of(ntiles):
        items = 2 * ntiles
        if items <= cap:
            return items
        rounds = -(-items // cap)
        return -(-items // rounds)
    return grid_of


def EARLIER_RULE(cap):
    return lambda ntiles: min(2 * ntiles, cap)


def test_indexed_view_equals_the_materialised_reference():
    """A Reference over K windows seen through an index map reports what a Reference over the n materialised windows reports: z, yard, floor and
    err - and its yard and floor are those of the windows the map uses, not of the whole Reference."""
    w = synth.synthetic_weights(21, 1.0)
    x = synth.synthetic_windows(48, seed=9)
    x[40:] *= 3.0                                               # windows the map leaves out, with another yard
    index = np.array([5, 0, 17, 5, 5, 31, 0, 39, 2, 17] * 3 + [11], np.int64)
    assert index.max() < 40
    ref, mat = hp.Reference(w, x), hp.Reference(w, x[index])
    view = ref.view(index)
    assert np.array_equal(view.x, mat.x) and np.array_equal(view.used, np.unique(index)) and np.array_equal(ref.h32f[index], mat.h32f)
    rng = np.random.default_rng(3)
    for head in (hp.dense_head(1), hp.fw_only(hp.dense_head(2)), hp.bw_only(hp.dense_head(2)), hp.one_hot_head(150)):
        # the C oracle evaluates window by window: the same bits.  The float64 oracle and the float64 products hcat . head run a window in a batch
        # of another size: the same value up to the last bits of float64 (1e-13 at |z| <= 2), a ten-millionth of yard
        assert np.array_equal(view.prob_c32(head), mat.prob_c32(head))
        assert np.abs(view.z64(head) - mat.z64(head)).max() <= 1e-13 and np.abs(view.z32(head) - mat.z32(head)).max() <= 1e-13
        assert abs(view.floor(head) - mat.floor(head)) <= 1e-13 and abs(view.yard(head) - mat.yard(head)) <= 1e-13 and view.yard(head) > 1e-8
        prob = mat.prob_c32(head).copy()
        prob[7] = hp.head_prob_np((ref.h32f[index[7]] + rng.standard_normal(2 * hp.HID).astype(np.float32) * 1e-3)[None], head)[0]
        a, b = hp.report(view, prob, head), hp.report(mat, prob, head)
        assert a["worst"] == b["worst"] == 7 and abs(a["err"] - b["err"]) <= 1e-13 and abs(a["ratio"] - b["ratio"]) <= 1e-6 * abs(b["ratio"])
    head = hp.dense_head(1)
    everything = ref.view(np.arange(len(x)))
    assert everything.yard(head) == ref.yard(head) and everything.floor(head) == ref.floor(head)
    assert ref.view(np.arange(40, 48)).yard(head) != ref.view(np.arange(40)).yard(head)
    for bad in ([48], [-1], []):
        with pytest.raises(AssertionError):
            ref.view(np.array(bad, np.int64))
    with pytest.raises(AssertionError):
        view.err(np.zeros((len(index) + 1, 2), np.float32), head)     # a kernel output of another length than the map


def test_pool_and_index_maps():
    x = wi.pool(GOLDEN)
    assert x.shape == (wi.K, 21, 7) and wi.K <= 2304 and x.dtype == np.float32
    assert np.abs(x[:wi.N_HOT, :, 4]).max() == 5.0 and x[:wi.N_HOT, :, 6].max() > 20000        # hot: means on the clip, long events
    rows, idx = wi.pool_rows(x), wi.mixed_index(16400)
    c = wi.centres(idx)
    assert rows.shape == (wi.K * 21, 7) and c.dtype == np.int32 and c.min() >= 10 and c.max() < len(rows) - 10
    for i in (0, 1, 8000, 16399):
        assert np.array_equal(rows[c[i] - 10:c[i] + 11], x[idx[i]])
    # every mixed window comes up, hot and quiet within one tile, the two kept-out windows never; a repeat sits at another lane
    assert np.array_equal(np.unique(idx), np.arange(wi.N_MIXED)) and wi.LONE not in idx and wi.UNREAD not in idx
    assert all(((idx[t * 128:(t + 1) * 128] < wi.N_HOT).any() and (idx[t * 128:(t + 1) * 128] >= wi.N_HOT).any()) for t in range(0, 128, 9))
    first, second = np.flatnonzero(idx == idx[0])[:2]
    assert (second - first) % 16 != 0
    assert np.array_equal(np.concatenate([wi.quiet_block(q) for q in range(wi.QUIET_BLOCKS)]), np.arange(wi.N_HOT, wi.N_HOT + 128 * wi.QUIET_BLOCKS))
    assert wi.pieces(5, 2) == [(0, 256), (256, 512), (512, 640)] and wi.pieces(2, 2) == [(0, 256)]


@pytest.mark.parametrize("cap", CAPS)
def test_case_builders_give_every_workgroup_its_items(cap):
    """For each cap: the searches land on launches in which every workgroup runs the intended number of items in the intended directions, the
    ragged tile is met in the last round, and the poisoned-predecessor maps put a tile of the other kind before every later item."""
    grid_of = PRESENT_RULE(cap)
    found = {}
    for rounds in (3, 4):
        for parity in ("odd", "even"):
            geo = wi.search(grid_of, cap, rounds, parity, exact=parity == "even")
            found[rounds, parity] = (geo.ntiles, geo.grid)
            per, pats = geo.items_per_group(), geo.patterns()
            assert geo.rounds == rounds and geo.grid <= cap and geo.grid % 2 == (parity == "odd")
            if parity == "even":
                assert (per == rounds).all() and set(pats) == {"f" * rounds, "b" * rounds} and pats["f" * rounds] == pats["b" * rounds] == geo.grid // 2
            else:
                assert per.max() == rounds and (per < rounds).sum() <= rounds - 1 and per.min() == rounds - 1
                alternating = {("fb" * rounds)[:rounds], ("bf" * rounds)[:rounds]}
                assert alternating <= set(pats) and all(p in alternating or p in {a[:-1] for a in alternating} for p in pats)
            # the ragged tile (n = 128 (T - 1) + 16) is the last tile: both of its items are in the last round, as later items of their workgroups
            n = 128 * (geo.ntiles - 1) + 16
            last = set(wi.last_round_windows(geo, n))
            assert set(range(128 * (geo.ntiles - 1), n)) <= last and len(last) > 16 and min(last) >= 128 * (rounds - 1) * (geo.grid // 2)
            # poisoned predecessor, both ways round
            for hot_parity in (0, 1):
                index, hot, block = wi.poisoned_index(geo, hot_parity)
                other, same = wi.require_poisoned(geo, hot)
                assert other + same == geo.items - geo.grid and same <= (0 if parity == "even" else rounds - 1)
                assert index.shape == (128 * geo.ntiles,) and hot.sum() + (block >= 0).sum() == geo.ntiles
                tr = geo.tile_round()
                for t in range(geo.ntiles):
                    tile = index[128 * t:128 * (t + 1)]
                    assert hot[t] == (tr[t] % 2 == hot_parity)
                    assert (tile < wi.N_HOT).all() if hot[t] else np.array_equal(tile, wi.quiet_block(block[t]))
                assert len(set(block[block >= 0])) == min(wi.QUIET_BLOCKS, int((~hot).sum()))
    print("cap %d: (rounds, grid parity) -> (tiles, workgroups): %s" % (cap, found))
    if cap == 128:          # half of 256 CUs reserved: the launches the GPU module's docstring names
        assert found == {(3, "odd"): (130, 87), (3, "even"): (129, 86), (4, "odd"): (193, 97), (4, "even"): (196, 98)}
        assert wi.require(wi.Geometry(157, grid_of(157), cap), 3, "odd").grid == 105          # the 20,000 windows of test_gpu_hidden_parity.py


def test_a_broken_premise_fails_with_a_message():
    """A geometry that does not exercise a case is refused by name - with the grid rule from before launches were sized to whole rounds
    (min(items, cap) workgroups) no even three-round launch fills its workgroups exactly below 192 tiles, and 129 tiles give 128 workgroups of two
    or three items."""
    cap = 128
    with pytest.raises(AssertionError, match="PREMISE BROKEN.*wanted exactly 3 items"):
        wi.require(wi.Geometry(129, EARLIER_RULE(cap)(129), cap), 3, "even", exact=True)
    with pytest.raises(AssertionError, match="PREMISE BROKEN.*wanted an odd grid"):
        wi.require(wi.Geometry(157, EARLIER_RULE(cap)(157), cap), 3, "odd")
    with pytest.raises(AssertionError, match="PREMISE BROKEN: no tile count"):
        wi.search(EARLIER_RULE(cap), cap, 3, "odd")
    with pytest.raises(AssertionError, match="PREMISE BROKEN.*wanted 3 rounds"):
        wi.require(wi.Geometry(157, PRESENT_RULE(256)(157), 256), 3, "odd")             # nothing reserved: two rounds
    with pytest.raises(AssertionError, match="PREMISE BROKEN.*reports 300 workgroups"):
        wi.Geometry(157, 300, 128)
    geo = wi.Geometry(129, 86, cap)
    with pytest.raises(AssertionError, match="PREMISE BROKEN.*later items"):
        wi.require_poisoned(geo, np.ones(129, bool))                                    # nothing quiet
    with pytest.raises(AssertionError, match="PREMISE BROKEN.*later items"):
        wi.require_poisoned(geo, (np.arange(129) // 2) % 2 == 0)                        # kinds that ignore the rounds
