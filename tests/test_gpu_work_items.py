"""GPU (-m gpu): the classifier kernels held to the float64 oracle in hidden-state space ACROSS A WORKGROUP'S WORK ITEMS.

The kernels are persistent: a workgroup walks its (tile, direction) items and must re-establish everything at the top of each - h = 0, c = 0, the
accumulators, the weight-ring slot, the layer-0 cell rows in LDS, the fp32 kernel's h sequences.  tests/test_gpu_hidden_parity.py holds calls in
which a workgroup runs at most two items (once forward, once backward, the ragged tile never a later item).  Here every workgroup runs three or
four, with DM_OPT_RESERVED_CUS at its maximum so that the shapes stay small:

* three rounds on an odd grid (a workgroup alternates fw / bw / fw or bw / fw / bw) and on an even one (the same direction three times, the ragged
  tile met in the last round; once through materialised windows, once through dm_predict_read_at on a row matrix, so that the centre-row
  addressing is exercised in later items), four rounds on an odd and an even grid;
* poisoned predecessor: the tiles of rounds 0 and 2 hold read-shaped windows on the +-5 clip, those of round 1 quiet synthetic ones - and the other
  way round; every window is held to the oracle, and the quiet ones are bit-identical to the same windows in a call of one item per workgroup;
* any round, any grid: every case gives the same bits under the reserved grid, under the full grid, and cut at tile boundaries into calls of one
  round;
* a range violation (DM_ERANGE) raised from an item of the last round, once from the ragged tile.

The launch geometry is what the library REPORTS (DM_INFO_GRID_CAP, DM_INFO_LAST_GRID); the tile counts are searched against it
(tests/work_items.py) and every case asserts its premise - rounds, items per workgroup, direction patterns - from the geometry of its own call: a
grid rule that no longer gives a case its launch fails it with "PREMISE BROKEN".  With 256 CUs, 128 of them reserved, the searches land on
129 tiles / 86 workgroups and 130 / 87 (three rounds), 196 / 98 and 193 / 97 (four); the 20,000 windows of test_gpu_hidden_parity.py run on 105.

No tolerance is new: err <= hidden_probe.allowance(precision, yard, floor), yard and floor over the distinct windows a call uses (the CPU oracles
cost the pool's 2,304 windows per weight set, hidden_probe.Reference.view).  A window's arithmetic does not depend on its item, so a case beyond
the allowance is a finding.  Measured 2026-10-19 on one MI355X (162 [hidden] lines, all inside; the worst ratio = (err - 2 floor) / yard per mode):

    f32   (17, 4.0) three rounds, even grid, ragged tile last, windows, fw only of dense 2: yard 1.07e-06 floor 3.33e-07 err 1.23e-06 ratio 0.53 (bound 1.52e-06)
    f16x3 (17, 4.0) three rounds, even grid, ragged tile last, windows, bw only of dense 2: yard 1.2e-06 floor 5.17e-07 err 1.64e-06 ratio 0.51 (bound 2.11e-06)
    f16i8 (17, 4.0) 20,000 windows, three rounds, odd grid, fw only of dense 2: yard 1.38e-06 floor 3.88e-07 err 3.41e-05 ratio 24.14 (bound 8.36e-05)

against hidden_probe.R = 0.8 / 0.9 / 60.  Teeth (checked once, on a library that is not part of the repository): with the zeroing of c1reg / c2reg
and of the layer-0 cell rows skipped after a workgroup's first item (f16x3, f16i8), and with the head accumulators lacc not zeroed again (f32), every
oracle-held test here fails in all three modes, at ratios of 10^6, from the first window of round 1 (even grids) or round 2 (odd grids, fp32) on.
test_gpu_hidden_parity.py sees the f16 defect in its 24 dense-probe tests (a workgroup's second item) and the fp32 one nowhere."""
import numpy as np
import pytest

import hidden_probe as hp
import work_items as wi
from conftest import GOLDEN
from deepmod_amd import _lib, model
from test_gpu_hidden_parity import reference as cached_reference, weights

pytestmark = pytest.mark.gpu

WEIGHTS = ["trained", (17, 4.0)]
HEADS = [("dense 1", hp.dense_head(1)), ("fw only of dense 2", hp.fw_only(hp.dense_head(2))), ("bw only of dense 2", hp.bw_only(hp.dense_head(2)))]

_POOL, _SEARCHED = {}, {}


def pool():
    if "x" not in _POOL:
        _POOL["x"] = wi.pool(GOLDEN)
        _POOL["rows"] = wi.pool_rows(_POOL["x"])
    return _POOL["x"]


def pool_reference(wname):
    """One Reference over the pool per weight set, shared by every case, head and precision."""
    return cached_reference(wname, "work item pool", pool())


class Call:
    """n windows and what the oracle says about them.  form 'windows': materialised [n, 21, 7]; 'read_at': centre rows into the pool's row matrix."""

    def __init__(self, ref, form="windows", index=None, rows=None):
        self.ref, self.form, self.index = ref, form, index
        if form == "windows":
            self.x = ref.x
            self.n = len(self.x)
        else:
            self.rows = _POOL["rows"] if rows is None else rows
            self.centres = wi.centres(index)
            self.n = len(self.centres)
        self.ntiles = -(-self.n // wi.TILE)


class Probe:
    """A model under a probe head, its reserved CUs, and the geometry of every call as the library reports it."""

    def __init__(self, w, head, precision, device):
        self.m = model.BiLSTMModel(hp.probe_weights(w, head), device=device, precision=precision)
        self.full_cap, before = self.m.launch_geometry()         # nothing reserved yet: the device's CUs
        assert before == 0 and self.full_cap >= 4, (self.full_cap, before)
        self.cap = self.full_cap

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.m.close()

    def reserve(self, most):
        """DM_OPT_RESERVED_CUS at its maximum (half the CUs), or 0."""
        reserved = self.full_cap // 2 if most else 0
        self.m.set_option(_lib.DM_OPT_RESERVED_CUS, reserved)
        self.cap = self.m.get_info(_lib.DM_INFO_GRID_CAP)
        assert self.cap == self.full_cap - reserved, (self.cap, self.full_cap, reserved)
        return self.cap

    def run(self, call, lo=0, hi=None):
        hi = call.n if hi is None else hi
        if call.form == "windows":
            prob = self.m.predict_windows(call.x[lo:hi])[0]
        else:
            prob = self.m.predict_read_at(call.rows, call.centres[lo:hi])[0]
        cap, grid = self.m.launch_geometry()
        assert cap == self.cap
        return prob, wi.Geometry(-(-(hi - lo) // wi.TILE), grid, cap)


@pytest.fixture(scope="module", params=["f32", "f16x3", "f16i8"])
def kernel(gpu_device, hip_lib, request):
    """Every test runs for every precision mode of the library, as in test_gpu_hidden_parity.py; a probe head is a model of its own."""
    def probe(w, head):
        return Probe(w, head, request.param, gpu_device)
    probe.precision = request.param
    probe.device = gpu_device
    return probe


def searched(device, rounds, parity, exact=False):
    """wi.search against what the library reports for launches of T tiles under the reserved grid (one cheap call per T: all-zero rows, the grid
    depends on the window count alone).  Searched once; every case then asserts the premise again from its own call."""
    if "probe" not in _SEARCHED:
        pool()
        _SEARCHED["probe"] = p = Probe(weights("trained"), hp.dense_head(1), "f16x3", device)
        p.reserve(True)
    p = _SEARCHED["probe"]
    key = (p.cap, rounds, parity, exact)
    if key not in _SEARCHED:
        zero_rows = np.zeros((wi.WIN, wi.NFEAT), np.float32)

        def grid_of(ntiles):
            p.m.predict_read_at(zero_rows, np.full(wi.TILE * (ntiles - 1) + 1, wi.WIN // 2, np.int32))
            return p.m.launch_geometry()[1]
        _SEARCHED[key] = wi.search(grid_of, p.cap, rounds, parity, exact)
    return _SEARCHED[key]


_PRINTED = set()


def _once(line):
    """A case's geometry is the same under every head: printed once."""
    if line not in _PRINTED:
        _PRINTED.add(line)
        print(line)


def test_launch_geometry_is_reported(kernel):
    """DM_INFO_GRID_CAP follows DM_OPT_RESERVED_CUS, DM_INFO_LAST_GRID every classifier launch of every kernel; reading them changes nothing."""
    with kernel(weights("trained"), hp.dense_head(1)) as p:
        assert p.m.launch_geometry() == (p.full_cap, 0)
        prob, geo = p.run(Call(pool_reference("trained").view(np.arange(300))))      # three tiles: six items, one per workgroup
        assert (geo.cap, geo.grid, geo.rounds) == (p.full_cap, 6, 1)
        assert p.reserve(True) == p.full_cap - p.full_cap // 2 and p.m.launch_geometry() == (p.cap, 6)          # the last launch is still that one
        with pytest.raises(_lib.DeepModHipError):
            p.m.set_option(_lib.DM_OPT_RESERVED_CUS, p.full_cap // 2 + 1)
        assert p.m.launch_geometry() == (p.cap, 6)
        again, geo = p.run(Call(pool_reference("trained").view(np.arange(129))))
        assert (geo.cap, geo.grid) == (p.cap, 4) and not _same_bits(again, prob[:129]).size
        _, geo = p.run(Call(None, "read_at", np.arange(5)))
        assert geo.grid == 2
        assert p.reserve(False) == p.full_cap


def _same_bits(a, b):
    return np.flatnonzero((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any(axis=1))


def _held_at_any_grid(kernel, wname, call, premise, what, extra=None):
    """One case under every head: the reserved-grid call, its premise asserted from the reported geometry; the same bits under the full grid and
    cut into single-round pieces; every window within the allowance of the float64 oracle.  All findings are collected before the assertion."""
    w, failed = weights(wname), []
    for hname, head in HEADS:
        with kernel(w, head) as p:
            p.reserve(True)
            prob, geo = p.run(call)
            assert geo.ntiles == call.ntiles
            premise(geo)
            _once("[items]  %-5s %s %s: n = %d, %s" % (kernel.precision, wname, what, call.n, geo.describe()))
            p.reserve(False)
            prob_full, geo_full = p.run(call)
            assert geo_full.cap == p.full_cap and geo_full.grid != geo.grid, (geo_full.describe(), geo.describe())
            d = _same_bits(prob, prob_full)
            if d.size:
                failed.append("%s: %d windows differ between %d and %d workgroups, first at %d (tile %d)" % (hname, d.size, geo.grid, geo_full.grid, d[0], d[0] // wi.TILE))
            parts = []
            for lo, hi in wi.pieces(call.ntiles, max(1, p.full_cap // 2)):
                pp, g = p.run(call, lo, min(hi, call.n))
                if not (g.rounds == 1 and g.grid == g.items):
                    raise AssertionError("PREMISE BROKEN: a piece meant to run one item per workgroup: " + g.describe())
                parts.append(pp)
            d = _same_bits(prob, np.concatenate(parts, axis=0))
            if d.size:
                item_rounds = geo.item_round()
                failed.append("%s: %d windows differ from the single-round pieces, first at %d (tile %d, rounds of its items %d / %d)" %
                              (hname, d.size, d[0], d[0] // wi.TILE, item_rounds[2 * (d[0] // wi.TILE)], item_rounds[2 * (d[0] // wi.TILE) + 1]))
            r = hp.report(call.ref, prob, head)
            bound = hp.allowance(kernel.precision, r["yard"], r["floor"])
            print("[hidden] %-5s %s %s, %s: yard %.3g floor %.3g err %.3g ratio %.2f (bound %.3g)" %
                  (kernel.precision, wname, what, hname, r["yard"], r["floor"], r["err"], r["ratio"], bound))
            if not r["err"] <= bound:
                failed.append("%s: err %.3g > %.3g (yard %.3g, floor %.3g, ratio %.2f) at window %d (tile %d)" %
                              (hname, r["err"], bound, r["yard"], r["floor"], r["ratio"], r["worst"], r["worst"] // wi.TILE))
            if extra is not None:
                failed += ["%s: %s" % (hname, f) for f in extra(p, head, prob, geo)]
    assert not failed, "%s %s %s:\n%s" % (kernel.precision, wname, what, "\n".join(failed))


@pytest.mark.parametrize("wname", WEIGHTS, ids=str)
def test_three_rounds_on_an_odd_grid(wname, kernel):
    """The 20,000 synthetic windows of test_gpu_hidden_parity.py and their Reference, under the reserved grid: a workgroup alternates fw / bw / fw
    or bw / fw / bw."""
    call = Call(cached_reference(wname, "windows20000"))
    _held_at_any_grid(kernel, wname, call, lambda geo: wi.require(geo, 3, "odd"), "20,000 windows, three rounds, odd grid")


@pytest.mark.parametrize("form", ["windows", "read_at"])
@pytest.mark.parametrize("wname", WEIGHTS, ids=str)
def test_three_rounds_on_an_even_grid_with_the_ragged_tile_last(wname, form, kernel):
    """Every workgroup runs the same direction three times; n = 128 (T - 1) + 16, so the ragged tile's two items are the last round of their
    workgroups.  Once through materialised windows, once through dm_predict_read_at on the pool as a row matrix (block k = rows 21 k .. 21 k + 20,
    centres 21 k + 10): the widx addressing in later items."""
    found = searched(kernel.device, 3, "even", exact=True)
    n = wi.TILE * (found.ntiles - 1) + 16
    index = wi.mixed_index(n)
    call = Call(pool_reference(wname).view(index), form, index)

    def premise(geo):
        wi.require(geo, 3, "even", exact=True)
        assert set(range(wi.TILE * (geo.ntiles - 1), n)) <= set(wi.last_round_windows(geo, n)), "PREMISE BROKEN: the ragged tile is not in the last round: " + geo.describe()
    _held_at_any_grid(kernel, wname, call, premise, "three rounds, even grid, ragged tile last, %s" % form)


@pytest.mark.parametrize("parity", ["odd", "even"])
@pytest.mark.parametrize("wname", WEIGHTS, ids=str)
def test_four_rounds(wname, parity, kernel):
    """A third and a fourth item of every workgroup: alternating directions on the odd grid, one direction four times on the even one."""
    exact = parity == "even"
    found = searched(kernel.device, 4, parity, exact)
    n = wi.TILE * (found.ntiles - 1) + 77
    index = wi.mixed_index(n, offset=1201)
    call = Call(pool_reference(wname).view(index), "windows", index)
    _held_at_any_grid(kernel, wname, call, lambda geo: wi.require(geo, 4, parity, exact), "four rounds, %s grid" % parity)


@pytest.mark.parametrize("hot_parity", [0, 1], ids=["hot_quiet_hot", "quiet_hot_quiet"])
@pytest.mark.parametrize("parity", ["even", "odd"])
@pytest.mark.parametrize("wname", WEIGHTS, ids=str)
def test_poisoned_predecessor(wname, parity, hot_parity, kernel):
    """Rounds 0 and 2 hold read-shaped windows on the +-5 clip (long events, saturated cells), round 1 quiet synthetic ones - and the other way
    round.  Every window is held to the oracle; each quiet tile is bit-identical to the same 128 windows in a call of their own (two items, one per
    workgroup): c, h, an accumulator, a ring slot or stale scratch leaking from one item into the next shows here."""
    exact = parity == "even"
    found = searched(kernel.device, 3, parity, exact)
    index, hot, block = wi.poisoned_index(found, hot_parity)
    call = Call(pool_reference(wname).view(index), "windows", index)
    ref = pool_reference(wname)

    def premise(geo):
        wi.require(geo, 3, parity, exact)
        assert (geo.ntiles, geo.grid) == (found.ntiles, found.grid), "PREMISE BROKEN: the call runs on another grid than the one its tiles were filled for: %s" % geo.describe()
        other, same = wi.require_poisoned(geo, hot)
        _once("[items]  %-5s %s poisoned predecessor, %s grid, hot rounds %s: %d hot tiles, %d quiet; %d later items follow a tile of the other kind, %d one of their own" %
              (kernel.precision, wname, parity, "0 and 2" if hot_parity == 0 else "1", int(hot.sum()), int((~hot).sum()), other, same))

    def alone(p, head, prob, geo):
        out, single = [], {}
        p.reserve(True)
        for t in np.flatnonzero(~hot):
            q = int(block[t])
            if q not in single:
                single[q], g = p.run(Call(ref.view(wi.quiet_block(q)), "windows"))
                if not (g.rounds == 1 and g.grid == g.items == 2):
                    raise AssertionError("PREMISE BROKEN: a call of one tile meant to run one item per workgroup: " + g.describe())
            d = _same_bits(prob[t * wi.TILE:(t + 1) * wi.TILE], single[q])
            if d.size:
                out.append("quiet tile %d (round %d): %d windows differ from the same windows run alone, first at lane %d" % (t, geo.tile_round()[t], d.size, d[0]))
        return out[:8] + (["... %d quiet tiles in all" % len(out)] if len(out) > 8 else [])
    _held_at_any_grid(kernel, wname, call, premise, "poisoned predecessor, %s grid, %s" % (parity, "hot/quiet/hot" if hot_parity == 0 else "quiet/hot/quiet"), alone)


@pytest.mark.parametrize("precision", ["f16x3", "f16i8"])
def test_range_violation_from_a_later_item(precision, gpu_device, hip_lib):
    """One unrepresentable value in a row that only ONE window reads - a window of a full tile of the last round, then a window of the ragged tile
    (also last round) - must fail the call with DM_ERANGE, whichever direction's item reads the row; the same value in a block no selected centre
    reads must not, and the outputs stay the clean call's bits."""
    found = searched(gpu_device, 3, "even", exact=True)
    n = wi.TILE * (found.ntiles - 1) + 16
    base_index = wi.mixed_index(n)
    last = sorted(wi.last_round_windows(found, n))
    ragged0 = wi.TILE * (found.ntiles - 1)
    places = [("a full tile of the last round", last[0] + 37), ("the ragged tile", ragged0 + 5)]
    assert last[0] + 37 < ragged0 <= ragged0 + 5 < n and set(i for _, i in places) <= set(last), "PREMISE BROKEN: " + found.describe()
    rows = np.array(wi.pool_rows(pool()))
    poisons = [(0, 1.0e6), (4, np.nan), (wi.NFEAT - 1, 1.0e30)]                # beyond 65504, NaN, an event length beyond 65504 * 2^10
    failures = []
    with Probe(weights((17, 4.0)), hp.dense_head(1), precision, gpu_device) as p:
        p.reserve(True)
        for where, i in places:
            index = base_index.copy()
            index[i] = wi.LONE
            assert (index == wi.LONE).sum() == 1 and not (index == wi.UNREAD).any()
            clean, geo = p.run(Call(None, "read_at", index, rows))
            wi.require(geo, 3, "even", exact=True)
            assert geo.item_round()[2 * (i // wi.TILE)] == geo.item_round()[2 * (i // wi.TILE) + 1] == 2
            print("[items]  %-5s range flag from window %d in %s (tile %d, round 2 of its workgroups): %s" % (precision, i, where, i // wi.TILE, geo.describe()))
            for j, (row, reader) in enumerate([(0, "forward step 0"), (3, "forward"), (10, "both"), (17, "backward"), (20, "backward step 0")]):
                f, v = poisons[j % len(poisons)]
                bad = rows.copy()
                bad[wi.WIN * wi.LONE + row, f] = v
                try:
                    p.run(Call(None, "read_at", index, bad))
                    failures.append("ACCEPTED: %r on feature %d of row %d (%s) of window %d in %s" % (v, f, row, reader, i, where))
                except _lib.DeepModRangeError:
                    pass
                again, _ = p.run(Call(None, "read_at", index, rows))                 # the flag does not stick
                if _same_bits(again, clean).size:
                    failures.append("the clean call gives other bits after the refusal at row %d of window %d" % (row, i))
                unread = rows.copy()
                unread[wi.WIN * wi.UNREAD + row, f] = v
                try:
                    got, _ = p.run(Call(None, "read_at", index, unread))
                    if _same_bits(got, clean).size:
                        failures.append("a block no centre selects changed the outputs (row %d)" % row)
                except _lib.DeepModRangeError:
                    failures.append("REFUSED although no selected centre reads it: %r on feature %d of row %d of the unread block" % (v, f, row))
            # and the lone window's block itself is harmless when no centre selects it
            bad = rows.copy()
            bad[wi.WIN * wi.LONE + 10, 0] = 1.0e6
            try:
                p.run(Call(None, "read_at", base_index, bad))
            except _lib.DeepModRangeError:
                failures.append("REFUSED although no selected centre reads the lone block")
    assert not failures, "\n".join(failures)


def teardown_module(module):
    p = _SEARCHED.pop("probe", None)
    if p is not None:
        p.m.close()
