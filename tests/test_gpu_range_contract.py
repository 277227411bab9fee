"""GPU (-m gpu): the input range contract of the split-f16 kernels (include/deepmod_hip.h: DM_PREC_F16X3, DM_PREC_F16I8) held at EVERY input position.

An input the f16 operands cannot carry - features 0..5 beyond +-65504, an event length beyond 65504 * 2^k (k = DM_INFO_F16_LENGTH_SHIFT), a NaN - must fail the
call with DM_ERANGE; the streaming worker's last line of defence against a wrong BED is that flag.  The check lives in the layer-0 stage of the kernel, per lane,
per window half and per step, on a row prefetched a step earlier (step 0 on its own path).  Dropping it for one step, one direction, one lane group or one window
half changes no output bit, so no parity test can see it: these tests poison ONE cell at a time (tests/range_contract.py; tests/test_range_contract.py checks
the cases on the CPU) and ask for the error - and for a clean call right after, for the values exactly ON the bounds, for the rows nobody reads, and for the
marker that owns the launch when calls are asynchronous.

Where the poisoned cell decides who must see it: rows 0..9 of a window are read by the forward work item only, rows 11..20 by the backward one; a window's place
in its wave is window mod 32 (two halves of 16 = the MFMA rows); window 128 is the lone window of a ragged tile, re-read by that tile's dead lanes."""
import numpy as np
import pytest

import range_contract as rc
from deepmod_amd import _lib, model, synth
from oracle import oracle_np
from test_gpu_parity import TOL, TOL_I8, _check

pytestmark = pytest.mark.gpu

PREC = {"f32": _lib.DM_PREC_F32, "f16x3": _lib.DM_PREC_F16X3, "f16i8": _lib.DM_PREC_F16I8}
_ORACLE = {}


def _weights():
    return synth.synthetic_weights(22, 4.0)


def _oracle(key, w, x):
    """The C oracle, once per (weights, input) for all precisions."""
    if key not in _ORACLE:
        _ORACLE[key] = oracle_np.predict_windows_c(w, x)
    return _ORACLE[key]


def _model(w, prec, device):
    m = model.BiLSTMModel(w, device=device, precision=prec)
    assert m.get_info(_lib.DM_INFO_PRECISION) == PREC[prec] and m.get_info(_lib.DM_INFO_F16_REPRESENTABLE) == 1
    return m


@pytest.fixture(scope="module")
def base():
    x = synth.synthetic_windows(rc.N_BASE, seed=41)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module", params=["f16x3", "f16i8"])
def split(gpu_device, request):
    """One model per split precision on ordinary weights, its k, its tolerance against the oracle."""
    class S:
        pass
    s = S()
    s.prec, s.tol, s.device = request.param, (TOL_I8 if request.param == "f16i8" else TOL), gpu_device
    s.w = _weights()
    s.m = _model(s.w, s.prec, gpu_device)
    s.k = s.m.get_info(_lib.DM_INFO_F16_LENGTH_SHIFT)
    assert s.k == 10                                    # ordinary weights
    yield s
    s.m.close()


def _bits(prob, cls):
    return prob.view(np.uint32).copy(), cls.copy()


def _sweep(m, base, cases, clean_every=1):
    """Every case: one call that must raise DM_ERANGE; after every clean_every-th one, the clean batch must pass and give the bits it gave before."""
    want = _bits(*m.predict_windows(base))
    failures = []
    for i, case in enumerate(cases):
        try:
            m.predict_windows(rc.poisoned(base, case))
            failures.append("ACCEPTED: " + rc.describe(case))
        except _lib.DeepModRangeError:
            pass
        if i % clean_every == 0:
            try:
                got = _bits(*m.predict_windows(base))
            except _lib.DeepModRangeError:
                failures.append("the flag STUCK (clean call refused) after: " + rc.describe(case))
            else:
                if not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                    failures.append("clean call gives other bits after: " + rc.describe(case))
    assert not failures, "%d failures in %d cases:\n%s" % (len(failures), len(cases), "\n".join(failures[:60]))


def test_every_cell_of_one_window_is_checked(split, base):
    """S1: all 21 x 7 cells of window 77, poison kinds rotating; a clean call after every case."""
    _sweep(split.m, base, rc.s1_cases(split.k))


def test_every_window_of_a_full_and_a_ragged_tile_is_checked(split, base):
    """S2: windows 0..128 (every lane of every wave, both window halves, the lone window of the ragged tile) at five cells: forward step 0, backward step 0 on
    the length, the last step of both directions, one more row of either direction.  S2 is run whole, with a clean call after every case: 1,290 calls of 129
    windows.  Should the module's time on the GPU ask for it (profiles/range_contract/README.md), range_contract.S2_THIN is the subset to keep."""
    _sweep(split.m, base, rc.s2_cases(split.k))


@pytest.mark.parametrize("k_target", [10, 5, 0])
def test_values_on_the_bounds_pass_and_their_neighbours_are_refused(split, base, k_target):
    """The bounds themselves, read from the model: on ordinary weights (k = 10) and on models whose layer-0 length row is scaled up by a power of two until the
    library reports k = 5 and k = 0.  +-65504 on every cell of features 0..5, +-65504 * 2^k on every length, -0.0 and the fp32 predecessor of 65504 everywhere:
    each one call that passes AND agrees with the C oracle at the precision's tolerance; the fp32 successor of 65504 on one cell of each of features 0..5 and
    +-65505 * 2^k on one length: refused."""
    factor = 1.0 if k_target == 10 else rc.length_row_factor(split.w, k_target)
    w = rc.length_row_scaled(split.w, factor)
    m = split.m if k_target == 10 else _model(w, split.prec, split.device)
    k = m.get_info(_lib.DM_INFO_F16_LENGTH_SHIFT)
    assert k == k_target
    try:
        for name, x in rc.pass_cases(base, k).items():
            prob, cls = m.predict_windows(x)                        # a DeepModRangeError here: a value ON the bound was refused
            ref_prob, ref_cls = _oracle((k_target, name), w, x)
            err = _check(prob, cls, ref_prob, ref_cls, split.tol)
            print("%s k=%d %s: max|dp| = %.3g" % (split.prec, k, name, err))
        _sweep(m, base, rc.raise_boundary_cases(k))
    finally:
        if m is not split.m:
            m.close()


@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("at", [False, True], ids=["predict_read", "predict_read_at"])
def test_rows_forms_check_the_rows_they_read_and_no_others(split, at, resident):
    """dm_predict_read / dm_predict_read_at on host arrays and on device-resident ones, 129 windows: the first context row (only the first window's forward
    step 0 reads it), the last one (only the last window's backward step 0), a mid row - refused; the rows right outside, NaN included, and (read_at) a row in a
    gap between two centres - not refused, and the outputs are the clean call's bit for bit."""
    m, dev = split.m, split.device
    m_rows = rc.rows_m(at)
    rows = synth.synthetic_windows(m_rows, seed=43)[:, 10, :].copy()
    centres = rc.at_centres()
    keep = []

    def call(r):
        if not resident:
            return _bits(*(m.predict_read_at(r, centres) if at else m.predict_read(r, rc.ROWS_FIRST, rc.ROWS_COUNT)))
        d_r = model.DeviceArray.from_host(r, dev)
        d_p = model.DeviceArray((rc.ROWS_COUNT, 2), np.float32, dev)
        d_c = model.DeviceArray((rc.ROWS_COUNT,), np.uint8, dev)
        d_i = model.DeviceArray.from_host(centres, dev)
        keep[:] = [d_r, d_p, d_c, d_i]
        try:
            if at:
                m.predict_read_at(d_r, d_i, prob=d_p, cls=d_c)
            else:
                m.predict_read(d_r, rc.ROWS_FIRST, rc.ROWS_COUNT, prob=d_p, cls=d_c)
            return _bits(d_p.to_host(), d_c.to_host())
        finally:
            for d in keep:
                d.free()

    want = call(rows)
    failures = []
    for row, f, v, must_raise in rc.rows_edge_cases(split.k, at):
        r = rows.copy()
        r[row, f] = v
        what = "row %d (first read row %d, last read row %d) feature %d value %r" % (row, rc.ROWS_FIRST - 10, max(rc.rows_read(at)), f, float(v))
        try:
            got = call(r)
        except _lib.DeepModRangeError:
            if not must_raise:
                failures.append("REFUSED although no window reads it: " + what)
        else:
            if must_raise:
                failures.append("ACCEPTED: " + what)
            elif not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
                failures.append("an unread row changed the outputs: " + what)
        got = call(rows)                                            # the flag does not stick
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
    assert not failures, "\n".join(failures)


def test_fp32_kernel_takes_the_same_inputs(gpu_device, base):
    """Control: with DM_PREC_F32 ten of the S1 cases with finite poison are never refused and agree with the C oracle."""
    w = _weights()
    m = _model(w, "f32", gpu_device)
    k = m.get_info(_lib.DM_INFO_F16_LENGTH_SHIFT)
    finite = [c for c in rc.s1_cases(k) if np.isfinite(c[3])]
    by_f = [[c for c in finite if c[2] == f] for f in range(7)]
    picked = [by_f[f][(2 * f) % len(by_f[f])] for f in range(7)] + [by_f[rc.LENGTH][-1], by_f[4][-1], by_f[0][-1]]      # every feature, early and late rows
    assert len(set(c[:3] for c in picked)) == 10
    for case in picked:
        x = rc.poisoned(base, case)
        prob, cls = m.predict_windows(x)
        ref_prob, ref_cls = oracle_np.predict_windows_c(w, x)
        try:
            _check(prob, cls, ref_prob, ref_cls, TOL)
        except AssertionError as exc:
            raise AssertionError("%s: %s" % (rc.describe(case), exc))
    m.close()


# ---- reporting: which call, which marker ------------------------------------------------------------------------------------------------------------

class _Async:
    """A model with DM_OPT_ASYNC = 1 and device-resident feature rows, clean and with one poisoned cell, as the streaming worker holds them."""

    def __init__(self, split, row, feature, batches):
        self.m = _model(split.w, split.prec, split.device)
        self.m.set_option(_lib.DM_OPT_ASYNC, 1)
        self.m_rows = rc.rows_m(False)
        rows = synth.synthetic_windows(self.m_rows, seed=43)[:, 10, :].copy()
        bad = rows.copy()
        bad[row, feature] = rc.poison_kinds(feature, split.k)[0]
        self.d_clean = model.DeviceArray.from_host(rows, split.device)
        self.d_bad = model.DeviceArray.from_host(bad, split.device)
        self.d_cls = model.DeviceArray((batches, self.m_rows), np.uint8, split.device)

    def launch(self, batch, poisoned):
        self.m.predict_rows_device((self.d_bad if poisoned else self.d_clean).ptr, self.m_rows, rc.ROWS_FIRST, rc.ROWS_COUNT,
                                   self.d_cls.ptr + batch * self.m_rows + rc.ROWS_FIRST)

    def classes(self):
        return self.d_cls.to_host()[:, rc.ROWS_FIRST:rc.ROWS_FIRST + rc.ROWS_COUNT]

    def close(self):
        for d in (self.d_clean, self.d_bad, self.d_cls):
            d.free()
        self.m.close()


def _raises_range(fn, *args):
    try:
        fn(*args)
    except _lib.DeepModRangeError:
        return True
    return False


@pytest.mark.parametrize("j,row,feature", [(3, rc.ROWS_FIRST - 10, 0), (9, rc.ROWS_FIRST + rc.ROWS_COUNT + 9, rc.LENGTH)], ids=["batch3_first_row", "batch9_last_row"])
def test_violation_is_reported_once_at_the_marker_of_its_batch(split, j, row, feature):
    """Ten batches through markers i % DM_MARKS, each marker waited for before it is recorded again; batch j alone holds a poisoned cell: wait_mark raises
    exactly once, exactly at batch j's marker, dm_model_sync is clean afterwards and the other batches' classes are untouched."""
    marks, n = rc.dm_marks(), 10
    a = _Async(split, row, feature, n)
    raised = []
    for b in range(n):
        s = b % marks
        if b >= marks and _raises_range(a.m.wait_mark, s):
            raised.append(b - marks)
        a.launch(b, b == j)
        a.m.mark(s)
    for b in range(max(0, n - marks), n):
        if _raises_range(a.m.wait_mark, b % marks):
            raised.append(b)
    assert raised == [j], "DM_ERANGE of batch %d was reported at the markers of batches %s" % (j, raised)
    for s in range(marks):
        a.m.wait_mark(s)                                            # reported once
    a.m.sync()
    cls = a.classes()
    clean = [b for b in range(n) if b != j]
    assert all(np.array_equal(cls[b], cls[clean[0]]) for b in clean)
    a.close()


def test_marker_recorded_again_before_anybody_waited_leaves_the_violation_to_sync(split):
    """Marker 0 recorded after the poisoned launch and again after a clean one, nobody waited in between: wait_mark(0) covers the launches since the marker
    recorded before it - the clean one - and dm_model_sync reports the violation, once."""
    a = _Async(split, rc.ROWS_FIRST + 50, 4, 2)
    a.launch(0, True)
    a.m.mark(0)
    a.launch(1, False)
    a.m.mark(0)
    a.m.wait_mark(0)
    with pytest.raises(_lib.DeepModRangeError):
        a.m.sync()
    a.m.sync()
    a.m.wait_mark(0)
    a.close()


def test_more_markers_than_range_slots_never_lose_a_violation(split):
    """One poisoned launch, then marker 0 recorded eighteen times with no wait - more than the library has range slots (2 DM_MARKS + 2).  The violation is
    reported by the first dm_model_sync at the latest, exactly once, never zero times."""
    a = _Async(split, rc.ROWS_FIRST + 50, rc.LENGTH, 1)
    a.launch(0, True)
    for _ in range(18):
        a.m.mark(0)
    with pytest.raises(_lib.DeepModRangeError):
        a.m.sync()
    a.m.sync()
    a.m.wait_mark(0)
    a.launch(0, False)                                              # and the model goes on working: markers find slots again
    a.m.mark(0)
    a.m.wait_mark(0)
    a.launch(0, True)
    a.m.mark(1)
    with pytest.raises(_lib.DeepModRangeError):
        a.m.wait_mark(1)
    a.m.sync()
    a.close()


def test_poison_in_the_second_staged_batch_of_one_host_call(split):
    """One host call of 65,537 + 128 windows (staged as 65,536 + 129) with the poison in the last window, on the length of the backward work item's step 0: the call
    raises on return.  The module's single large case."""
    n = 65537 + 128
    x = np.tile(synth.synthetic_windows(1031, seed=47), (n // 1031 + 1, 1, 1))[:n]
    assert rc.in_contract(x, split.k)
    x[n - 1, 20, rc.LENGTH] = rc.length_beyond(split.k)
    with pytest.raises(_lib.DeepModRangeError):
        split.m.predict_windows(x)
    x[n - 1, 20, rc.LENGTH] = 3.0
    prob, cls = split.m.predict_windows(x)                          # the same call without the poison passes: the flag does not stick
    assert np.isfinite(prob).all() and np.array_equal(prob[:1031], prob[1031:2062])
