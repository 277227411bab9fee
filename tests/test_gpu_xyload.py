"""The device text parser and row selection of `predict` (csrc/xyparse.hip.inc) on the GPU.  Reference: np.loadtxt(dtype=float32, ndmin=2) of
the same bytes (myMultiBiRNN.py:307), bit for bit and with flag 0, and train.labelled_rows (the selection of getDataFromFile_new, :311-343).
The shapes sit on the kernels' seams: T = dm_xyload_tile_bytes() text bytes per block, S = dm_xyload_scan_block() elements per scan block."""
import io

import numpy as np
import pytest

from deepmod_amd import model, synth, xyload
from test_xyload_host import PLACES, SELECTION_CASES, TRIGGERS, bits, loadtxt, statement, table_text, trigger_text

pytestmark = pytest.mark.gpu

SHORT = " ".join(["0.000"] * 10) + "\n"                               # 60 bytes
LONG = " ".join(["-12345678901234.5"] + ["123456789012.345"] * 9) + "\n"   # ten fields of 15 digits


@pytest.fixture(scope="module")
def loader(gpu_device):
    ld = xyload.XYLoader(gpu_device)
    yield ld
    ld.close()


def line_of(n_bytes):
    """a line of exactly n_bytes (60 .. 170) bytes with its newline: zeros with more decimals"""
    extra, fields = n_bytes - 60, []
    for _ in range(10):
        k = min(extra, 11)
        fields.append("0.000" + "7" * k)
        extra -= k
    assert extra == 0
    return " ".join(fields) + "\n"


def text_with_newline_at(offset, rows_after=5):
    """short lines, then one line whose '\\n' is byte `offset` of the text, then rows_after random rows"""
    q, rem = divmod(offset + 1, 60)
    head = SHORT * q if rem == 0 else SHORT * (q - 1) + line_of(60 + rem)
    assert head[offset] == "\n" and len(head) == offset + 1
    return (head + random_rows(rows_after, 1)).encode()


def random_rows(n, seed):
    rng = np.random.default_rng(seed)
    t = np.zeros((n, 10))
    t[:, 0] = rng.integers(0, 10 ** 9, n)
    t[:, 1:7] = rng.integers(0, 2, (n, 6))
    t[:, 7:] = rng.normal(0, 30, (n, 3))
    out = io.StringIO()
    np.savetxt(out, t, fmt="%.3f")
    return out.getvalue()


def parse_cases():
    T, S = xyload.tile_bytes(), xyload.scan_block()
    per_tile = T // 64
    cases = {"no_row": b"", "one_row": SHORT.encode(), "two_rows": (SHORT + LONG).encode(), "one_row_no_newline": SHORT.encode()[:-1],
             "shortest_lines": (SHORT * 200).encode(), "longest_lines": (LONG * 100).encode(),
             "newline_last_byte_of_a_tile": text_with_newline_at(T - 1), "newline_first_byte_of_a_tile": text_with_newline_at(T),
             "field_across_tiles": text_with_newline_at(T + 27), "newline_ends_the_third_tile": text_with_newline_at(3 * T - 1, rows_after=0),
             "random_three_tiles": random_rows(3 * T // 70, 2).encode()}
    for name, rows in (("tile", per_tile), ("scan_block", per_tile * S)):
        for d in (-1, 0, 1):
            cases["%s_of_lines_%+d" % (name, d)] = (line_of(64) * (rows + d)).encode()
    return cases


CASE_NAMES = ["no_row", "one_row", "two_rows", "one_row_no_newline", "shortest_lines", "longest_lines", "newline_last_byte_of_a_tile", "newline_first_byte_of_a_tile",
              "field_across_tiles", "newline_ends_the_third_tile", "random_three_tiles", "tile_of_lines_-1", "tile_of_lines_+0", "tile_of_lines_+1",
              "scan_block_of_lines_-1", "scan_block_of_lines_+0", "scan_block_of_lines_+1"]


@pytest.fixture(scope="module")
def cases(gpu_device):
    c = parse_cases()
    assert sorted(c) == sorted(CASE_NAMES)
    return c


def device_table(loader, text):
    rows, flag, bad = loader.parse(text)
    feats, head = loader.fetch_table()
    assert feats.shape == (rows, 7) and head.shape == (rows, 3)
    return np.concatenate([head, feats], axis=1), flag, bad


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_parse_is_bit_equal_to_loadtxt(loader, cases, name):
    text = cases[name]
    table, flag, bad = device_table(loader, text)
    assert (flag, bad) == (0, -1)
    want = loadtxt(text) if text else np.zeros((0, 10), np.float32)
    assert table.shape == want.shape and np.array_equal(bits(table), bits(want))
    again, _, _ = device_table(loader, text)
    assert again.tobytes() == table.tobytes()                            # two calls, the same bytes


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("name", sorted(TRIGGERS))
def test_device_flag_and_line_are_the_host_twins(loader, name, place):
    for text in (trigger_text(name, place), random_rows(2 * xyload.tile_bytes() // 70, 3).encode() + trigger_text(name, place)):
        _, flag, bad = xyload.parse_host(text)
        assert flag == 1 and bad > 0
        assert loader.parse(text)[1:] == (flag, bad)
        with pytest.raises(Exception, match="outside the device grammar"):
            loader.select()


def device_selection(loader, table, test):
    rows, flag, _ = loader.parse(table_text(table))
    assert flag == 0 and rows == len(table)
    lo, hi = (test[1], test[2]) if test[0] in "-+" else (0, 0)
    try:
        n = loader.select(test[0], lo, hi, "f")
    except ValueError as exc:
        return int(str(exc).split("labelled row ")[1].split()[0])
    centre, label = loader.fetch_selection()
    assert len(centre) == n
    return centre, label


@pytest.mark.parametrize("name", sorted(SELECTION_CASES))
def test_device_selection_is_the_numpy_statement(loader, name):
    table, test, short = SELECTION_CASES[name]
    got, want = device_selection(loader, table, test), statement(loadtxt(table_text(table)), test)
    if short is not None:
        assert got == want == short
    else:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].dtype == np.int32 and got[1].dtype == np.uint8


def big_table(n_rows):
    rng = np.random.default_rng(9)
    t = np.zeros((n_rows, 10), np.float32)
    t[:, 0] = 1000 + np.arange(n_rows)
    t[np.arange(n_rows), 3 + rng.integers(0, 4, n_rows)] = 1.0
    t[:, 7:] = np.round(rng.normal(0, 1, (n_rows, 3)), 3)
    positive = rng.random(n_rows) < 0.5
    t[:, 1], t[:, 2] = ~positive, positive
    return t


def test_every_row_labelled_over_several_scan_blocks(loader):
    n_rows = 3 * xyload.scan_block() + 7
    table, test = big_table(n_rows), ['+', 1009, 1000 + n_rows - 10]
    centre, label = device_selection(loader, table, test)
    want = statement(table, test)
    assert np.array_equal(centre, np.arange(10, n_rows - 10)) and np.array_equal(centre, want[0]) and np.array_equal(label, want[1])
    assert device_selection(loader, table, ['N', '100']) == 0            # without the region the first row has no window


def test_the_classifier_on_the_device_table_is_the_classifier_on_the_host_table(loader, gpu_device):
    table = big_table(700)
    table[::3, 1:3] = 0.0
    table[:10, 1:3] = table[-10:, 1:3] = 0.0
    text = table_text(table)
    rows, n, fallback = loader.load(text, {"windowsize": 21, "test": ['N', '100']}, "f")
    assert rows == 700 and not fallback and n > 300
    host = loadtxt(text)
    centres, labels = statement(host, ['N', '100'])
    m = model.BiLSTMModel(synth.synthetic_weights(seed=11, scale=4.0), gpu_device, precision="f16x3")
    try:
        want_prob, want_cls = m.predict_read_at(host[:, 3:], centres)
        feats_ptr, centre_ptr, r, k = loader.device_pointers()
        assert (r, k) == (rows, n) and n == len(centres)
        prob, cls = model.DeviceArray((n, 2), np.float32, gpu_device), model.DeviceArray(n, np.uint8, gpu_device)
        m.predict_rows_at_device(feats_ptr, rows, centre_ptr, n, cls.ptr, prob.ptr)
        m.sync()
        assert np.array_equal(bits(prob.to_host()), bits(want_prob)) and np.array_equal(cls.to_host(), want_cls)
        prob1, cls6, label6 = loader.classify(m)                          # the 6 bytes per window `predict` downloads
        assert np.array_equal(bits(prob1), bits(want_prob[:, 1])) and np.array_equal(cls6, want_cls) and np.array_equal(label6, labels)
    finally:
        m.close()


def test_a_flagged_text_is_loaded_by_the_host_loader(loader, capsys):
    """nan in a window: the table is np.loadtxt's, the rows are train.labelled_rows' (NaN windows dropped with the loader's warning)."""
    table = big_table(80)
    table[:10, 1:3] = table[-10:, 1:3] = 0.0
    text = table_text(table)
    lines = text.split(b"\n")
    cells = lines[40].split(b" ")
    cells[8] = b"nan"
    lines[40] = b" ".join(cells)
    text = b"\n".join(lines)
    mo = {"windowsize": 21, "test": ['N', '100']}
    rows, n, fallback = loader.load(text, mo, "some.xy.gz")
    out = capsys.readouterr().out
    assert fallback and rows == 80 and "some.xy.gz: line 41" in out and "Warning: NaN in a window of some.xy.gz" in out
    host = loadtxt(text)
    centres, labels = statement(host, ['N', '100'])
    assert n == len(centres) == 60 - 21
    (feats, head), (centre, label) = loader.fetch_table(), loader.fetch_selection()
    assert np.array_equal(bits(np.concatenate([head, feats], axis=1)), bits(host)) and np.array_equal(centre, centres) and np.array_equal(label, labels)
    assert loader.times() == (0.0, 0.0)
