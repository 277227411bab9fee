"""The .xy text parser and row selection of `predict`, without a GPU: dm_xyload_parse_host runs the line routine the device runs
(csrc/xyparse.hip.inc, parse_row) compiled for the host.  Reference: np.loadtxt(dtype=float32, ndmin=2) of the same bytes
(myMultiBiRNN.py:307) - every table below is bit-equal to it WITH flag 0, so nothing passes by falling back - and
train.getDataFromFile_new / train.labelled_rows for the selection (:311-343)."""
import glob
import gzip
import io
import json
import os

import numpy as np
import pytest

from deepmod_amd import train, xyload

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def loadtxt(text):
    return np.loadtxt(io.BytesIO(text), dtype=np.float32, ndmin=2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_equal(text, rows=None):
    table, flag, bad = xyload.parse_host(text)
    assert (flag, bad) == (0, -1)
    want = loadtxt(text)
    assert table.shape == want.shape and np.array_equal(bits(table), bits(want))
    if rows is not None:
        assert len(table) == rows
    return table


def rows_of(values):
    """values [R][10] of strings -> text"""
    return ("\n".join(" ".join(r) for r in values) + "\n").encode()


def column_text(fields):
    """one field per row in column 9, zeros elsewhere"""
    return rows_of([["0.000"] * 9 + [f] for f in fields])


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "getfeatures", "*.json.gz"))), ids=os.path.basename)
def test_the_recorded_feature_files_parse_bit_equal(path):
    files = json.load(gzip.open(path))["files"]
    assert files
    for f in files.values():
        check_equal(f["xy"].encode())


def test_every_thousandth_up_to_twenty():
    fields = ["%.3f" % (k / 1000.0) for k in range(-20000, 20001)] + ["-0.000"]
    table = check_equal(column_text(fields))
    assert bits(table[-1, 9]) == 0x80000000                      # -0.000 is -0.0


def test_random_float32_values_printed_with_three_decimals():
    rng = np.random.default_rng(5)                                # magnitudes log-uniform in [1e-3, 2^30): every field has digits to divide
    v = np.exp(rng.uniform(np.log(1e-3), np.log(2.0 ** 30), 100000)) * rng.choice([-1.0, 1.0], 100000)
    v = v.astype(np.float32)
    assert np.abs(v).max() < 2.0 ** 30 and len(np.unique(v)) > 99000
    v = v.reshape(-1, 10)
    out = io.BytesIO()
    np.savetxt(out, v.astype(np.float64), fmt="%.3f")
    check_equal(out.getvalue(), rows=10000)


def test_positions_around_two_to_the_24_and_digit_counts():
    fields = ["16777215.000", "16777216.000", "16777217.000", "999999999999.000", "7", "42", "123456789012345", "12345678901234.5", "0.00000000000001",
              "-999999999999999"]
    table = check_equal(rows_of([[f] + ["0.000"] * 9 for f in fields]))
    assert table[2, 0] == np.float32(16777216.0)                  # already rounded by the parse


def test_final_newline_single_row_and_empty_text():
    row = b"5.000 0.000 1.000 0.000 1.000 0.000 0.000 -1.250 0.125 3.000"
    assert np.array_equal(bits(check_equal(row + b"\n" + row, rows=2)), bits(check_equal(row + b"\n" + row + b"\n", rows=2)))
    check_equal(row + b"\n", rows=1)
    check_equal(row, rows=1)
    table, flag, bad = xyload.parse_host(b"")
    assert table.shape == (0, 10) and (flag, bad) == (0, -1)


GOOD = ["1.000", "0.000", "1.000", "0.000", "0.000", "1.000", "0.000", "-0.731", "0.250", "12.000"]


def with_field(i, f):
    return " ".join(GOOD[:i] + [f] + GOOD[i + 1:])


# name -> a line outside the grammar (include/deepmod_hip.h)
TRIGGERS = {
    "nan": with_field(8, "nan"), "inf": with_field(7, "inf"), "minus_inf": with_field(7, "-inf"), "exponent": with_field(9, "1.2e1"),
    "plus": with_field(7, "+0.731"), "tab": " ".join(GOOD[:4]) + "\t" + " ".join(GOOD[4:]), "two_spaces": " ".join(GOOD[:4]) + "  " + " ".join(GOOD[4:]),
    "carriage_return": " ".join(GOOD) + "\r", "empty_line": "", "comment": "# " + " ".join(GOOD), "nine_fields": " ".join(GOOD[:9]),
    "eleven_fields": " ".join(GOOD + ["1.000"]), "sixteen_digits": with_field(0, "1234567890123.456"), "no_whole_part": with_field(8, ".5"),
    "no_decimals": with_field(8, "5."), "leading_space": " " + " ".join(GOOD), "trailing_space": " ".join(GOOD) + " ",
}
PLACES = {"first": 0, "middle": 3, "last": 6}


def trigger_text(name, place):
    lines = [" ".join(GOOD)] * 7
    lines[PLACES[place]] = TRIGGERS[name]
    return ("\n".join(lines) + "\n").encode()


@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("name", sorted(TRIGGERS))
def test_a_line_outside_the_grammar_flags_the_file_and_the_host_loader_decides(name, place):
    text = trigger_text(name, place)
    table, flag, bad = xyload.parse_host(text)
    assert flag == 1 and bad == PLACES[place] + 1
    try:
        want = loadtxt(text)
    except Exception as exc:                                       # np.loadtxt refuses the text: so does the wrapper, with the same kind of error
        with pytest.raises(type(exc)):
            xyload.load_host(text)
        return
    got, flag, _ = xyload.load_host(text)
    assert flag == 1 and got.shape == want.shape and np.array_equal(bits(got), bits(want))


# ---- selection: train.labelled_rows is the statement; the device kernels are held to the same cases in test_gpu_xyload.py ----
def table_with_labels(n_rows, labelled, positions=None, positive=None):
    rng = np.random.default_rng(n_rows)
    t = np.zeros((n_rows, 10))                       # float64: a position above 2^24 reaches the text as written here
    t[:, 0] = np.arange(n_rows) if positions is None else positions
    t[np.arange(n_rows), 3 + rng.integers(0, 4, n_rows)] = 1.0
    t[:, 7:] = np.round(rng.normal(0, 1, (n_rows, 3)), 3)
    lab = np.asarray(labelled, dtype=np.int64)
    pos = np.zeros(len(lab), bool) if positive is None else np.asarray(positive, bool)
    t[lab[pos], 2] = 1.0
    t[lab[~pos], 1] = 1.0
    return t


def table_text(t):
    out = io.BytesIO()
    np.savetxt(out, t.astype(np.float64), fmt="%.3f")
    return out.getvalue()


def test_the_text_of_a_case_keeps_an_odd_position_above_two_to_the_24():
    assert b"\n16777217.000 " in table_text(table_with_labels(60, [], positions=ODD))


BIG = 16777216 + 2 * np.arange(60)              # float32 positions above 2^24 are even
ODD = 16777197 + np.arange(60)                  # row 20 is 16777217 in the text and 16777216 as float32: not above lo = 16777216
SELECTION_CASES = {
    # name: (table, test option, first short row or None)
    "edges_accepted": (table_with_labels(64, [10, 30, 53], positive=[1, 0, 1]), ['N', '100'], None),
    "row_9_refused": (table_with_labels(64, [9, 30]), ['N', '100'], 9),
    "row_R_minus_10_refused": (table_with_labels(64, [30, 54]), ['N', '100'], 54),
    "no_labelled_row": (table_with_labels(40, []), ['N', '100'], None),
    "every_row_labelled": (table_with_labels(30, range(30)), ['N', '100'], 0),
    "minus_between_rounded_positions": (table_with_labels(60, range(10, 50), positions=BIG, positive=np.arange(40) % 3 == 0), ['-', 16777216 + 41, 16777216 + 61], None),
    "plus_between_rounded_positions": (table_with_labels(60, range(10, 50), positions=BIG, positive=np.arange(40) % 3 == 0), ['+', 16777216 + 41, 16777216 + 61], None),
    "plus_with_a_position_the_parse_rounds_onto_the_bound": (table_with_labels(60, range(10, 50), positions=ODD), ['+', 16777216, 16777240], None),
    "minus_with_a_position_the_parse_rounds_onto_the_bound": (table_with_labels(60, range(10, 50), positions=ODD), ['-', 16777216, 16777240], None),
    "every_row_labelled_inside_plus": (table_with_labels(300, range(300), positions=1000 + np.arange(300), positive=np.arange(300) % 2 == 1), ['+', 1009, 1290], None),
    "plus_excludes_a_short_row": (table_with_labels(64, [5, 30, 31], positions=1000 + np.arange(64)), ['+', 1020, 1040], None),
}


def statement(table, test):
    """(centres, labels) of train.labelled_rows, or the row its error names"""
    try:
        rows = train.labelled_rows(table, {"windowsize": 21, "test": test}, "f")
    except ValueError as exc:
        return int(str(exc).split("labelled row ")[1].split()[0])
    return rows.astype(np.int32), (table[rows, 2].astype(int) == 1).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(SELECTION_CASES))
def test_the_selection_cases_mean_what_they_say(name):
    table, test, short = SELECTION_CASES[name]
    got = statement(loadtxt(table_text(table)), test)
    if short is not None:
        assert got == short
        return
    centres, labels = got
    if name == "no_labelled_row":
        assert len(centres) == 0
    if name == "edges_accepted":
        assert centres.tolist() == [10, 30, 53] and labels.tolist() == [1, 0, 1]
    if name.endswith("rounds_onto_the_bound"):                     # the float32 position decides: a double comparison would keep row 20 inside
        assert (20 in centres.tolist()) == (test[0] == '-') and (21 in centres.tolist()) == (test[0] == '+')
    if name.endswith("between_rounded_positions"):
        inside = [r for r in range(10, 50) if 16777216 + 41 < int(BIG[r]) < 16777216 + 61]
        assert 0 < len(inside) < 40
        assert centres.tolist() == (inside if test[0] == '+' else [r for r in range(10, 50) if r not in inside])
    # getDataFromFile_new returns the windows of exactly these rows
    x, y, _ = train.getDataFromFile_new(io.BytesIO(table_text(table)), {"windowsize": 21, "test": test})
    assert len(y) == len(centres) and (len(centres) == 0 or np.array_equal(np.asarray(y)[:, 1] == 1, labels == 1))


@pytest.mark.parametrize("name", sorted(SELECTION_CASES))
def test_the_host_twin_of_the_selection_is_the_numpy_statement(name):
    """dm_xyload_select_host runs row_wanted, the edge rule and the label rule of the kernels, on the host twin's own table."""
    table, test, short = SELECTION_CASES[name]
    text = table_text(table)
    mine, flag, _ = xyload.parse_host(text)
    assert flag == 0
    want = statement(loadtxt(text), test)
    lo, hi = (test[1], test[2]) if test[0] in "-+" else (0, 0)
    if short is not None:
        with pytest.raises(ValueError, match="f: labelled row %d is closer than 10 rows to the edge of the file" % short):
            xyload.select_host(mine, test[0], lo, hi, "f")
        return
    centre, label = xyload.select_host(mine, test[0], lo, hi, "f")
    assert centre.dtype == np.int32 and label.dtype == np.uint8 and np.array_equal(centre, want[0]) and np.array_equal(label, want[1])


def test_a_text_of_eleven_columns_is_refused_not_recut():
    """np.loadtxt accepts ten lines of eleven fields; cut into rows of ten they would be a table of garbage."""
    text = ((" ".join(GOOD + ["1.000"]) + "\n") * 10).encode()
    assert loadtxt(text).shape == (10, 11) and xyload.parse_host(text)[1:] == (1, 1)
    with pytest.raises(ValueError, match="10 columns"):
        xyload.load_host(text)
    assert xyload.loadtxt_host(b"").shape == (0, 10)
