"""The .xy text of one feature file -> its table and the labelled rows, on the GPU (dm_xyload_* of the C ABI, csrc/xyparse.hip.inc).

`XYLoader.load` is train.getDataFromFile_new without the windows: the table stays on the device as the feature rows dm_predict_read_at takes,
the labelled rows as its centres.  A text outside the device grammar (nan, inf, exponents, tabs ... - include/deepmod_hip.h) is loaded by
np.loadtxt and selected by train.labelled_rows on the host, and that result is uploaded: the outcome is the host loader's either way, NaN
rule and warning included.  `parse_host` is the device's line routine compiled for the host (no GPU needed).
"""
from __future__ import annotations

import ctypes
import io
from typing import Optional, Tuple

import numpy as np

from . import _lib, train

SHORT_ROW = "%s: labelled row %d is closer than %d rows to the edge of the file (%d rows): no whole window"      # train.labelled_rows' words
KIND = {'N': 0, '0': 0, '-': ord('-'), '+': ord('+')}


def tile_bytes() -> int:
    return _lib.load().dm_xyload_tile_bytes()


def scan_block() -> int:
    return _lib.load().dm_xyload_scan_block()


def parse_host(text: bytes) -> Tuple[np.ndarray, int, int]:
    """-> (table float32 [R,10], flag, first bad line (1-based, -1: none)); rows outside the grammar are zeros."""
    lib = _lib.load()
    flag, bad = ctypes.c_int32(0), ctypes.c_int64(-1)
    buf = ctypes.c_char_p(text)
    rows = lib.dm_xyload_parse_host(buf, len(text), None, 0, ctypes.byref(flag), ctypes.byref(bad))
    if rows < 0:
        _lib.check(int(rows))
    table = np.zeros((rows, 10), np.float32)
    if rows:
        lib.dm_xyload_parse_host(buf, len(text), table.ctypes.data, rows, ctypes.byref(flag), ctypes.byref(bad))
    return table, flag.value, bad.value


def loadtxt_host(text: bytes) -> np.ndarray:
    """What the host loader makes of the same bytes (np.loadtxt's own errors for a text it refuses)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # 'input contained no data' of an empty text
        table = np.loadtxt(io.BytesIO(text), dtype=np.float32, ndmin=2)
    if table.size == 0:
        return np.zeros((0, 10), np.float32)
    if table.shape[1] != 10:                            # the host loader would split such a table into other columns: not a feature file
        raise ValueError("a feature file has 10 columns (position, 2 labels, 7 features), this text has %d" % table.shape[1])
    return table


def load_host(text: bytes) -> Tuple[np.ndarray, int, int]:
    """parse_host with the fallback of XYLoader.load: the table of a flagged text is np.loadtxt's."""
    table, flag, bad = parse_host(text)
    if flag:
        table = loadtxt_host(text)
    return table, flag, bad


def select_host(table: np.ndarray, kind='N', lo: int = 0, hi: int = 0, fn: str = "<text>") -> Tuple[np.ndarray, np.ndarray]:
    """XYLoader.select on a host table by the routines the kernels run (no GPU needed) -> (centre int32 [n], label u8 [n])."""
    lib = _lib.load()
    table = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 10)
    centre, label = np.empty(len(table), np.int32), np.empty(len(table), np.uint8)
    short = ctypes.c_int64(-1)
    n = lib.dm_xyload_select_host(table.ctypes.data, len(table), KIND[kind], int(lo), int(hi), centre.ctypes.data, label.ctypes.data, len(table), ctypes.byref(short))
    if n < 0 and short.value >= 0:
        raise ValueError(SHORT_ROW % (fn, short.value, 10, len(table)))
    if n < 0:
        _lib.check(int(n))
    return centre[:n].copy(), label[:n].copy()


class XYLoader:
    """One dm_xyload on one GPU; its buffers grow and are kept between files."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        self.device = device
        self._h = self._lib.dm_xyload_create(device)
        if not self._h:
            raise _lib.DeepModHipError("dm_xyload_create: " + _lib.last_error())
        self.n_rows, self.n = -1, -1

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dm_xyload_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def parse(self, text: bytes) -> Tuple[int, int, int]:
        """-> (rows, flag, first bad line)"""
        rows, flag, bad = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(-1)
        self.n_rows = self.n = -1
        _lib.check(self._lib.dm_xyload_parse(self._h, ctypes.c_char_p(text), len(text), ctypes.byref(rows), ctypes.byref(flag), ctypes.byref(bad)))
        self.n_rows = rows.value
        return rows.value, flag.value, bad.value

    def set_table(self, table: np.ndarray):
        table = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 10)
        self.n_rows = self.n = -1
        _lib.check(self._lib.dm_xyload_set_table(self._h, table.ctypes.data, len(table)))
        self.n_rows = len(table)

    def select(self, kind='N', lo: int = 0, hi: int = 0, fn: str = "<text>") -> int:
        """-> n; ValueError with the loader's words for a labelled row without a whole window."""
        short = ctypes.c_int64(-1)
        self.n = -1
        n = self._lib.dm_xyload_select(self._h, KIND[kind], int(lo), int(hi), ctypes.byref(short))
        if n < 0 and short.value >= 0:
            raise ValueError(SHORT_ROW % (fn, short.value, 10, self.n_rows))
        if n < 0:
            _lib.check(int(n))
        self.n = int(n)
        return self.n

    def set_selection(self, centre: np.ndarray, label: np.ndarray):
        centre = np.ascontiguousarray(centre, dtype=np.int32)
        label = np.ascontiguousarray(label, dtype=np.uint8)
        self.n = -1
        _lib.check(self._lib.dm_xyload_set_selection(self._h, centre.ctypes.data, label.ctypes.data, len(centre)))
        self.n = len(centre)

    def device_pointers(self) -> Tuple[Optional[int], Optional[int], int, int]:
        """-> (feats address, centre address, rows, n)"""
        feats, centre, rows, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self._lib.dm_xyload_device(self._h, ctypes.byref(feats), ctypes.byref(centre), ctypes.byref(rows), ctypes.byref(n)))
        return feats.value, centre.value, rows.value, n.value

    def fetch_table(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (feats [R,7], head [R,3]): the whole table, 40 bytes per row - tests and tools; `predict` leaves it on the device."""
        feats, head = np.empty((self.n_rows, 7), np.float32), np.empty((self.n_rows, 3), np.float32)
        _lib.check(self._lib.dm_xyload_fetch(self._h, feats.ctypes.data, head.ctypes.data, None, None))
        return feats, head

    def fetch_head(self) -> np.ndarray:
        """-> head [R,3] (position, two labels) alone: 12 bytes per row (`train --resident` takes its y from it)."""
        head = np.empty((self.n_rows, 3), np.float32)
        _lib.check(self._lib.dm_xyload_fetch(self._h, None, head.ctypes.data, None, None))
        return head

    def fetch_selection(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (centre int32 [n], label u8 [n])"""
        centre, label = np.empty(max(self.n, 0), np.int32), np.empty(max(self.n, 0), np.uint8)
        _lib.check(self._lib.dm_xyload_fetch(self._h, None, None, centre.ctypes.data, label.ctypes.data))
        return centre, label

    def classify(self, model) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The selected windows through model (a model.BiLSTMModel) -> (probability of class 1 float32 [n], class u8 [n], label u8 [n]):
        6 bytes per window come back, the table stays on the device.  Inputs the split-f16 kernel cannot represent are computed by the fp32
        kernel, as Session.run does."""
        prob1, cls, label = np.empty(max(self.n, 0), np.float32), np.empty(max(self.n, 0), np.uint8), np.empty(max(self.n, 0), np.uint8)
        if self.n <= 0:
            return prob1, cls, label

        def run():
            _lib.check(self._lib.dm_xyload_classify(self._h, model._h, prob1.ctypes.data, cls.ctypes.data, label.ctypes.data))
        try:
            run()
        except _lib.DeepModRangeError:
            keep = model.get_info(_lib.DM_INFO_PRECISION)
            model.set_option(_lib.DM_OPT_PRECISION, _lib.DM_PREC_F32)
            try:
                run()
            finally:
                model.set_option(_lib.DM_OPT_PRECISION, keep)
        return prob1, cls, label

    def times(self) -> Tuple[float, float]:
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _lib.check(self._lib.dm_xyload_times(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def load(self, text: bytes, moptions, fn: str = "<text>") -> Tuple[int, int, bool]:
        """One file: parse + select under moptions['test'] (['N', ..] | ['0', ..]: every labelled row; ['-' | '+', lo, hi]).
        -> (rows, n, fallback).  A flagged text is named with its first offending line and loaded on the host."""
        test = moptions['test']
        rows, flag, bad = self.parse(text)
        if not flag:
            lo, hi = (test[1], test[2]) if test[0] in ('-', '+') else (0, 0)
            return rows, self.select(test[0], lo, hi, fn), False
        print("Note: %s: line %d is not in the form the GPU parser takes: the file is loaded on the host" % (fn, bad))
        table = loadtxt_host(text)
        sel = train.labelled_rows(table, moptions, fn)
        self.set_table(table)
        self.set_selection(sel, table[sel, 2].astype(int) == 1)
        return len(table), len(sel), True


class XYSet:
    """One dm_xyset on one GPU: loaded files kept on the device as segments (feature rows [R][7], centres int32 [n], labels u8 [n] - 28 bytes per
    row + 5 per window), classified again and again without their text being read a second time (`train --validate`), or the source of a
    training step's windows by id (`train --resident 1`: gather, Trainer.step_set)."""

    def __init__(self, device: int = 0, initial_rows: int = 1 << 16):
        self._lib = _lib.load()
        self.device = device
        self._h = self._lib.dm_xyset_create(device, int(initial_rows))
        if not self._h:
            raise _lib.DeepModHipError("dm_xyset_create: " + _lib.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dm_xyset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, loader: XYLoader) -> bool:
        """The loader's table and selection become the next segment -> whether one was added (a file without a window adds none)."""
        _lib.check(self._lib.dm_xyset_append(self._h, loader._h))
        return loader.n > 0

    def segments(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (rows int64 [k], windows int64 [k]) of the k segments"""
        k = int(self._lib.dm_xyset_segments(self._h, None, None, 0))
        if k < 0:
            _lib.check(k)
        rows, windows = np.zeros(k, np.int64), np.zeros(k, np.int64)
        if k:
            self._lib.dm_xyset_segments(self._h, rows.ctypes.data, windows.ctypes.data, k)
        return rows, windows

    def nbytes(self) -> int:
        return int(self._lib.dm_xyset_bytes(self._h))

    def gather(self, ids) -> np.ndarray:
        """The windows of ids (a window's id is its index over the concatenated segments) -> float32 [n,21,7], gathered on the device: what
        train.getDataFromFile_new returns for those windows of the segments' files."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        x = np.empty((len(ids), 21, 7), np.float32)
        _lib.check(self._lib.dm_xyset_gather(self._h, ids.ctypes.data, len(ids), x.ctypes.data))
        return x

    def classify(self, model, segment: int, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Segment `segment` through model -> (probability of class 1 float32 [n], class u8 [n], label u8 [n]), as XYLoader.classify gives them
        for the segment's file: a segment the split-f16 kernel cannot represent is computed by the fp32 kernel, that segment alone."""
        if n is None:
            n = int(self.segments()[1][segment])
        prob1, cls, label = np.empty(n, np.float32), np.empty(n, np.uint8), np.empty(n, np.uint8)

        def run():
            _lib.check(self._lib.dm_xyset_classify(self._h, model._h, int(segment), prob1.ctypes.data, cls.ctypes.data, label.ctypes.data))
        try:
            run()
        except _lib.DeepModRangeError:
            keep = model.get_info(_lib.DM_INFO_PRECISION)
            model.set_option(_lib.DM_OPT_PRECISION, _lib.DM_PREC_F32)
            try:
                run()
            finally:
                model.set_option(_lib.DM_OPT_PRECISION, keep)
        return prob1, cls, label
