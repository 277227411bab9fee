"""`DeepMod.py getfeatures`: raw reads + a reference + known modified positions -> the labelled *.xy.gz files `train` reads.

Counterpart of the reference's bin/DeepMod_scripts/myGetFeatureBasedPos.py with its names:

  getFeature_manager   :653-757   position lists, output folder, worker batches of --files_per_thread inputs
  getFeature_handler   :564-583   one batch -> <outFolder>/<batch id>/
  mGetFeature1         :28-103    events + signal statistics -> alignment records -> handle_record
  handle_record        :109-350   alignment walk, filters, get_Feature, the <k>.xy.gz / <k>.xy.ind files
  get_Feature          :355-528   labels, feature rows, the +-25 row selection
  handle_line          :541-559   one SAM line (readmap.handle_line: the same function as myDetect's)
  readFA, readMotifMod :588-647   the genome and the motif positions of both strands

Two paths give the same bytes.  mGetFeature1 is the command: the signal statistics of a batch stay on the device (signal.py), the alignment walk
and the labels run in compiled code on --threads host threads (dm_xy_read, csrc/xyrows.inc), the row selection and the text are HIP kernels
(dm_xy_rows, csrc/xyrows.hip.inc); the host cuts the text at read boundaries and gzips it.  handle_record is the per-read path over an f5data
dictionary (rawreads.get_Event_Signals) with the device stage stated in numpy below (xy_keep_np, xy_matrix_np, xy_text_np): what the CPU tests
hold to the reference's goldens and the GPU tests hold the kernels to.

Departures from the reference: inputs are sorted; one GPU process with host threads instead of a process per batch; an --outFolder that already
holds */*.xy.gz is refused, not deleted; --region takes a contig name only (the reference compares an int with a string for start / end and
raises TypeError under Python 3); the per-read progress prints are not reproduced; a read whose alignment table has fewer bases than aligned
events is reported ("Error alignment table") where the reference ends with an IndexError; only --fnum 7.
"""
from __future__ import annotations

import ctypes
import glob
import io
import os
import sys
import time
import zlib
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional

import numpy as np

from . import _lib
from .readmap import handle_line  # noqa: F401  (myGetFeatureBasedPos.handle_line is myDetect.handle_line)

GZIP_LEVEL = 1            # the contract is on the decompressed bytes; level 1 keeps the host's share of a run small
ROW_BYTES = 80            # feat_list.nbytes per row: 10 float64 (:120)
NEIGHBOURS = 25           # :516
XY_ERRORS = {_lib.DM_XY_LESS_EVENT: "Less(<500) events", _lib.DM_XY_INDEX_ERROR: "Error alignment table"}
_COMP = bytes.maketrans(b'ACGTacgt', b'TGCAtgca')


# ------------------------------------------------------------------------------------------------ position lists
def readFA(mfa, t_chr=None):
    """{contig: upper-cased sequence} of a FASTA file, of contig t_chr only if given (:588-610)."""
    fadict, cur, parts = {}, None, []
    with open(mfa, 'r') as mr:
        for line in mr:
            line = line.strip()
            if not line:
                continue
            if line[0] == '>':
                if cur is not None and t_chr in (None, cur):
                    fadict[cur] = ''.join(parts)
                cur, parts = line[1:].split()[0], []
            elif t_chr in (None, cur):
                parts.append(line.upper())
    if cur is not None and t_chr in (None, cur):
        fadict[cur] = ''.join(parts)
    return fadict


def _find_all(seq: bytes, pat: bytes) -> np.ndarray:
    """start indices of every (overlapping) occurrence of pat in seq"""
    s = np.frombuffer(seq, np.uint8)
    if len(s) < len(pat):
        return np.zeros(0, np.int64)
    hit = np.ones(len(s) - len(pat) + 1, bool)
    for k, ch in enumerate(pat):
        hit &= s[k:k + len(hit)] == ch
    return np.flatnonzero(hit).astype(np.int64)


def readMotifMod(fadict, mpat='Cg', mposinpat=0, t_chr=None, t_start=None, t_end=None):
    """(cpgdict, all_a) of :615-647 as sorted position arrays: cpgdict[contig] = {'+': positions of the motif's base of interest on the forward
    strand, '-': on the reverse strand (not those that are '+' already: the reference's elif)}, all_a the same for the single base."""
    pat3 = mpat.upper().encode('ascii')
    comp_pat3 = pat3.translate(_COMP)[::-1]
    comp_mposinpat = len(comp_pat3) - 1 - mposinpat
    base = mpat[mposinpat:mposinpat + 1].encode('ascii')              # (the reference compares with mpat as given: a lower-case base never matches)
    cpgdict, all_a = {}, {}

    def window(p):
        return p[(p >= (0 if t_start is None else t_start)) & (p <= (np.iinfo(np.int64).max if t_end is None else t_end))]
    for fak, seq in fadict.items():
        sb = seq.encode('ascii')
        plus = window(_find_all(sb, pat3) + mposinpat)
        minus = window(_find_all(sb, comp_pat3) + comp_mposinpat)
        minus = minus[~np.isin(minus, plus)]
        cpgdict[fak] = {'+': plus, '-': minus}
        a_plus = window(_find_all(sb, base))
        a_minus = window(_find_all(sb, base.translate(_COMP)))
        all_a[fak] = {'+': a_plus, '-': a_minus[~np.isin(a_minus, a_plus)]}
        print('%s%d site: %d(+) %d(-) for %s' % (pat3.decode(), mposinpat, len(plus), len(minus), fak))
    return cpgdict, all_a


def readPosFiles(pattern, fadict):
    """The lines `chr strand pos` of every file the pattern matches (:688-698) -> {contig: {'+': positions, '-': positions}}."""
    out = defaultdict(lambda: {'+': [], '-': []})
    for fn in sorted(glob.glob(pattern)):
        with open(fn) as fh:
            for line in fh:
                if not line.strip():
                    continue
                tchr, tstrand, tpos = line.split()[:3]
                if tchr not in fadict or not 0 <= int(tpos) < len(fadict[tchr]) or tstrand not in ('+', '-'):
                    raise ValueError('%s: position %s %s %s is not in the reference' % (fn, tchr, tstrand, tpos))
                out[tchr][tstrand].append(int(tpos))
    return {c: {s: np.array(sorted(set(v)), np.int64) for s, v in d.items()} for c, d in out.items()}


class SiteLists:
    """moptions['fulmodlist'] / ['anymodlist'] / ['nomodlist'] behind one dm_xysites handle.  contigs: the names the alignments can carry."""

    def __init__(self, contigs, ful, anym=None, nom=None):
        self._lib = _lib.load()
        self.contigs = list(contigs)
        for d in (ful, anym, nom):
            self.contigs += [c for c in (d or {}) if c not in self.contigs]
        self.index = {c: i for i, c in enumerate(self.contigs)}
        self.lists = (ful, anym, nom)
        self.h = self._lib.dm_xy_sites_create(max(len(self.contigs), 1), int(anym is not None), int(nom is not None))
        if not self.h:
            raise _lib.DeepModHipError("dm_xy_sites_create: " + _lib.last_error())
        for kind, d in enumerate(self.lists):
            for c, per in (d or {}).items():
                for strand, arr in per.items():
                    arr = np.ascontiguousarray(arr, np.int64)
                    _lib.check(self._lib.dm_xy_sites_set(self.h, self.index[c], 0 if strand == '+' else 1, kind, arr.ctypes.data, len(arr)))

    def close(self):
        if self.h:
            self._lib.dm_xy_sites_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------ the device stage, stated in numpy
def row_starts(rdesc, n_rows):
    return np.concatenate([np.asarray(rdesc, np.int64).reshape(-1, 4)[:, 0], [n_rows]]).astype(np.int64)


def xy_keep_np(lab, rdesc):
    """:512-526 for the reads of a batch: keep [n_rows] (1 = the row is written) and read_row_off [reads + 1].  A row is kept if a labelled row of its
    read lies within +-25 rows; more than 0.9 of a read's rows kept: all of them (the reference's float comparison); none: nothing."""
    lab = np.asarray(lab)
    off = row_starts(rdesc, len(lab))
    keep = np.zeros(len(lab), np.uint8)
    counts = []
    for r0, r1 in zip(off[:-1], off[1:]):
        n = int(r1 - r0)
        d = np.zeros(n + 1, np.int64)
        idx = np.flatnonzero(lab[r0:r1] != 0)
        np.add.at(d, np.maximum(idx - NEIGHBOURS, 0), 1)
        np.add.at(d, np.minimum(idx + NEIGHBOURS, n - 1) + 1, -1)
        k = np.cumsum(d)[:n] > 0
        kept = int(k.sum())
        if kept > 0 and kept > n * 0.9:
            k[:] = True
        keep[r0:r1] = k
        counts.append(int(k.sum()))
    return keep, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def xy_matrix_np(pos, lab, code, rdesc, ev3):
    """get_Feature's matrix [n_rows][10] of a batch from its device form: ev3 [n_events][3] float32 = (mean, stdv, length) of the batch's events."""
    pos, lab, code = np.asarray(pos, np.int64), np.asarray(lab), np.asarray(code)
    rdesc = np.asarray(rdesc, np.int64).reshape(-1, 4)
    n = len(pos)
    off = row_starts(rdesc, n)
    m = np.zeros((n, 10))
    m[:, 0] = pos
    m[:, 1] = lab == 1
    m[:, 2] = lab == 2
    for c in range(4):
        m[:, 3 + c] = code == c
    ev3 = np.asarray(ev3, np.float32).reshape(-1, 3)
    for r, (r0, r1) in enumerate(zip(off[:-1], off[1:])):
        e = np.arange(r0, r1) + rdesc[r, 1]
        has = (e >= rdesc[r, 2]) & (e < rdesc[r, 3])
        m[r0:r1][has, 7:10] = ev3[e[has]]
    return m


def xy_text_np(matrix) -> bytes:
    """np.savetxt(fmt='%.3f') of the rows (:123), the reference's own writer"""
    buf = io.BytesIO()
    if len(matrix):
        np.savetxt(buf, matrix, fmt='%.3f')
    return buf.getvalue()


def xy_rows_np(pos, lab, code, rdesc, ev3):
    """The whole device stage (what dm_xy_rows + dm_xy_rows_fetch return): (text, keep, read_row_off, read_byte_off)."""
    keep, row_off = xy_keep_np(lab, rdesc)
    m = xy_matrix_np(pos, lab, code, rdesc, ev3)
    off = row_starts(rdesc, len(keep))
    texts = [xy_text_np(m[r0:r1][keep[r0:r1] != 0]) for r0, r1 in zip(off[:-1], off[1:])]
    byte_off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    return b''.join(texts), keep, row_off, byte_off


def format_value_rule(v: np.float32) -> str:
    """The formatting rule of the kernels for one fp32 value below 2^30 in magnitude (csrc/xyrows.hip.inc put_value), in Python integers."""
    v = np.float32(v)
    q = int(np.rint(abs(float(v)) * 1000.0))
    return '%s%d.%03d' % ('-' if np.signbit(v) else '', q // 1000, q % 1000)


def format_host(rows) -> bytes:
    """dm_xy_format_host: the text of rows [n][10] float64"""
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 10)
    need = lib.dm_xy_format_host(rows.ctypes.data, len(rows), None, 0)
    if need < 0:
        _lib.check(int(need))
    buf = ctypes.create_string_buffer(max(int(need), 1))
    if lib.dm_xy_format_host(rows.ctypes.data, len(rows), buf, need) != need:
        raise _lib.DeepModHipError('dm_xy_format_host: ' + _lib.last_error())
    return buf.raw[:need]


class XYRows:
    """One dm_xyrows handle: the device stage of a batch on a GPU."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        self._h = self._lib.dm_xy_create(device)
        if not self._h:
            raise _lib.DeepModHipError("dm_xy_create: " + _lib.last_error())

    def close(self):
        if self._h:
            self._lib.dm_xy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rows(self, pos, lab, code, rdesc, ev3_ptr: int, n_events: int, want_keep: bool = False):
        """-> (text bytes, keep or None, read_row_off, read_byte_off, flag)"""
        pos, lab, code = np.ascontiguousarray(pos, np.int64), np.ascontiguousarray(lab, np.uint8), np.ascontiguousarray(code, np.uint8)
        rdesc = np.ascontiguousarray(rdesc, np.int64).reshape(-1, 4)
        if not (len(pos) == len(lab) == len(code)):
            raise ValueError('pos, lab and code of different lengths')
        flag = ctypes.c_int32(0)
        total = self._lib.dm_xy_rows(self._h, pos.ctypes.data, lab.ctypes.data, code.ctypes.data, rdesc.ctypes.data, len(rdesc), len(pos), ev3_ptr,
                                     n_events, ctypes.byref(flag))
        if total < 0:
            _lib.check(int(total))
        text = np.empty(max(int(total), 1), np.uint8)
        keep = np.empty(len(pos), np.uint8) if want_keep else None
        row_off, byte_off = np.empty(len(rdesc) + 1, np.int64), np.empty(len(rdesc) + 1, np.int64)
        _lib.check(self._lib.dm_xy_rows_fetch(self._h, text.ctypes.data, None if keep is None else keep.ctypes.data, row_off.ctypes.data, byte_off.ctypes.data))
        return text[:total], keep, row_off, byte_off, int(flag.value)

    def scan(self, values) -> np.ndarray:
        """dm_xy_scan: the exclusive prefix sums of int64 values and their total, by the kernels of the stage"""
        v = np.concatenate([np.asarray(values, np.int64), [0]])
        _lib.check(self._lib.dm_xy_scan(self._h, v.ctypes.data, len(v) - 1))
        return v

    def times(self):
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        _lib.check(self._lib.dm_xy_times(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


def rows_host(pos, lab, code, rdesc, ev3):
    """dm_xy_rows_host: the device stage in compiled host code, from host statistics -> (text, keep, read_row_off, read_byte_off)"""
    lib = _lib.load()
    pos, lab, code = np.ascontiguousarray(pos, np.int64), np.ascontiguousarray(lab, np.uint8), np.ascontiguousarray(code, np.uint8)
    rdesc = np.ascontiguousarray(rdesc, np.int64).reshape(-1, 4)
    ev3 = np.ascontiguousarray(ev3, np.float32).reshape(-1, 3)
    keep = np.empty(len(pos), np.uint8)
    row_off, byte_off = np.empty(len(rdesc) + 1, np.int64), np.empty(len(rdesc) + 1, np.int64)
    args = (pos.ctypes.data, lab.ctypes.data, code.ctypes.data, rdesc.ctypes.data, len(rdesc), len(pos), ev3.ctypes.data, len(ev3))
    total = lib.dm_xy_rows_host(*args, keep.ctypes.data, row_off.ctypes.data, byte_off.ctypes.data, None, 0)
    if total < 0:
        _lib.check(int(total))
    text = np.empty(max(int(total), 1), np.uint8)
    if lib.dm_xy_rows_host(*args, None, None, None, text.ctypes.data, total) != total:
        raise _lib.DeepModHipError('dm_xy_rows_host: ' + _lib.last_error())
    return text[:total].tobytes(), keep, row_off, byte_off


# ------------------------------------------------------------------------------------------------ per read: walk + labels (compiled)
def _motif_args(moptions):
    if 'motif' in moptions and moptions['motif'] is not None:
        return moptions['motif'][0].encode('ascii'), int(moptions['motif'][1])
    return None, 0


def walk_read(moptions, sites: SiteLists, rname, flag, pos1, cigar, readseq, ref_bytes, n_events, row0=0, ev0=0):
    """dm_xy_read for one alignment record -> {'status', 'pos', 'lab', 'code', 'rdesc', 'strand', 'start_clip', 'end_clip'}"""
    lib = _lib.load()
    motif, mpos = _motif_args(moptions)
    cap = int(n_events) + 200
    pos, lab, code = np.empty(cap, np.int64), np.empty(cap, np.uint8), np.empty(cap, np.uint8)
    rdesc = np.zeros(4, np.int64)
    info = (ctypes.c_int64 * _lib.DM_XY_INFO_LEN)()
    seq_b = readseq.encode('ascii') if isinstance(readseq, str) else readseq
    _lib.check(lib.dm_xy_read(sites.h, sites.index[rname], int(flag), int(pos1), cigar.encode('ascii'), seq_b, len(seq_b), ref_bytes, len(ref_bytes),
                              int(n_events), motif, mpos, int(moptions['posneg']), pos.ctypes.data, lab.ctypes.data, code.ctypes.data, cap, int(row0), int(ev0),
                              rdesc.ctypes.data, info))
    n = int(info[_lib.DM_XY_N_ROWS]) if info[_lib.DM_XY_STATUS] == _lib.DM_XY_OK else 0
    return {'status': int(info[_lib.DM_XY_STATUS]), 'pos': pos[:n], 'lab': lab[:n], 'code': code[:n], 'rdesc': rdesc,
            'strand': '-' if info[_lib.DM_XY_STRAND] else '+', 'start_clip': int(info[_lib.DM_XY_START_CLIP]), 'end_clip': int(info[_lib.DM_XY_END_CLIP]),
            'pos_after_clip': int(info[_lib.DM_XY_POS_AFTER_CLIP]), 'events_after_clip': int(info[_lib.DM_XY_EVENTS_AFTER_CLIP])}


def _event_block(modevents) -> np.ndarray:
    """(mean, stdv, length) of a read's events as the float32 block the signal stage leaves on the device"""
    ev3 = np.empty((len(modevents), 3), np.float32)
    ev3[:, 0], ev3[:, 1], ev3[:, 2] = modevents['mean'], modevents['stdv'], modevents['length']
    return ev3


def get_Feature(moptions, sp_options, sp_param, f5align, f5data, readk, start_clip, end_clip, base_map_info, forward_reverse, rname, mapped_start_pos,
                num_insertions, num_deletions):
    """(mfeatures, isdif) of :355-528 for an alignment table the caller has: the KEPT rows [k][10] (an empty list if none is kept)."""
    lib = _lib.load()
    sites: SiteLists = moptions['sites']
    modevents = sp_param['f5data'][readk][1]
    motif, mpos = _motif_args(moptions)
    refb = np.ascontiguousarray(np.char.encode(base_map_info['refbase'], 'ascii'))
    readb = np.ascontiguousarray(np.char.encode(base_map_info['readbase'], 'ascii'))
    refi = np.ascontiguousarray(base_map_info['refbasei'], np.uint64)
    cap = len(modevents) + 200
    pos, lab, code = np.empty(cap, np.int64), np.empty(cap, np.uint8), np.empty(cap, np.uint8)
    rdesc = np.zeros(4, np.int64)
    info = (ctypes.c_int64 * _lib.DM_XY_INFO_LEN)()
    _lib.check(lib.dm_xy_labels(sites.h, sites.index[rname], 0 if forward_reverse == '+' else 1, motif, mpos, int(moptions['posneg']), refb.ctypes.data,
                                readb.ctypes.data, refi.ctypes.data, len(refi), len(modevents), int(start_clip), int(end_clip), int(mapped_start_pos),
                                int(num_insertions), pos.ctypes.data, lab.ctypes.data, code.ctypes.data, cap, 0, 0, rdesc.ctypes.data, info))
    if info[_lib.DM_XY_STATUS] != _lib.DM_XY_OK:
        raise IndexError('alignment table with fewer bases than aligned events (status %d)' % info[_lib.DM_XY_STATUS])
    n = int(info[_lib.DM_XY_N_ROWS])
    aligned = np.flatnonzero(base_map_info['readbase'] != '-')[:n - 200]
    from .rawreads import event_bases
    isdif = bool((base_map_info['readbase'][aligned] != event_bases(modevents['model_state'][start_clip:start_clip + len(aligned)])).any())
    keep, _ = xy_keep_np(lab[:n], rdesc)
    m = xy_matrix_np(pos[:n], lab[:n], code[:n], rdesc, _event_block(modevents))
    kept = m[keep != 0]
    return (kept if len(kept) else []), isdif


# ------------------------------------------------------------------------------------------------ the files
class XYWriter:
    """<ctfolder>/<k>.xy.gz and <k>.xy.ind (:119-130, :340-350): the kept rows of consecutive reads; a new file begins before the next read once
    the rows so far exceed size_per_batch bytes at 80 bytes per row.  With a pool the gzip + write of a finished file runs on a host thread."""

    def __init__(self, ctfolder: str, size_per_batch: float, pool: Optional[ThreadPoolExecutor] = None, times: Optional[Dict[str, float]] = None):
        self.ctfolder, self.size, self.pool, self.times = ctfolder, size_per_batch, pool, times
        self.index, self.entries, self.chunks, self.rows, self.jobs = 0, [], [], 0, []

    def add(self, src: str, n_rows: int, text) -> None:
        if n_rows <= 0:
            return
        if self.entries and self.rows * ROW_BYTES > self.size:
            self.flush()
        self.entries.append((src, self.rows))
        self.chunks.append(text)
        self.rows += n_rows

    def _store(self, base: str, chunks, entries):
        t0 = time.perf_counter()
        co = zlib.compressobj(GZIP_LEVEL, zlib.DEFLATED, 31)                 # wbits 31: a gzip container
        data = b''.join([co.compress(c) for c in chunks] + [co.flush()])
        t1 = time.perf_counter()
        with open(base + '.xy.gz', 'wb') as fh:
            fh.write(data)
        with open(base + '.xy.ind', 'w') as fh:
            for src, first in entries:
                fh.write('%d %s\n' % (first, src))
        return t1 - t0, time.perf_counter() - t1

    def flush(self) -> None:
        if not self.entries:
            return
        args = (os.path.join(self.ctfolder, str(self.index)), self.chunks, self.entries)
        self.jobs.append(self.pool.submit(self._store, *args) if self.pool is not None else self._store(*args))
        self.index, self.entries, self.chunks, self.rows = self.index + 1, [], [], 0

    def close(self) -> None:
        self.flush()
        for j in self.jobs:
            gz, wr = j.result() if self.pool is not None else j
            if self.times is not None:                                       # summed over the host threads
                self.times['gzip'] = self.times.get('gzip', 0.0) + gz
                self.times['write'] = self.times.get('write', 0.0) + wr
        self.jobs = []


def _in_region(moptions, rname) -> bool:
    return moptions.get('region', [None, None, None])[0] in ('', None, rname)


def _reference_bytes(moptions, sp_param, rname):
    """sp_param['ref_info'][rname] as ASCII bytes (getRefSeq of the reference; here the FASTA readFA already holds)"""
    cache = sp_param.setdefault('ref_bytes', {})
    if rname not in cache:
        if rname not in sp_param['ref_info']:
            fa = moptions.get('fadict')
            if fa is None or rname not in fa:
                return None
            sp_param['ref_info'][rname] = fa[rname]
        cache[rname] = sp_param['ref_info'][rname].encode('ascii')
    return cache[rname]


def handle_record(moptions, sp_options, sp_param, f5align, f5data):
    """The per-read path of :109-350: every alignment record of f5align, in its order, through the compiled walk and the numpy statement of the
    device stage, into the files of sp_options['ctfolder']."""
    sites: SiteLists = moptions['sites']
    writer = XYWriter(sp_options['ctfolder'], moptions['size_per_batch'])
    for readk in list(f5align.keys()):
        mapq, flag, rname, pos, cigar, readseq = f5align[readk]
        if rname not in sites.index or not _in_region(moptions, rname):
            continue
        ref_b = _reference_bytes(moptions, sp_param, rname)
        if ref_b is None:
            sp_options["Error"]["No reference sequence"].append(f5data[readk][3])
            continue
        modevents = f5data[readk][1]
        try:
            w = walk_read(moptions, sites, rname, flag, pos, cigar, readseq, ref_b, len(modevents))
        except _lib.DeepModHipError as exc:
            sp_options["Error"]["CIGAR-Error: %s" % exc].append(f5data[readk][3])
            continue
        if w['status'] in XY_ERRORS:
            sp_options["Error"][XY_ERRORS[w['status']]].append(f5data[readk][3])
        if w['status'] != _lib.DM_XY_OK:
            continue
        text, keep, row_off, _ = xy_rows_np(w['pos'], w['lab'], w['code'], w['rdesc'], _event_block(modevents))
        writer.add(f5data[readk][3], int(row_off[-1]), text)
    writer.close()


# ------------------------------------------------------------------------------------------------ the command: one batch on the GPU
class _Batch:
    """The reads of a worker batch that have events: ids / src per read, samples and event tables back to back (signal.py's layout)."""

    def __init__(self):
        self.ids, self.src, self.raw, self.bases = [], [], [], []
        self.start, self.length, self.fb_mean, self.fb_stdv = [], [], [], []          # event tables
        self.move, self.first = [], []                                               # move tables

    @staticmethod
    def offsets(parts):
        return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def _load_event_container(lib, f5f, batch: _Batch, errors) -> None:
    """getEvent's merge (dm_events_merge, rawreads.py) for the reads of one container with event tables"""
    from . import batch as dmbatch
    c = dmbatch._open_event_container(f5f)
    mev_off = np.empty(c.n + 1, np.int64)
    cap = max(c.n_ev, 1)
    mean, stdv = np.empty(cap, np.float32), np.empty(cap, np.float32)
    start, length, base = np.empty(cap, np.uint64), np.empty(cap, np.uint64), np.empty(cap, 'S1')
    got = lib.dm_events_merge(*dmbatch._merge_args(c, mev_off), mean.ctypes.data, stdv.ctypes.data, start.ctypes.data, length.ctypes.data, base.ctypes.data)
    if got < 0:
        raise ValueError('event offsets of a damaged container')
    for i, m in enumerate(c.meta):
        lo, hi = int(mev_off[i]), int(mev_off[i + 1])
        if hi == lo:
            errors['No events data'].append(f5f)
            continue
        batch.ids.append(m['read_id'].replace(" ", ":::").replace("\t", "|||"))
        batch.src.append(f5f)
        batch.raw.append(np.asarray(c.z['raw'][int(c.raw_off[i]):int(c.raw_off[i + 1])]))
        batch.bases.append(base[lo:hi])
        batch.start.append(start[lo:hi])
        batch.length.append(length[lo:hi])
        batch.fb_mean.append(mean[lo:hi])
        batch.fb_stdv.append(stdv[lo:hi])


def _load_move_container(lib, f5f, batch: _Batch, errors) -> None:
    from . import batch as dmbatch
    c = dmbatch._open_move_container(f5f)
    if c.mv is None:
        errors['No move data'].extend([f5f] * c.n)
        return
    if c.n and (int(c.mv_off[-1]) > len(c.mv) or int(c.fq_off[-1]) > len(c.fq) or (np.diff(c.mv_off) < 0).any() or (np.diff(c.fq_off) < 0).any()):
        raise ValueError('move offsets of a damaged container')
    for i, m in enumerate(c.meta):
        batch.ids.append(m['read_id'].replace(" ", ":::").replace("\t", "|||"))
        batch.src.append(f5f)
        batch.raw.append(np.asarray(c.z['raw'][int(c.raw_off[i]):int(c.raw_off[i + 1])]))
        batch.bases.append(c.fq[int(c.fq_off[i]):int(c.fq_off[i + 1])].view('S1'))
        batch.move.append(c.mv[int(c.mv_off[i]):int(c.mv_off[i + 1])])
        batch.first.append(int(c.first[i]))


def _drop_unplannable(lib, sp_options, batch: _Batch) -> None:
    """Event tables come from files: a read whose events cover no signal (dm_signal_plan_batch refuses it, and with it a whole batch) is reported and
    leaves the batch before the signal stage sees it."""
    keep = []
    for i in range(len(batch.ids)):
        raw_off, ev_off = np.array([0, len(batch.raw[i])], np.int64), np.array([0, len(batch.start[i])], np.int64)
        st, ln = np.ascontiguousarray(batch.start[i], np.uint64), np.ascontiguousarray(batch.length[i], np.uint64)
        fe = np.empty(1, np.int64)
        if lib.dm_signal_plan_batch(1, raw_off.ctypes.data, ev_off.ctypes.data, st.ctypes.data, ln.ctypes.data, fe.ctypes.data) == 0:
            keep.append(i)
        else:
            sp_options["Error"]["Cannot open fast5 or other errors"].append(batch.src[i])
            print("Cannot open fast5 or other errors: {} ({})".format(batch.src[i], _lib.last_error()))
    for name in ('ids', 'src', 'raw', 'bases', 'start', 'length', 'fb_mean', 'fb_stdv'):
        setattr(batch, name, [getattr(batch, name)[i] for i in keep])


def _signal_stage(moptions, sp_options, batch: _Batch, normalizer, device: int):
    """The statistics of the batch's events into a device block -> (block, ev_off, usable events per read; 0 = the read failed)"""
    from .model import DeviceArray
    ev_off = _Batch.offsets(batch.bases)
    raw, raw_off = np.concatenate(batch.raw), _Batch.offsets(batch.raw)
    block = DeviceArray((max(int(ev_off[-1]), 1), 3), np.float32, device)
    per_read = np.diff(ev_off)
    try:
        if moptions.get('move'):
            status, _ = normalizer.move_stats_device(raw, raw_off, np.concatenate(batch.move), _Batch.offsets(batch.move), np.array(batch.first, np.int64),
                                                     ev_off, block.ptr)
            usable = np.where(status == 0, per_read, 0)
        else:
            first_empty, _ = normalizer.event_stats_device(raw, raw_off, np.concatenate(batch.start), np.concatenate(batch.length), ev_off, block.ptr,
                                                           np.concatenate(batch.fb_mean), np.concatenate(batch.fb_stdv))
            # :337-340 of myDetect: the statistics loop stops at an empty event; behind event 500 the table is cut in front of it
            usable = np.where((first_empty < per_read) & (first_empty > 500), first_empty - 1, per_read)
    except _lib.DeepModHipError:
        block.free()
        raise
    for i in np.flatnonzero(usable == 0):
        sp_options["Error"]["Cannot open fast5 or other errors"].append(batch.src[i])
    return block, ev_off, usable


def mGetFeature1(moptions, sp_options, f5files):
    """One worker batch on the GPU (:28-103): containers -> events -> signal statistics (resident) -> alignment records -> labelled rows (compiled
    walk on the host threads) -> row selection and text (dm_xy_rows) -> the files of sp_options['ctfolder']."""
    from . import detect, readmap, signal as dm_signal
    lib = _lib.load()
    times = sp_options.setdefault('times', {})
    pool: ThreadPoolExecutor = sp_options['pool']
    device = int(moptions.get('device', 0))
    errors = sp_options["Error"]
    clock = time.perf_counter
    t0 = clock()

    def load(f5f):
        part, errs = _Batch(), defaultdict(list)
        try:
            (_load_move_container if moptions.get('move') else _load_event_container)(lib, f5f, part, errs)
        except Exception:
            errs = defaultdict(list, {"Cannot open fast5 or other errors": [f5f]})
            print("Cannot open fast5 or other errors: {}".format(f5f))
            part = _Batch()
        return part, errs
    batch = _Batch()
    for part, errs in pool.map(load, f5files):
        for k, v in errs.items():
            errors[k].extend(v)
        for name in ('ids', 'src', 'raw', 'bases', 'start', 'length', 'fb_mean', 'fb_stdv', 'move', 'first'):
            getattr(batch, name).extend(getattr(part, name))
    times['load'] = times.get('load', 0.0) + clock() - t0
    if not moptions.get('move'):
        _drop_unplannable(lib, sp_options, batch)
    if not batch.ids:
        return
    t0 = clock()
    normalizer = sp_options.get('normalizer') or sp_options.setdefault('normalizer', dm_signal.SignalNormalizer(device))
    block, ev_off, usable = _signal_stage(moptions, sp_options, batch, normalizer, device)
    times['signal'] = times.get('signal', 0.0) + clock() - t0
    try:
        t0 = clock()
        f5data = {}
        for i, rid in enumerate(batch.ids):
            if usable[i] == 0:
                continue
            if rid in f5data:
                print('Duplicate id', rid, batch.src[i])
            f5data[rid] = (batch.bases[i].tobytes().decode('ascii', 'replace'), i, None, batch.src[i], (0, 0))
        align_info = detect._alignment_lines(moptions, sp_options, f5files, f5data)
        if align_info is None:
            for f5k in sorted(f5data.keys()):
                errors["Cannot running aligment"].append(f5data[f5k][3])
            return
        sp_param = {'f5data': f5data, 'ref_info': {}, 'f5status': "", 'line': ""}
        f5align = readmap.parse_sam(moptions, sp_options, sp_param, align_info, f5data)
        times['align'] = times.get('align', 0.0) + clock() - t0
        t0 = clock()
        sites: SiteLists = moptions['sites']

        def walk(readk):
            mapq, flag, rname, pos, cigar, readseq = f5align[readk]
            i = f5data[readk][1]
            if rname not in sites.index or not _in_region(moptions, rname):
                return readk, None, None
            ref_b = moptions['ref_bytes'].get(rname)
            if ref_b is None:
                return readk, "No reference sequence", None
            try:
                w = walk_read(moptions, sites, rname, flag, pos, cigar, readseq, ref_b, int(usable[i]), 0, int(ev_off[i]))
            except _lib.DeepModHipError as exc:
                return readk, "CIGAR-Error: %s" % exc, None
            return readk, XY_ERRORS.get(w['status']), (w if w['status'] == _lib.DM_XY_OK else None)
        walked = []
        for readk, err, w in pool.map(walk, list(f5align.keys())):
            if err is not None:
                errors[err].append(f5data[readk][3])
            if w is not None:
                walked.append((readk, w))
        times['walk'] = times.get('walk', 0.0) + clock() - t0
        if not walked:
            return
        row0 = _Batch.offsets([w['pos'] for _, w in walked])
        rdesc = np.stack([w['rdesc'] for _, w in walked])
        rdesc[:, 0] += row0[:-1]                    # the walk numbered every read's rows from 0
        rdesc[:, 1] -= row0[:-1]
        pos, lab, code = (np.concatenate([w[k] for _, w in walked]) for k in ('pos', 'lab', 'code'))
        t0 = clock()
        xy = sp_options.get('xyrows') or sp_options.setdefault('xyrows', XYRows(device))
        text, _, row_off, byte_off, flag = xy.rows(pos, lab, code, rdesc, block.ptr, int(ev_off[-1]))
        t1 = clock()
        keep_ms, text_ms = xy.times()
        times['xy_keep'] = times.get('xy_keep', 0.0) + keep_ms / 1e3
        times['xy_text'] = times.get('xy_text', 0.0) + text_ms / 1e3
        times['download'] = times.get('download', 0.0) + max(t1 - t0 - (keep_ms + text_ms) / 1e3, 0.0)      # uploads, the host's checks and the D2H copies of the call
        times['host_text_batches'] = times.get('host_text_batches', 0) + flag
        writer = XYWriter(sp_options['ctfolder'], moptions['size_per_batch'], pool, times)
        view = memoryview(text)
        for k, (readk, _) in enumerate(walked):
            writer.add(f5data[readk][3], int(row_off[k + 1] - row_off[k]), view[int(byte_off[k]):int(byte_off[k + 1])])
        writer.close()
    finally:
        block.free()


def getFeature_handler(moptions, h5files_Q, failed_Q, version_Q=None):
    """The worker of :564-583: batches (files, folder id) from the list h5files_Q, errors appended to the list failed_Q."""
    pool = ThreadPoolExecutor(max(int(moptions['threads']), 1))
    shared = {}
    try:
        for f5files, ctfolderid in h5files_Q:
            sp_options = defaultdict()
            sp_options.update(shared)
            sp_options['ctfolder'] = moptions['outFolder'] + str(ctfolderid)
            sp_options['Error'] = defaultdict(list)
            sp_options['pool'] = pool
            sp_options['times'] = moptions.setdefault('times', {})
            os.makedirs(sp_options['ctfolder'], exist_ok=True)
            mGetFeature1(moptions, sp_options, f5files)
            shared = {k: sp_options[k] for k in ('normalizer', 'xyrows') if k in sp_options}
            for errtype, errfiles in sp_options["Error"].items():
                failed_Q.append((errtype, errfiles))
    finally:
        pool.shutdown()
        for h in shared.values():
            h.close()


def position_lists(moptions, fadict) -> SiteLists:
    """moptions['fulmodlist'] / ['anymodlist'] / ['nomodlist'] of :668-701"""
    if moptions['motifORPos'] == 1:
        ful, _ = readMotifMod(fadict, moptions['motif'][0], moptions['motif'][1], moptions['region'][0], moptions['region'][1], moptions['region'][2])
        anym = nom = None
    else:
        ful, anym, nom = (readPosFiles(moptions[k], fadict) for k in ('fulmod', 'anymod', 'nomod'))
    for tchr in (ful if anym is None else anym):
        nf = sum(len(v) for v in ful.get(tchr, {}).values())
        na = -1 if anym is None else sum(len(v) for v in anym.get(tchr, {}).values())
        if nf > 0 or na > 0:
            print('%s fulmod=%d anymod=%d nomod=%d' % (tchr, nf, na, -1 if nom is None else sum(len(v) for v in nom.get(tchr, {}).values())))
    return SiteLists(list(fadict.keys()), ful, anym, nom)


def existing_output(out_folder: str) -> List[str]:
    return sorted(glob.glob(os.path.join(out_folder, '*', '*.xy.gz')))


def getFeature_manager(moptions):
    """:653-757 on one GPU."""
    from . import detect, rawreads
    start_time = time.time()
    if existing_output(moptions['outFolder']):
        raise SystemExit('Error: getfeatures: --outFolder %s already holds */*.xy.gz files (the reference deletes the folder; this build does not)' % moptions['outFolder'])
    if _lib.load().dm_device_count() < 1:
        raise SystemExit('Error: no gfx950 GPU visible (this build has no CPU path)')
    os.makedirs(moptions['outFolder'], exist_ok=True)
    moptions['size_per_batch'] = moptions['size_per_batch'] * (10 ** 7)
    fadict = readFA(moptions['Ref'], moptions['region'][0])
    moptions['fadict'] = fadict
    moptions['ref_bytes'] = {c: s.encode('ascii') for c, s in fadict.items()}
    moptions['sites'] = position_lists(moptions, fadict)
    f5files = [f for f in detect.discover_inputs(moptions['wrkBase'], moptions['recursive'] == 1) if f.endswith(rawreads.RAW_SUFFIX)]
    print('Total files=%d' % len(f5files))
    per = moptions['files_per_thread']
    batches = [(f5files[i:i + per], i // per) for i in range(0, len(f5files), per)]
    failed: List = []
    try:
        getFeature_handler(moptions, batches, failed)
    finally:
        moptions['sites'].close()
    failed_files = defaultdict(list)
    for errk, fns in failed:
        failed_files[errk].extend(fns)
    if len(failed_files) > 0:
        print('Error information for different fast5 files:')
        for errtype, errfiles in failed_files.items():
            print('\t%s %d' % (errtype, len(errfiles)))
    sys.stdout.flush()
    print("Total consuming time %d" % (time.time() - start_time))
    return failed_files
