"""The batch builder of the streaming detect: the host side of one worker batch, file list -> `Prepared` (deepmod_amd/stream.py has the overview of
the path).  It runs in feeder threads and feeder processes and never touches the device itself: the signal stage is reached through the normalizer
it is given.  `prepare_batch` is the entry; `_prepare_batch_c` does the per-read work behind the C ABI in named stages, `_prepare_batch_py` is the
per-read restatement the tests compare it with."""
from __future__ import annotations

import contextlib
import ctypes
import json
import os
import time
from collections import defaultdict, namedtuple
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np

from . import predstore, rawreads

PAD = 100          # zero-padded feature rows on both sides of a read (myDetect.py:850-851)
HALF = 10          # windowsize // 2


class Prepared:
    """One worker batch, ready for the device.  Rows of the reads are concatenated, reads grouped by (contig, strand)."""
    __slots__ = ('_rows', 'pos', 'flags', 'n_rows', 'groups', 'n_windows', 'n_reads', 'errors', 'contig_len', 'timing', 'files', 'on_done', 'f32', 'sel',
                 'ev3', 'code', 'rdesc', 'sig')

    @property
    def rows(self):
        """Feature rows [n_rows][7].  A batch in the device form (ev3 / code / rdesc, see below) has none on the host: a consumer that asks
        for them anyway (the CPU backend of the tests, a comparison) gets the host restatement of dm_rows_assemble."""
        if self._rows is None and self.ev3 is not None:
            return assemble_rows(self.ev3, self.code, self.rdesc, self.n_rows)
        if self._rows is None and self.sig is not None:
            raise ValueError('the event statistics of this batch stay on the device (resident form): its feature rows exist only there')
        return self._rows

    @rows.setter
    def rows(self, value):
        self._rows = value

    def __init__(self):
        self._rows = np.zeros((0, 7), np.float32)
        # device form of a batch of raw reads (round 5, rowsbatch.inc dm_rows_emit_device): ev3 f32[E][3] = (mean, stdv, length) of the events the rows
        # show, code u8[n_rows] = one-hot class of a row (255: none), rdesc i64[reads][4] = (first row, row -> event shift, first event, end event);
        # `rows` is then built on the device (HipBackend.submit -> dm_rows_assemble): 13 instead of 28 bytes per row cross the host and PCIe
        self.ev3 = self.code = self.rdesc = None
        # resident form (round 6): sig = (feeder, request number) of the signal request whose statistics block - (mean, stdv, length) of every merged event
        # of the batch, written by dm_signal_event_stats_device - stays on the device; code / rdesc as above, rdesc's event indices point into that block
        self.sig = None
        self.pos = np.zeros(0, np.int64)          # [n_rows classified rows | extra rows]
        self.flags = np.zeros(0, np.uint8)
        self.n_rows = 0
        self.groups: List[Tuple] = []   # (chr, strand, row_lo, row_hi, extra_lo, extra_hi[, sel_lo, sel_hi])
        # compact form (the compiled path's default): sel = int32 feature-row indices of the windows centred on a base of interest -
        # the only ones whose class can reach the BED (myDetect.py:1091); pos / flags then hold [len(sel) | extras] entries and
        # groups carry (sel_lo, sel_hi).  None: classic form, pos / flags hold one entry per feature row and every window is classified.
        self.sel = None
        self.n_windows = 0
        self.n_reads = 0
        self.errors: Dict[str, List[str]] = defaultdict(list)
        self.contig_len: Dict[str, int] = {}
        self.timing: Dict[str, float] = defaultdict(float)
        self.files: List[str] = []
        self.f32 = False             # a feature outside the split-f16 kernel's range (or NaN): this batch runs the fp32 kernel
        self.on_done = None          # called once the device has consumed the host arrays (a feeder slot goes back to its queue)


def assemble_rows(ev3: np.ndarray, code: np.ndarray, rdesc: np.ndarray, n_rows: int) -> np.ndarray:
    """Host restatement of dm_rows_assemble (deepmod_hip.hip rows_assemble_kernel): the device form of a raw batch -> rows [n_rows][7] =
    one-hot of the row's reference base | mean, stdv, length of the event it shows (get_Feature, myDetect.py:839-903)."""
    rows = np.zeros((n_rows, 7), np.float32)
    if n_rows == 0:
        return rows
    code = np.asarray(code[:n_rows])
    for c in range(4):
        rows[code == c, c] = 1.0
    rdesc = np.asarray(rdesc, np.int64).reshape(-1, 4)
    q = np.arange(n_rows, dtype=np.int64)
    r = np.searchsorted(rdesc[:, 0], q, side='right') - 1          # the last read whose first row is <= q
    e = q + rdesc[r, 1]
    has = (e >= rdesc[r, 2]) & (e < rdesc[r, 3])
    rows[has, 4:7] = np.asarray(ev3, np.float32).reshape(-1, 3)[e[has]]
    return rows


def rows_from_packed(pk: Dict, base: str, src: str, out: Prepared) -> None:
    """Packed container arrays -> device-ready rows, appended to `out` as per-read pieces (see `finish`).
    Vectorised over all reads of the container.  Per read (arguments of the reference's mPredict1, myDetect.py:787-834):
    the k-th aligned event (k < n = events - clips) is the k-th table row whose readbase is not '-' and its window is
    centred on feature row 100 + k; sum_handler (:1089-1100) then counts, for table rows with refbase == Base:
    touch, cov if readbase != '-', mod if that row was classified 1."""
    ro, bo, eo = pk['row_off'], pk['bmi_off'], pk['ev_off']
    nreads = len(pk['reads'])
    if nreads == 0:
        return
    meta = pk['reads']
    start_clip = np.array([m['start_clip'] for m in meta], np.int64)
    end_clip = np.array([m['end_clip'] for m in meta], np.int64)
    # clips come from a container's metadata: classified BEFORE any arithmetic with them (values near the ends of int64 would wrap the
    # subtraction into a plausible count) - negative: an index error of the ledger; too large for the read: no aligned event = "Less Event"
    # (the same rule as rowsbatch.inc plan_read: the ledger keys of the two build paths agree)
    nev = eo[1:] - eo[:-1]
    clip_neg = (start_clip < 0) | (end_clip < 0)
    clip_over = ~clip_neg & ((start_clip > nev) | (end_clip > nev - np.minimum(start_clip, nev)))
    start_clip = np.where(clip_neg | clip_over, 0, start_clip)
    end_clip = np.where(clip_neg | clip_over, 0, end_clip)
    n_al = np.where(clip_neg | clip_over, 0, nev - start_clip - end_clip)     # aligned events per read
    readb, refb, refi = pk['readbase'], pk['refbase'], pk['refbasei']
    not_gap = readb != b'-'
    is_base = refb == base.encode('ascii')                                # Base is one of ACGT: never '-', 'N', 'n'
    cnt = np.cumsum(not_gap, dtype=np.int64)
    excl = np.append(cnt - not_gap, cnt[-1] if len(cnt) else 0)          # aligned rows before row j (whole container); [B] = total
    read_of = np.repeat(np.arange(nreads), bo[1:] - bo[:-1])
    first_cnt = excl[bo[:-1]]
    k = excl[:-1] - first_cnt[read_of]                                     # rank of an aligned row within its read
    n_have = excl[bo[1:]] - first_cnt                                      # aligned table rows per read
    ok = (n_al >= 50) & (n_have >= n_al) & ((ro[1:] - ro[:-1]) == n_al + 2 * PAD)
    for i in np.flatnonzero(~ok):
        if clip_neg[i]:
            out.errors["Prediction failed: IndexError"].append(src)
        elif n_al[i] < 50:
            out.errors["Less Event"].append(src)                          # myDetect.py:702-705
        else:
            out.errors["Prediction failed: IndexError"].append(src)       # fewer aligned table rows than aligned events
    # event base vs table base of every aligned row (the reference prints and goes on, :826-828)
    ev_base = pk['evbase']
    sel = not_gap & (k < n_al[read_of]) & ok[read_of]
    ev_idx = eo[:-1][read_of] + start_clip[read_of] + k
    bad = np.flatnonzero(sel & (ev_base[np.minimum(ev_idx, max(len(ev_base) - 1, 0))] != readb)) if len(ev_base) else []
    for j in bad[:20]:
        print('Error Does not match', readb[j].decode(), ev_base[ev_idx[j]].decode(), int(j - bo[read_of[j]]), int(k[j] + start_clip[read_of[j]]))
    nrows = len(pk['tx'])
    pos_row = np.zeros(nrows, np.int64)
    flag_row = np.zeros(nrows, np.uint8)
    dst = ro[:-1][read_of] + PAD + k
    pos_row[dst[sel]] = refi[sel]
    flag_row[dst[sel]] = is_base[sel].astype(np.uint8) | np.uint8(2)
    extra = is_base & ~sel & ok[read_of]                                   # deletion rows (and aligned rows past n): no window
    ex_idx = np.flatnonzero(extra)
    ex_read = read_of[ex_idx]
    ex_flag = np.uint8(1) | (not_gap[ex_idx].astype(np.uint8) << 1)
    ex_off = np.searchsorted(ex_read, np.arange(nreads + 1))
    for i in np.flatnonzero(ok):
        m = meta[i]
        out._pieces.append((m['chr'], m['strand'], pk['tx'][ro[i]:ro[i + 1]], pos_row[ro[i]:ro[i + 1]], flag_row[ro[i]:ro[i + 1]],
                            refi[ex_idx[ex_off[i]:ex_off[i + 1]]], ex_flag[ex_off[i]:ex_off[i + 1]], int(n_al[i])))
    for c, ln in pk.get('contig_len', {}).items():
        out.contig_len[c] = max(out.contig_len.get(c, 0), int(ln))


def rows_from_reads(reads: Iterable[Dict], base: str, src: str, out: Prepared) -> None:
    """Classic read dicts (mfeatures, base_map_info, events, clips: what readmap.map_records and the format-1 feature
    containers produce) -> the same pieces, through the packed layout."""
    reads = list(reads)
    if not reads:
        return
    tx, refb, readb, refi, evb, metas = [], [], [], [], [], []
    for rd in reads:
        bmi = rd['base_map_info']
        tx.append(np.asarray(rd['mfeatures'][:, 3:], np.float32))
        if 'table_s1' in rd:                       # reads that came through dm_map_read carry the byte columns already
            rb, qb, ri = rd['table_s1']
            refb.append(rb); readb.append(qb); refi.append(ri)
        else:
            refb.append(predstore.u1_to_s1(bmi['refbase']))
            readb.append(predstore.u1_to_s1(bmi['readbase']))
            refi.append(bmi['refbasei'].astype(np.int64))
        evb.append(predstore.u1_to_s1(rawreads.event_bases(rd['events']['model_state'])))
        metas.append(rd)
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    pk = {'tx': np.concatenate(tx), 'refbase': np.concatenate(refb), 'readbase': np.concatenate(readb),
          'refbasei': np.concatenate(refi), 'evbase': np.concatenate(evb), 'row_off': off(tx), 'bmi_off': off(refb),
          'ev_off': off(evb), 'reads': metas, 'contig_len': {}}
    rows_from_packed(pk, base, src, out)


def finish(out: Prepared, alloc=None) -> Prepared:
    """Group the collected reads by (contig, strand) and build the contiguous host arrays of the batch.
    alloc(n_rows, n_pos) -> (rows[n_rows, 7] f32, pos[n_pos] i64, flags[n_pos] u8) lets a feeder process build them directly in
    shared memory."""
    pieces = out._pieces
    order = sorted(range(len(pieces)), key=lambda i: (pieces[i][0], pieces[i][1]))
    rows, pos, flags, xpos, xflags = [], [], [], [], []
    r = x = 0
    cur = None
    for i in order:
        c, s, tx, p, f, xp, xf, n = pieces[i]
        if cur is None or (c, s) != cur[:2]:
            if cur is not None:
                out.groups.append((cur[0], cur[1], cur[2], r, cur[3], x))
            cur = (c, s, r, x)
        rows.append(tx); pos.append(p); flags.append(f); xpos.append(xp); xflags.append(xf)
        r += len(tx)
        x += len(xp)
        out.n_windows += n
        out.n_reads += 1
        if len(p):
            mx = int(max(p.max(), xp.max() if len(xp) else 0)) + 1
            if mx > out.contig_len.get(c, 0):
                out.contig_len[c] = mx            # lower bound when no reference length is known
    if cur is not None:
        out.groups.append((cur[0], cur[1], cur[2], r, cur[3], x))
    if rows and alloc is not None:
        out.rows, out.pos, out.flags = alloc(r, r + x)
        np.concatenate(rows, out=out.rows, casting='same_kind')
        np.concatenate(pos + xpos, out=out.pos, casting='same_kind')
        np.concatenate(flags + xflags, out=out.flags, casting='same_kind')
    elif rows:
        out.rows = np.ascontiguousarray(np.concatenate(rows), np.float32)
        out.pos = np.concatenate(pos + xpos)
        out.flags = np.concatenate(flags + xflags)
    out.n_rows = r
    out._pieces = []
    out.f32 = not in_f16_range(out.rows)
    return out


def in_f16_range(rows: np.ndarray) -> bool:
    """True if the split-f16 kernel takes these feature rows (include/deepmod_hip.h: |x| <= 65504; an event length may go up
    to 65504 * 2^k, but a read with an event that long is rare enough to take the fp32 kernel with the rest of its batch).
    NaN compares false: not in range."""
    if rows.size == 0:
        return True
    return bool(rows.max() <= 65504.0) and bool(rows.min() >= -65504.0)


class _PreparedBuilder(Prepared):
    __slots__ = ('_pieces',)

    def __init__(self):
        super().__init__()
        self._pieces = []


_REF_BYTES: Dict[Optional[str], Dict[str, bytes]] = {}      # reference path -> contig -> ASCII bytes (encoded once per feeder process)
_ROWS_ERRORS = {1: "Less Event", 2: "Prediction failed: IndexError", 4: "CIGAR-Error", 6: "No reference sequence", 7: "Error Does not match"}


def _c_arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _option_on(moptions, key: str) -> bool:
    """An on/off switch of the batch builder: moptions[key] wins, else DEEPMOD_<KEY> of the environment ('0' is off); on by default."""
    return bool(moptions.get(key, os.environ.get('DEEPMOD_' + key.upper(), '1') != '0'))


def _container_failed(out: Prepared, f5f: str, detail: str = '') -> None:
    """A raw container (with `detail`: one read of it) that cannot be used: one line of the ledger, one of the log; the batch goes on without it."""
    out.errors["Cannot open fast5 or other errors"].append(f5f)
    print("Cannot open fast5 or other errors: {}{}".format(f5f, detail))


class _BatchRefused(Exception):
    """The batched signal call cannot take a read of this batch (events covering no signal): the per-read Python path builds the batch and reports it."""


# the rows handle of a batch and what goes with it - keep: see _rows_handle; contigs: name -> index, srcs: source file of every read, both in the order of adding
_Rows = namedtuple('_Rows', 'lib h keep contigs srcs')


@contextlib.contextmanager
def _rows_handle(lib, base: str):
    """dm_rows_create ... dm_rows_destroy around a block, and the ONE owner of what the handle borrows: dm_rows_add_raw / dm_rows_add_packed keep the
    pointers they get until emit, so a stage appends the Python objects behind every pointer to `keep` before its add call - no array is valid between
    add and emit merely because some local is still alive.  Handle and list go when the block is left, on every path."""
    from . import _lib
    rows = _Rows(lib, lib.dm_rows_create(base.encode('ascii')), [], {}, [])
    if not rows.h:
        raise _lib.DeepModHipError("dm_rows_create: " + _lib.last_error())
    try:
        yield rows
    finally:
        lib.dm_rows_destroy(rows.h)
        del rows.keep[:]


# an open raw container with event tables: z the mapped members, meta one record per read, raw_off / ev_off i64[n + 1] (raw_off checked against the samples),
# values = the ev_mean, ev_stdv (f64), ev_start, ev_length (u64) columns, move the ev_move column (i64)
_EventContainer = namedtuple('_EventContainer', 'path z meta n raw_off ev_off n_ev model_state values move')
# ... under --move: mv, mv_off, first, fq, fq_off are rawreads.MOVE_MEMBERS, all None for a container without move data
_MoveContainer = namedtuple('_MoveContainer', 'path z meta n raw_off mv mv_off first fq fq_off', defaults=(None,) * 5)
# what the signal stage gave for a batch: s_mean / s_stdv the statistics of every merged event (None: they stay on the device under `sig`), first_empty per read,
# m_mean / m_stdv the basecaller's values for the events at or behind a first empty event (None: no read has one)
_SignalStats = namedtuple('_SignalStats', 's_mean s_stdv first_empty m_mean m_stdv sig')


def _open_raw_container(f5f: str):
    """-> (mapped members, read metas, n, sample offsets) of a format-2 container, the offsets checked against the samples they index"""
    from . import npzmap
    z = npzmap.load(f5f, lazy=('ev_mean', 'ev_stdv'))
    if 'format' not in z:
        raise ValueError('format-1 raw container')
    meta = json.loads(str(z['meta']))
    n = len(meta)
    ro = _c_arr(z['raw_off'], np.int64)
    if len(ro) != n + 1 or ro[0] != 0 or (np.diff(ro) < 0).any() or ro[-1] > len(z['raw']):
        raise ValueError('signal offsets of a damaged container')
    return z, meta, n, ro


def _open_event_container(f5f: str) -> _EventContainer:
    """Open stage, event tables: path -> the columns dm_events_merge reads.  ValueError (or whatever the reader raises) for a damaged container."""
    z, meta, n, ro = _open_raw_container(f5f)
    eo = _c_arr(z['ev_off'], np.int64)
    if len(eo) != n + 1:
        raise ValueError('event offsets of a damaged container')
    ms = _c_arr(z['ev_model_state'], z['ev_model_state'].dtype)
    values = [_c_arr(z['ev_mean'], np.float64), _c_arr(z['ev_stdv'], np.float64), _c_arr(z['ev_start'], np.uint64), _c_arr(z['ev_length'], np.uint64)]
    return _EventContainer(f5f, z, meta, n, ro, eo, max(int(eo[-1]), 0), ms, values, _c_arr(z['ev_move'], np.int64))


def _open_move_container(f5f: str) -> _MoveContainer:
    """Open stage, detect --move: path -> the members dm_move_events reads (rawreads.py).  A container without them is no error here: its reads get the
    reference's reason one by one (_move_event_tables)."""
    z, meta, n, ro = _open_raw_container(f5f)
    if not all(k in z for k in rawreads.MOVE_MEMBERS):
        return _MoveContainer(f5f, z, meta, n, ro)
    if z['mv'].dtype != np.uint8 or z['fq'].dtype != np.uint8:
        raise ValueError('move tables of a damaged container')
    mvt, mvo, fst, fq, fqo = (_c_arr(z[k], dt) for k, dt in zip(rawreads.MOVE_MEMBERS, (np.uint8, np.int64, np.int64, np.uint8, np.int64)))
    # (dm_move_events checks the order of the offsets and their ends against the arrays)
    if len(mvo) != n + 1 or len(fqo) != n + 1 or len(fst) != n or (n and (mvo[0] != 0 or fqo[0] != 0)):
        raise ValueError('move offsets of a damaged container')
    return _MoveContainer(f5f, z, meta, n, ro, mvt, mvo, fst, fq, fqo)


class _RawBatch:
    """What the raw containers of a batch contribute, read after read in the order the signal request and dm_rows_add_raw see them: ids (None: a read without
    events) and id_src per read; raw_parts, whose concatenation is the samples; the merged event tables m_start / m_len / m_base, written in place at `w`
    container after container; under --move the move tables (move_parts, mv_offs, firsts), which travel to the signal stage themselves in the resident form.
    The *_offs lists grow while containers are added, raw_off / ev_off are their int64 arrays (_raw_events).  merges: (container, its merged offsets, events,
    position) of every dm_events_merge call - the record owns the arrays that call read, so _fallback_values can repeat it."""
    __slots__ = ('use_move', 'ids', 'id_src', 'raw_parts', 'raw_offs', 'ev_offs', 'raw_off', 'ev_off', 'm_start', 'm_len', 'm_base', 'w', 'move_parts', 'mv_offs', 'firsts', 'merges')

    def __init__(self, use_move: bool, cap_ev: int):
        self.use_move, self.w, self.merges, self.raw_off, self.ev_off = use_move, 0, [], None, None
        self.ids, self.id_src, self.raw_parts, self.raw_offs, self.ev_offs = [], [], [], [0], [0]
        self.move_parts, self.mv_offs, self.firsts = [], [0], []
        self.m_start, self.m_len, self.m_base = np.empty(max(cap_ev, 1), np.uint64), np.empty(max(cap_ev, 1), np.uint64), np.empty(max(cap_ev, 1), 'S1')

    def tables_at_w(self):
        """where the next container's merged (start, length, base) go"""
        return self.m_start.ctypes.data + 8 * self.w, self.m_len.ctypes.data + 8 * self.w, self.m_base.ctypes.data + self.w


def _merge_args(c: _EventContainer, mev_off: np.ndarray):
    """the input arguments of dm_events_merge for container c (the value and table outputs follow them)"""
    return (c.n, min(len(a) for a in c.values + [c.move, c.model_state]), c.ev_off.ctypes.data, *[a.ctypes.data for a in c.values],
            c.model_state.ctypes.data, c.model_state.dtype.itemsize // 4, c.move.ctypes.data, mev_off.ctypes.data)


def _merge_event_tables(lib, out: Prepared, opened: List[_EventContainer], b: _RawBatch) -> None:
    """Event tables of the batch, event-table containers: one dm_events_merge per container (getEvent's merge, rawreads.py) appends its reads to `b`.
    A read without events is a 'No events data' line of the ledger and keeps its place with id None."""
    for c in opened:
        mev_off = np.empty(c.n + 1, np.int64)
        # (the basecaller's mean / stdv are merged later and only if a read of the batch has an empty event: _fallback_values)
        got = lib.dm_events_merge(*_merge_args(c, mev_off), None, None, *b.tables_at_w())
        if got < 0:             # offsets that decrease or run past the table: a damaged container, the batch goes on without it
            _container_failed(out, c.path)
            continue
        b.merges.append((c, mev_off, got, b.w))
        per_read = mev_off[1:] - mev_off[:-1]
        for i, m in enumerate(c.meta):
            rid = m['read_id'].replace(" ", ":::").replace("\t", "|||")
            if per_read[i] == 0:
                out.errors['No events data'].append(c.path)
                rid = None
            b.ids.append(rid)
            b.id_src.append(c.path)
        b.raw_parts.append(c.z['raw'][:int(c.raw_off[-1])])          # samples behind the last read's end would shift every later container's offsets
        b.raw_offs.extend((b.raw_offs[-1] + c.raw_off[1:]).tolist())
        b.ev_offs.extend((b.ev_offs[-1] + mev_off[1:]).tolist())
        b.w += got


def _move_event_tables(lib, out: Prepared, opened: List[_MoveContainer], b: _RawBatch) -> None:
    """Event tables of the batch, detect --move: one dm_move_events per container segments its move tables (rawreads.py) and appends the reads that
    passed to `b`, with their move tables for the resident form of the signal request."""
    for c in opened:
        if c.mv is None:                 # a container without move data: the reference's reason, per read
            out.errors['No move data'].extend([c.path] * c.n)
            continue
        n, ro, mvt, mvo = c.n, c.raw_off, c.mv, c.mv_off
        mev_off, status = np.empty(n + 1, np.int64), np.empty(max(n, 1), np.int32)
        got = lib.dm_move_events(n, len(mvt), mvt.ctypes.data, mvo.ctypes.data, c.first.ctypes.data, ro.ctypes.data, len(c.fq), c.fq.ctypes.data,
                                 c.fq_off.ctypes.data, mev_off.ctypes.data, status.ctypes.data, *b.tables_at_w())
        if got < 0:
            _container_failed(out, c.path)
            continue
        good = np.flatnonzero(status[:n] == 0)
        for i in np.flatnonzero(status[:n] != 0):       # where the reference is undefined the read fails (rawreads.py)
            _container_failed(out, c.path, " (read {}: move table, status {})".format(c.meta[i]['read_id'], status[i]))
        for i in good:
            b.ids.append(c.meta[i]['read_id'].replace(" ", ":::").replace("\t", "|||"))
            b.id_src.append(c.path)
        for lo, hi in ([(0, n)] if len(good) == n else [(i, i + 1) for i in good]):      # the usual case: the container's arrays as they lie, else read by read
            b.raw_parts.append(c.z['raw'][int(ro[lo]):int(ro[hi])])
            b.move_parts.append(mvt[int(mvo[lo]):int(mvo[hi])])
            b.raw_offs.extend((b.raw_offs[-1] + (ro[lo + 1:hi + 1] - ro[lo])).tolist())
            b.mv_offs.extend((b.mv_offs[-1] + (mvo[lo + 1:hi + 1] - mvo[lo])).tolist())
        b.firsts.extend(c.first[good].tolist())
        per_read = (mev_off[1:] - mev_off[:-1])[good]               # (a failed read has no events: mev_off is already the compacted table's)
        b.ev_offs.extend((b.ev_offs[-1] + np.cumsum(per_read)).tolist())
        b.w += got


def _raw_events(lib, out: Prepared, raw_files: List[str], use_move: bool) -> _RawBatch:
    """Raw containers stage: paths -> the reads, samples and merged event tables of the batch (the reference's get_Event_Signals up to the signal
    normalisation, myDetect.py:392-465).  A container that cannot be opened or merged is reported and left out."""
    opener = _open_move_container if use_move else _open_event_container       # detect --move: the events come from the basecaller move tables (rawreads.py)
    opened = []
    for f5f in raw_files:
        try:
            opened.append(opener(f5f))
        except Exception:
            _container_failed(out, f5f)
    # the merged event tables of the whole batch, written in place container after container (no per-container pieces to concatenate)
    b = _RawBatch(use_move, sum(len(c.fq) for c in opened if c.mv is not None) if use_move else sum(c.n_ev for c in opened))
    (_move_event_tables if use_move else _merge_event_tables)(lib, out, opened, b)
    b.m_start, b.m_len, b.m_base = b.m_start[:b.w], b.m_len[:b.w], b.m_base[:b.w]
    b.raw_off, b.ev_off = np.array(b.raw_offs, np.int64), np.array(b.ev_offs, np.int64)
    return b


def _fallback_values(lib, b: _RawBatch):
    """The basecaller's mean / stdv of every merged event of the batch (getEvent's rounding): needed only for events at or behind a read's
    first empty event - the containers are merged once more, this time with the value columns."""
    from . import _lib
    if b.use_move:
        raise RuntimeError('a move read with an empty event: dm_move_events admits none')
    mm_, ms_ = np.empty(max(b.w, 1), np.float32), np.empty(max(b.w, 1), np.float32)
    for c, mev_off, got, at in b.merges:
        a_, b_ = np.empty(c.n_ev, np.float32), np.empty(c.n_ev, np.float32)
        scratch = (np.empty(c.n_ev, np.uint64), np.empty(c.n_ev, np.uint64), np.empty(c.n_ev, 'S1'))
        if lib.dm_events_merge(*_merge_args(c, mev_off), a_.ctypes.data, b_.ctypes.data, scratch[0].ctypes.data, scratch[1].ctypes.data, scratch[2].ctypes.data) != got:
            raise _lib.DeepModHipError('dm_events_merge: ' + _lib.last_error())
        mm_[at:at + got], ms_[at:at + got] = a_[:got], b_[:got]
    return mm_[:b.w], ms_[:b.w]


def _signal_request(lib, moptions, normalizer, b: _RawBatch, only_raw: bool, select_base: bool, rows_on_device: bool) -> _SignalStats:
    """Signal stage: the one request of the batch (normalisation + event statistics), in one of four ways: resident with the move tables segmented on the
    device, resident with host-built tables, resident, synchronous.  _BatchRefused when the batched call cannot take a read."""
    from . import _lib
    # resident form (round 6): a batch of raw containers only, whose rows are built on the device anyway - the signal request is POSTED
    # (samples + event tables into the server's request file, no wait) and its statistics never come back: the feeder needs only
    # first_empty (host arithmetic, dm_signal_plan_batch) to walk its alignments while the signal kernels run
    want_resident = (hasattr(normalizer, 'post_arrays') and only_raw and select_base and rows_on_device and _option_on(moptions, 'stats_on_device'))
    raw_off, mev_off, m_start, m_len = b.raw_off, b.ev_off, b.m_start, b.m_len
    per_read = mev_off[1:] - mev_off[:-1]
    s_mean = s_stdv = m_mean = m_stdv = sig = None
    try:
        if want_resident and b.use_move:
            # every event of a read that passed dm_move_events is non-empty: first_empty is the event count.  The move tables themselves are
            # posted (one byte per two samples instead of 16 per event) and segmented on the device; moptions['move_on_device'] = False /
            # DEEPMOD_MOVE_ON_DEVICE=0 posts the host-built tables through the event-table request instead
            first_empty = per_read.astype(np.int64)
            if hasattr(normalizer, 'post_move') and _option_on(moptions, 'move_on_device'):
                sig = normalizer.post_move(b.raw_parts, raw_off, b.move_parts, np.array(b.mv_offs, np.int64), np.array(b.firsts, np.int64), mev_off)
            else:
                sig = normalizer.post_arrays(b.raw_parts, raw_off, m_start, m_len, mev_off, first_empty, None, None)
        elif want_resident:
            first_empty = np.empty(len(raw_off) - 1, np.int64)
            _lib.check(lib.dm_signal_plan_batch(len(raw_off) - 1, raw_off.ctypes.data, mev_off.ctypes.data, m_start.ctypes.data, m_len.ctypes.data,
                                                first_empty.ctypes.data))
            if bool((first_empty < per_read).any()):
                m_mean, m_stdv = _fallback_values(lib, b)
            sig = normalizer.post_arrays(b.raw_parts, raw_off, m_start, m_len, mev_off, first_empty, m_mean, m_stdv)
        else:
            s_mean, s_stdv, first_empty = normalizer.event_stats_arrays(b.raw_parts, raw_off, m_start, m_len, mev_off)
            if bool((np.asarray(first_empty) < per_read).any()):
                m_mean, m_stdv = _fallback_values(lib, b)
    except _lib.DeepModHipError as exc:
        # a read the batched signal call cannot take (events covering no signal): the per-read Python path reports it
        raise _BatchRefused() from exc
    return _SignalStats(s_mean, s_stdv, first_empty, m_mean, m_stdv, sig)


def _add_alignments(rows: _Rows, out: Prepared, moptions, raw_files: List[str], b: _RawBatch, st: _SignalStats) -> None:
    """Alignment stage (myDetect.py:488-715): the reads of `b` and their statistics -> alignment records (the reference's own aligner call when the binary is
    on PATH, else the side-car .sam files) -> one dm_rows_add_raw, which walks them and plans the feature rows (get_Feature, :839-903)."""
    from . import _lib, detect, readmap
    mev_off, contigs = b.ev_off, rows.contigs
    f5data = {}
    for gi, rid in enumerate(b.ids):
        if rid is None:
            continue
        if rid in f5data:
            print('Duplicate id', rid, b.id_src[gi])
        call = b.m_base[mev_off[gi]:mev_off[gi + 1]].tobytes().decode('ascii', 'replace') if moptions.get('Ref') else ''
        f5data[rid] = (call, gi, None, b.id_src[gi], (0, 0))
    align_info = detect._alignment_lines(moptions, {'Error': out.errors}, raw_files, f5data)
    if align_info is None:
        for f5k in sorted(f5data.keys()):
            out.errors["Cannot running aligment"].append(f5data[f5k][3])
        return
    sp_param = {'f5data': f5data, 'ref_info': {}, 'f5status': "", 'line': ""}
    f5align = readmap.parse_sam(moptions, {'Error': out.errors}, sp_param, align_info, f5data)
    recs = list(f5align.items())
    nrec = len(recs)
    seqs = readmap.read_fasta(moptions['Ref']) if moptions.get('Ref') else {}
    ref_bytes = _REF_BYTES.setdefault(moptions.get('Ref'), {})
    flag = np.zeros(nrec, np.int32); pos1 = np.zeros(nrec, np.int64); rlen = np.zeros(nrec, np.int64)
    cidx = np.full(nrec, -1, np.int32); ev_read = np.zeros(nrec, np.int32); skip = np.zeros(nrec, np.uint8)
    cig_b, seq_b = [], []
    for i, (qname, (mapq, fl, rname, ps, cigar, seq)) in enumerate(recs):
        flag[i], pos1[i], ev_read[i] = fl, ps, f5data[qname][1]
        cig_b.append(cigar.encode('ascii')); seq_b.append(seq.encode('ascii'))
        rlen[i] = len(seq_b[-1])
        if (not moptions.get('ConUnk', True)) and any(ch in rname for ch in '_-/:'):
            skip[i] = 1
        if rname not in contigs:
            contigs[rname] = len(contigs)
        cidx[i] = contigs[rname]
        if rname in seqs and rname not in ref_bytes:
            ref_bytes[rname] = seqs[rname].encode('ascii')
        if rname not in seqs:
            print('Fatal Error!!! cannot find the chrosome sequence %s' % rname)
    names = sorted(contigs, key=contigs.get)
    nct = len(names)
    ref_used = [ref_bytes.get(nm) for nm in names]
    ref_ptr = (ctypes.c_char_p * max(nct, 1))(*ref_used)
    ref_len = np.array([len(ref_bytes[nm]) if nm in ref_bytes else 0 for nm in names] or [0], np.int64)
    cig_ptr = (ctypes.c_char_p * max(nrec, 1))(*cig_b)
    seq_ptr = (ctypes.c_char_p * max(nrec, 1))(*seq_b)
    region = [mr for mr in moptions.get('region', [[None, None, None]])]
    any_all = any(mr[0] in ['', None] and mr[1] in ['', None] and mr[2] in ['', None] for mr in region)
    if any_all:
        region = []
    elif not region:
        skip[:] = 1          # an EMPTY region list matches nothing (myDetect.py:548-556 leaves isinreg False): n_region = 0 below means "no filter"
    rg_c = np.array([(-1 if mr[0] in ['', None] else contigs.get(mr[0], 0x7fffffff)) for mr in region] or [0], np.int32)   # a contig no record of the batch names: matches nothing
    rg_lo = np.array([(-1 if mr[1] in ['', None] else int(mr[1])) for mr in region] or [0], np.int64)
    rg_hi = np.array([(-1 if mr[2] in ['', None] else int(mr[2])) for mr in region] or [0], np.int64)
    rows.keep.extend([flag, pos1, rlen, cidx, ev_read, skip, cig_b, seq_b, ref_used, ref_ptr, ref_len, cig_ptr, seq_ptr, mev_off, st.m_mean, st.m_stdv,
                      b.m_len, b.m_base, st.s_mean, st.s_stdv, st.first_empty, rg_c, rg_lo, rg_hi])
    ptr = lambda a: None if a is None else a.ctypes.data
    _lib.check(rows.lib.dm_rows_add_raw(rows.h, nrec, flag.ctypes.data, pos1.ctypes.data, cig_ptr, seq_ptr, rlen.ctypes.data, cidx.ctypes.data,
                                        ev_read.ctypes.data, skip.ctypes.data, nct, ref_ptr, ref_len.ctypes.data, len(mev_off) - 1, len(b.m_len), mev_off.ctypes.data,
                                        ptr(st.m_mean), ptr(st.m_stdv), b.m_len.ctypes.data, b.m_base.ctypes.data, ptr(st.s_mean), ptr(st.s_stdv),
                                        st.first_empty.ctypes.data, len(region), rg_c.ctypes.data, rg_lo.ctypes.data, rg_hi.ctypes.data))
    rows.srcs.extend(f5data[q][3] for q, _ in recs)
    for nm in names:
        if nm in ref_bytes:
            out.contig_len[nm] = len(ref_bytes[nm])


def _add_feature_containers(rows: _Rows, out: Prepared, files: List[str]) -> None:
    """Feature containers stage: every other file of the batch enters at the prediction step (the arguments of mPredict1, myDetect.py:787-834) -
    predstore.load_packed, then one dm_rows_add_packed per container.  out.timing['load'] covers the reading, ['rows'] the rest."""
    from . import _lib
    contigs, strands_c = rows.contigs, {'+': 0, '-': 1}
    t0 = time.perf_counter()
    for cf in files:
        if cf.endswith(rawreads.RAW_SUFFIX):
            continue
        try:
            pk = predstore.load_packed(cf)
        except Exception:
            out.errors["Cannot open container"].append(cf)
            continue
        t1 = time.perf_counter()
        out.timing['load'] += t1 - t0
        meta = pk['reads']
        n = len(meta)
        if n:
            for m in meta:
                if m['chr'] not in contigs:
                    contigs[m['chr']] = len(contigs)
            row_off, bmi_off, ev_off = (_c_arr(pk[k], np.int64) for k in ('row_off', 'bmi_off', 'ev_off'))
            tx, refbasei = _c_arr(pk['tx'], np.float32), _c_arr(pk['refbasei'], np.int64)
            refbase, readbase, evbase = (_c_arr(pk[k], 'S1') for k in ('refbase', 'readbase', 'evbase'))
            arrs = [row_off, bmi_off, ev_off, tx, refbase, readbase, refbasei, evbase,
                    np.array([m['start_clip'] for m in meta], np.int64), np.array([m['end_clip'] for m in meta], np.int64),
                    np.array([contigs[m['chr']] for m in meta], np.int32), np.array([strands_c[m['strand']] for m in meta], np.int32)]
            rows.keep.append(arrs)
            n_tab = min(len(refbase), len(readbase), len(refbasei))
            if (min(len(row_off), len(bmi_off), len(ev_off)) != n + 1 or tx.ndim != 2 or tx.shape[1] != 7 or
                    rows.lib.dm_rows_add_packed(rows.h, n, len(tx), n_tab, len(evbase), len(contigs), *[a.ctypes.data for a in arrs]) != 0):
                # offset tables that do not fit their arrays (a truncated / damaged container): the file is reported, the batch goes on
                out.errors["Cannot open container"].append(cf)
                print("Cannot open container: %s (%s)" % (cf, _lib.last_error() or 'offset tables of the wrong length'))
                continue
            rows.srcs.extend([cf] * n)
        for c, ln in pk.get('contig_len', {}).items():
            out.contig_len[c] = max(out.contig_len.get(c, 0), int(ln))
        t0 = time.perf_counter()
        out.timing['rows'] += t0 - t1


def _rows_info(rows: _Rows, out: Prepared, compact: bool):
    """Info and ledger stage: dm_rows_info -> the sizes (R feature rows, T position entries, S windows on a base of interest), the ledger line or the
    log lines of every read that failed (myDetect.py:702-705, :826-828) and the read / window counts of the batch."""
    from . import _lib
    srcs = rows.srcs
    nreads = len(srcs)
    info = np.zeros((max(nreads, 1), 8), np.int64)
    mism = np.zeros((20, 4), np.int64)
    R, T, S, nm = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    if rows.lib.dm_rows_info(rows.h, ctypes.byref(R), ctypes.byref(T), ctypes.byref(S), info.ctypes.data, mism.ctypes.data, 20, ctypes.byref(nm)) < 0:
        raise _lib.DeepModHipError("dm_rows_info: " + _lib.last_error())
    for i in range(nreads):
        st = int(info[i, 0])
        if st in _ROWS_ERRORS:
            out.errors[_ROWS_ERRORS[st]].append(srcs[i])
        elif st == 3:
            print("Errorfast5 " + srcs[i])
            print('match-Error!!! no first and/or last match', srcs[i])
    for j in range(min(int(nm.value), 20)):
        print('Error Does not match: read %d of the batch (%s), table row %d, event %d, %d bases differ'
              % (mism[j, 0], srcs[int(mism[j, 0])], mism[j, 1], mism[j, 2], mism[j, 3]))
    R, T, S = int(R.value), int(T.value), int(S.value)
    if compact:
        T = S + (T - R)                 # [S windows on a base of interest | extras]
    ok = info[:nreads, 0] == 0
    out.n_reads = int(ok.sum())
    out.n_windows = int(info[:nreads, 3][ok].sum())
    out.n_rows = R
    return R, T, S


def _heap_alloc(R: int, T: int, S: int = 0, dev=None):
    """`alloc` of a batch that stays in this process: the tuples a feeder's alloc returns (feeder_process_main), from the heap"""
    if dev is not None:
        return (np.empty((max(dev[0], 1), 3), np.float32), np.empty(R, np.uint8), np.empty((dev[1], 4), np.int64), np.empty(T, np.int64), np.empty(T, np.uint8),
                np.empty(S, np.int32))
    return (np.empty((R, 7), np.float32), np.empty(T, np.int64), np.empty(T, np.uint8)) + ((np.empty(S, np.int32),) if S else ())


def _allocate(rows: _Rows, out: Prepared, alloc, R: int, T: int, S: int, compact: bool, rows_on_device: bool) -> None:
    """Allocate stage: the hand-over arrays of a batch of R > 0 rows, as fields of `out`, straight in the hand-over slot when `alloc` is given.  Four
    shapes: rows | pos | flags (classic); the same with sel (compact); ev3 | code | rdesc | pos | flags | sel (device form); the same without ev3
    (resident form).  alloc(R, T), alloc(R, T, S) and alloc(R, T, S, dev=(events, reads)) return them in that order."""
    from . import _lib
    # device form (round 5): a batch of raw reads only hands over (mean, stdv, length) per event, a class byte per row and a descriptor per
    # read; the [R][7] matrix is built on the device.  moptions['rows_on_device'] = False / DEEPMOD_ROWS_ON_DEVICE=0: rows on the host as before
    dev_form = None
    resident = out.sig is not None
    if compact and (resident or rows_on_device):
        ne, nr = ctypes.c_int64(), ctypes.c_int64()
        if rows.lib.dm_rows_device_info(rows.h, ctypes.byref(ne), ctypes.byref(nr)) == 1:
            dev_form = (0 if resident else int(ne.value), int(nr.value))
    if resident and dev_form is None:
        raise _lib.DeepModHipError('a batch whose statistics stay on the device must be a batch of raw reads')
    alloc = alloc or _heap_alloc
    if dev_form is not None:
        out.ev3, out.code, out.rdesc, out.pos, out.flags, sel = alloc(R, T, S, dev=dev_form)
        out.sel = sel if S else np.zeros(0, np.int32)
        if resident:
            out.ev3 = None
        out.rows = None
    else:
        got = alloc(R, T, S) if compact else alloc(R, T)
        out.rows, out.pos, out.flags = got[:3]
        out.sel = (got[3] if S else np.zeros(0, np.int32)) if compact else None


def _emit(rows: _Rows, out: Prepared, compact: bool) -> None:
    """Emit stage: dm_rows_emit* writes the allocated arrays in the form _allocate chose, reads grouped by (contig in name order, strand); then the groups,
    the lower bounds of the contig lengths and the range flag (which classifier kernel takes the batch) are read back."""
    from . import _lib
    lib, h, contigs = rows.lib, rows.h, rows.contigs
    names = sorted(contigs, key=contigs.get)
    rank = np.empty(max(len(names), 1), np.int32)
    rank[np.argsort(np.array(names, dtype=object), kind='stable') if names else []] = np.arange(len(names), dtype=np.int32)
    clen = np.zeros(max(len(names), 1), np.int64)
    groups = np.zeros((2 * max(len(names), 1), 8), np.int64)
    in_range = ctypes.c_int32(1)
    sel_dummy = np.zeros(1, np.int32)
    sel_ptr = (out.sel.ctypes.data if len(out.sel) else sel_dummy.ctypes.data) if compact else None
    tail = (out.pos.ctypes.data, out.flags.ctypes.data, groups.ctypes.data, len(groups), clen.ctypes.data, len(clen), ctypes.byref(in_range))
    if out.sig is not None:
        ng = lib.dm_rows_emit_resident(h, rank.ctypes.data, out.code.ctypes.data, out.rdesc.ctypes.data, sel_ptr, *tail)
    elif out.ev3 is not None:
        ng = lib.dm_rows_emit_device(h, rank.ctypes.data, out.ev3.ctypes.data, out.code.ctypes.data, out.rdesc.ctypes.data, sel_ptr, *tail)
    else:
        ng = lib.dm_rows_emit(h, rank.ctypes.data, out.rows.ctypes.data, sel_ptr, *tail)
    if ng < 0:
        raise _lib.DeepModHipError("dm_rows_emit: " + _lib.last_error())
    out.groups = [(names[int(g[0])], '+-'[int(g[1])]) + tuple(int(v) for v in (g[2:8] if compact else g[2:6])) for g in groups[:ng]]
    for i, nmn in enumerate(names):
        if clen[i] > out.contig_len.get(nmn, 0):
            out.contig_len[nmn] = int(clen[i])        # lower bound when no reference length is known
    out.f32 = not bool(in_range.value)


def _prepare_batch_c(moptions, files: List[str], make_normalizer=None, alloc=None) -> Prepared:
    """prepare_batch with the per-read work behind the C ABI, as the stages above: one dm_events_merge / dm_move_events per raw
    container, one signal request, one dm_rows_add_raw / dm_rows_add_packed per input kind, dm_rows_info + dm_rows_emit straight into the hand-over
    arrays.  Same Prepared (rows, pos, flags, groups, errors) as the Python path below, which stays as the restatement the tests compare with
    (tests/test_stream_feeders.py)."""
    from . import _lib
    lib = _lib.load()
    out = Prepared()
    out.files = list(files)
    # compact form unless the caller wants every window classified (moptions['select_base'] = False / DEEPMOD_SELECT_BASE=0)
    compact, rows_on_device = _option_on(moptions, 'select_base'), _option_on(moptions, 'rows_on_device')
    raw_files = [f for f in files if f.endswith(rawreads.RAW_SUFFIX)]
    try:
        with _rows_handle(lib, moptions['Base']) as rows:
            t0 = time.perf_counter()
            if raw_files:
                normalizer = make_normalizer() if make_normalizer else None
                if normalizer is None:
                    from . import signal as dmsignal
                    normalizer = dmsignal.SignalNormalizer(int(moptions.get('device', 0)))
                batch = _raw_events(lib, out, raw_files, bool(moptions.get('move')))
                t1 = time.perf_counter()
                out.timing['load'] += t1 - t0
                if batch.ids:
                    stats = _signal_request(lib, moptions, normalizer, batch, len(raw_files) == len(files), compact, rows_on_device)
                    out.sig = stats.sig
                    t2 = time.perf_counter()
                    out.timing['signal'] += t2 - t1
                    _add_alignments(rows, out, moptions, raw_files, batch, stats)
                    out.timing['map+features'] += time.perf_counter() - t2
            _add_feature_containers(rows, out, files)
            # ---- sizes, errors, then the arrays themselves (straight into the hand-over slot when alloc is given) ----
            t0 = time.perf_counter()
            R, T, S = _rows_info(rows, out, compact)
            if R:
                _allocate(rows, out, alloc, R, T, S, compact, rows_on_device)
                _emit(rows, out, compact)
            out.timing['rows'] += time.perf_counter() - t0
            return out
    except _BatchRefused:       # (the handle is gone by now)
        return _prepare_batch_py(moptions, files, make_normalizer, alloc)


def prepare_batch(moptions, files: List[str], make_normalizer=None, alloc=None) -> Prepared:
    """Host side of one worker batch (the reference's mDetect1 up to the call of mPredict1, myDetect.py:392-465, :488-715):
    raw containers go through signal normalisation, alignment records, dm_map_read and get_Feature; feature containers
    enter at the prediction step.  Default: the compiled path (_prepare_batch_c); moptions['rows_in_c'] = False (or
    DEEPMOD_ROWS_IN_C=0) selects the per-read Python restatement."""
    if _option_on(moptions, 'rows_in_c'):
        return _prepare_batch_c(moptions, files, make_normalizer, alloc)
    return _prepare_batch_py(moptions, files, make_normalizer, alloc)


def _prepare_batch_py(moptions, files: List[str], make_normalizer=None, alloc=None) -> Prepared:
    """The per-read Python / numpy path (rounds 1-2): kept as the restatement the compiled path is tested against."""
    out = _PreparedBuilder()
    out.files = list(files)
    base = moptions['Base']
    t0 = time.perf_counter()
    raw_files = [f for f in files if f.endswith(rawreads.RAW_SUFFIX)]
    if raw_files:
        from . import detect, readmap
        sp_options = {'Error': out.errors}
        normalizer = make_normalizer() if make_normalizer else None
        f5data = rawreads.get_Event_Signals(moptions, sp_options, raw_files, normalizer)
        t1 = time.perf_counter()
        out.timing['signal'] += t1 - t0
        if f5data:
            align_info = detect._alignment_lines(moptions, sp_options, raw_files, f5data)
            if align_info is None:
                for f5k in sorted(f5data.keys()):
                    out.errors["Cannot running aligment"].append(f5data[f5k][3])
            else:
                sp_param = {'f5data': f5data, 'ref_info': {}, 'f5status': "", 'line': ""}
                f5align = readmap.parse_sam(moptions, sp_options, sp_param, align_info, f5data)
                reads = readmap.map_records(moptions, sp_options, sp_param, f5align, f5data)
                t2 = time.perf_counter()
                out.timing['map+features'] += t2 - t1
                rows_from_reads(reads, base, raw_files[0], out)
                for c, seq in sp_param['ref_info'].items():
                    out.contig_len[c] = len(seq)
                out.timing['rows'] += time.perf_counter() - t2
        t0 = time.perf_counter()
    for cf in files:
        if cf.endswith(rawreads.RAW_SUFFIX):
            continue
        try:
            pk = predstore.load_packed(cf)
        except Exception:
            out.errors["Cannot open container"].append(cf)
            continue
        t1 = time.perf_counter()
        out.timing['load'] += t1 - t0
        rows_from_packed(pk, base, cf, out)
        t0 = time.perf_counter()
        out.timing['rows'] += t0 - t1
    finish(out, alloc)
    out.timing['rows'] += time.perf_counter() - t0
    return out
