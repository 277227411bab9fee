"""`bslabels`: the three position lists getfeatures --motifORPos 2 reads (--fulmod, --anymod, --nomod: `chr strand pos` lines;
getfeatures.readPosFiles), from 1 to 4 whole-genome bisulfite bedMethyl replicates and the reference.  The reference trained its human
5mC model on positions "completely methylated (>90 % in both bisulfite replicates)" and "completely un-methylated (<=0 % in both replicates)" and ships
nothing that writes them; this command does.

The replicates are read by exactly `bsperf`'s rules (bsperf.host_rows, bsperf.read_truth_device: one copy of the code).  A key (strand, position) is
admissible if the motif lies on that strand with its modified base at that position (siteperf.site_codes on the upper-cased reference bytes, as
getfeatures.readFA hands them over).  The class of an admissible key with R replicates, c = --cov:
  fulmod  every replicate has a record, the smallest coverage is >= c, every percentage is >= --methylated
  nomod   every replicate has a record, the smallest coverage is >= c, every percentage is <= --unmethylated
  anymod  every other key with a record in at least one replicate: partial methylation, replicates that disagree, low coverage, a key missing from one
A key with truth that is not admissible is in no list (off_motif).  The lists are disjoint.  anymod is deliberately wide: getfeatures --posneg 1 gives
a position of anymod no label and only a position of nomod the negative one, so a site one cannot be sure of must land in anymod.

HostEngine below is the numpy statement of the semantics and the yardstick of the kernels (csrc/bslabels.hip.inc, DeviceEngine).
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import numpy as np

from . import _lib, bsperf, merge, siteperf

MAX_REPLICATES, MAX_CONTIGS, MAX_NAME, MAX_COV, MAX_MOTIF = bsperf.MAX_REPLICATES, bsperf.MAX_CONTIGS, bsperf.MAX_NAME, bsperf.MAX_COV, 8
MAX_LENGTH = bsperf.MAX_LENGTH
LINE_KEYS = bsperf.LINE_KEYS
C_NONE, C_FUL, C_ANY, C_NO, C_OFF = 0, 1, 2, 3, 4                  # the class byte of a key (blk::C_* of csrc/bslabels.inc)
LISTS = {'fulmod': C_FUL, 'anymod': C_ANY, 'nomod': C_NO}
COUNT_KEYS = ('fulmod', 'anymod', 'nomod', 'off_motif', 'sites_without_truth')
CHUNK_BYTES = bsperf.CHUNK_BYTES
TEXT_RUN_BYTES = 64 << 20                                # of list text fetched from the device at once (whole tiles)


class BsLabelsError(ValueError):
    pass


def _renamed(exc: Exception, prefix: str = '') -> BsLabelsError:
    """An error of the code shared with bsperf / siteperf, under this command's name."""
    text = str(exc)
    for other in ('bsperf: ', 'siteperf: '):
        if text.startswith(other):
            text = text[len(other):]
    return BsLabelsError('bslabels: ' + prefix + text)


def check_motif(motif: str, k: int, base: str = None) -> None:
    """1 to 8 letters of A, C, G, T; k inside the motif; the letter there is --Base."""
    if not isinstance(motif, str) or not 1 <= len(motif) <= MAX_MOTIF:
        raise BsLabelsError('bslabels: --motif: a motif has 1 to %d bases (got %r)' % (MAX_MOTIF, motif))
    if not 0 <= int(k) < len(motif):
        raise BsLabelsError('bslabels: --ModinMotif %d is no position in the motif %s' % (k, motif))
    try:
        siteperf.check_motif(motif, int(k))
    except siteperf.SitePerfError as exc:
        raise _renamed(exc, '--motif: ')
    if base is not None and motif[k] != base:
        raise BsLabelsError('bslabels: --ModinMotif %d: the letter of the motif %s there is %s, not --Base %s' % (k, motif, motif[k], base))


def _check_engine_options(names, lengths, replicates, cov, methylated, unmethylated) -> List[int]:
    if not 1 <= len(names) <= MAX_CONTIGS:
        raise BsLabelsError('bslabels: --chr: 1 to %d contigs (got %d)' % (MAX_CONTIGS, len(names)))
    for n in names:
        if not 1 <= len(n) <= MAX_NAME or any(not 0x21 <= ord(c) <= 0x7e for c in n):
            raise BsLabelsError('bslabels: --chr: a contig name has 1 to %d printable bytes (got %r)' % (MAX_NAME, n))
    if len(set(names)) != len(names):
        raise BsLabelsError('bslabels: --chr: a contig is named twice')
    if lengths is None or len(lengths) != len(names) or any(v is None or not 1 <= int(v) <= MAX_LENGTH for v in lengths):
        raise BsLabelsError('bslabels: --Ref: every contig needs its length, 1 to 2^31 - 1 bases (getfeatures refuses a position that is not in the reference)')
    if not 1 <= int(replicates) <= MAX_REPLICATES:
        raise BsLabelsError('bslabels: --truth: 1 to %d replicate files (got %d)' % (MAX_REPLICATES, replicates))
    if not 1 <= int(cov) <= MAX_COV:
        raise BsLabelsError('bslabels: --cov: the least coverage is 1 to %d, where a record\'s coverage saturates (got %d)' % (MAX_COV, cov))
    if not 0 <= int(unmethylated) < int(methylated) <= 100:
        raise BsLabelsError('bslabels: --unmethylated / --methylated: 0 <= unmethylated < methylated <= 100 (got %d, %d)' % (unmethylated, methylated))
    return [int(v) for v in lengths]


class HostEngine:
    """The semantics in numpy, one contig at a time.  open: the contig's reference bytes (upper case) and the motif -> the site codes and zeroed
    truth slots; fill: the records of a replicate (bsperf.HostEngine.fill: its checks and its duplicate rule); classify -> counts int64 [2 strands][5]
    (COUNT_KEYS) of this contig and cls uint8 [2][length] (C_*)."""

    def __init__(self, names, lengths, replicates: int = 2, cov: int = 5, methylated: int = 90, unmethylated: int = 0):
        self.names = list(names)
        self.limit = _check_engine_options(self.names, lengths, replicates, cov, methylated, unmethylated)
        self.R, self.cov, self.methylated, self.unmethylated = int(replicates), int(cov), int(methylated), int(unmethylated)
        self.contig = None

    def close(self):
        pass

    def open(self, contig: int, seq, motif: str, k: int = 0, base: str = None):
        self.contig = None
        if not 0 <= contig < len(self.names):
            raise BsLabelsError('bslabels: contig %d of %d' % (contig, len(self.names)))
        check_motif(motif, k, base)
        if len(seq) != self.limit[contig]:
            raise BsLabelsError('bslabels: %d reference bytes for a contig of %d positions' % (len(seq), self.limit[contig]))
        self.code = siteperf.site_codes(seq, motif, k)
        self.length = len(self.code)
        self.truth = np.zeros((self.R, 2, self.length), np.uint32)
        self.contig, self.refused, self.counted, self.cls = contig, False, False, None

    def close_contig(self):
        self.contig = None

    def _opened(self):
        if self.contig is None:
            raise bsperf.BsPerfError('bsperf: no contig')

    def fill(self, replicate: int, pos, meta):
        try:
            if self.contig is not None and self.counted:
                raise bsperf.BsPerfError('bsperf: the contig has been classified')
            bsperf.HostEngine.fill(self, replicate, pos, meta)           # the slots, the range checks and the duplicate rule are bsperf's
        except bsperf.BsPerfError as exc:
            raise _renamed(exc)

    def classify(self) -> np.ndarray:
        if self.contig is None:
            raise BsLabelsError('bslabels: no contig is open')
        if self.refused or self.counted:
            raise BsLabelsError('bslabels: the contig was refused or has been classified')
        t = self.truth.astype(np.int64)
        rec = t != 0
        some, every = rec.any(axis=0), rec.all(axis=0)
        cov, pct = t & 0xffff, (t >> 16) & 0x7f
        deep = every & (cov.min(axis=0) >= self.cov)
        high, low = (pct >= self.methylated).all(axis=0), (pct <= self.unmethylated).all(axis=0)
        site = np.stack([(self.code & 1) != 0, (self.code & 2) != 0])
        cls = np.where(~some, C_NONE, np.where(~site, C_OFF, np.where(deep & high, C_FUL, np.where(deep & low, C_NO, C_ANY)))).astype(np.uint8)
        counts = np.zeros((2, len(COUNT_KEYS)), np.int64)
        for s in range(2):
            for j, c in enumerate((C_FUL, C_ANY, C_NO, C_OFF)):
                counts[s, j] = int((cls[s] == c).sum())
            counts[s, 4] = int((site[s] & ~some[s]).sum())
        self.cls, self.counted = cls, True
        return counts

    def fetch_classes(self) -> np.ndarray:
        if self.contig is None or self.cls is None:
            raise BsLabelsError('bslabels: no classified contig')
        return self.cls.copy()


def format_list_host(name: str, cls, which: int, first_pos: int = 0) -> bytes:
    """The text of one list (which: C_FUL, C_ANY, C_NO) from cls [2][n], the classes of positions first_pos .. first_pos + n - 1: '%s %s %d\\n'
    (name, strand, position) per key of the class, ascending position, '+' before '-' at one position."""
    cls = np.asarray(cls)
    key = np.sort(np.concatenate([np.nonzero(cls[0] == which)[0] * 2, np.nonzero(cls[1] == which)[0] * 2 + 1]))
    return ''.join('%s %s %d\n' % (name, '+-'[int(v) & 1], first_pos + (int(v) >> 1)) for v in key).encode('ascii')


def format_lists_host(name: str, cls, first_pos: int = 0) -> Dict[str, bytes]:
    """{'fulmod': text, 'anymod': text, 'nomod': text} of one contig from its class arrays."""
    return {k: format_list_host(name, cls, c, first_pos) for k, c in LISTS.items()}


def format_host_routine(name: str, which: int, cls_plus, cls_minus, first_pos: int = 0, cap: int = None) -> Tuple[int, bytes]:
    """The device's line routine compiled for the host (dm_bslabels_format_host; no GPU needed) -> (bytes of the text, the buffer of cap bytes
    it was handed, which was filled with 0xa5; cap None: a buffer of exactly the size).  A write behind the buffer is an error."""
    import ctypes
    lib = _lib.load()
    arrs = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in (cls_plus, cls_minus)]
    n = len(arrs[0] if arrs[0] is not None else arrs[1])
    ptr = [None if a is None else a.ctypes.data for a in arrs]
    enc = name.encode('ascii', 'replace')
    need = lib.dm_bslabels_format_host(enc, int(which), ptr[0], ptr[1], int(first_pos), n, None, 0)
    if need < 0:
        _lib.check(int(need))
    cap = need if cap is None else int(cap)
    raw = bytearray(b'\xa5' * (cap + 8))
    got = lib.dm_bslabels_format_host(enc, int(which), ptr[0], ptr[1], int(first_pos), n, (ctypes.c_char * len(raw)).from_buffer(raw), cap)
    if got < 0:
        _lib.check(int(got))
    if bytes(raw[cap:]) != b'\xa5' * 8:
        raise BsLabelsError('bslabels: dm_bslabels_format_host wrote behind its buffer')
    return int(got), bytes(raw[:cap])


def tile_positions() -> int:
    return _lib.load().dm_bslabels_tile_positions()


class DeviceEngine(bsperf.DeviceTruth, _lib.Handle):
    """The same on one GPU (dm_bslabels_* of the C ABI).  add_truth_text / add_truth_records / records are what bsperf.read_truth_device drives.
    times(): ms of the parse / fill / class / format kernels so far."""
    PREFIX, N_TIMES, ERROR = 'dm_bslabels', 4, BsLabelsError

    def __init__(self, names, lengths, replicates: int = 2, cov: int = 5, methylated: int = 90, unmethylated: int = 0, device: int = 0):
        self.names = list(names)
        self.limit = _check_engine_options(self.names, lengths, replicates, cov, methylated, unmethylated)
        self.R = int(replicates)
        arr, lens = bsperf._names_args(self.names, self.limit)
        self._create(device, len(self.names), arr, lens.ctypes.data, self.R, int(cov), int(methylated), int(unmethylated))
        self._n, self.length, self.name = 0, 0, None

    def open(self, contig: int, seq, motif: str, k: int = 0):
        seq = np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, np.uint8)
        self.length = 0
        self._libmod.check(self._lib.dm_bslabels_open(self._h, int(contig), seq.ctypes.data, len(seq), str(motif).encode('ascii', 'replace'), len(motif), int(k)))
        self.length, self.name = len(seq), self.names[contig]

    def close_contig(self):
        self.length = 0
        self._libmod.check(self._lib.dm_bslabels_close_contig(self._h))

    def classify(self) -> np.ndarray:
        counts = np.zeros((2, len(COUNT_KEYS)), np.int64)
        self._libmod.check(self._lib.dm_bslabels_classify(self._h, counts.ctypes.data))
        return counts

    def fetch_classes(self) -> np.ndarray:
        cls = np.zeros((2, max(self.length, 1)), np.uint8)
        self._libmod.check(self._lib.dm_bslabels_fetch_classes(self._h, cls.ctypes.data))
        return cls[:, :self.length]

    def format_begin(self, which: int) -> Tuple[int, int, int]:
        """-> (lines, bytes, bytes of the largest tile) of list `which` of the classified contig."""
        ct = self._ct
        a, b, c = ct.c_int64(0), ct.c_int64(0), ct.c_int64(0)
        self._libmod.check(self._lib.dm_bslabels_format_begin(self._h, int(which), ct.byref(a), ct.byref(b), ct.byref(c)))
        return a.value, b.value, c.value

    def format_next(self, cap: int, buf=None) -> Tuple[int, bytes]:
        """-> (1 while more follows else 0, the next run of whole tiles that fits cap bytes); buf: a ctypes buffer of at least cap bytes to reuse."""
        ct = self._ct
        buf = ct.create_string_buffer(max(int(cap), 1)) if buf is None else buf
        got = ct.c_int64(0)
        rc = self._lib.dm_bslabels_format_next(self._h, buf, int(cap), ct.byref(got))
        if rc < 0:
            self._libmod.check(rc)
        return rc, ct.string_at(buf, got.value)

    def runs(self, which: int, cap: int = None):
        """The text of list `which` in runs of whole tiles of at most cap bytes (None: TEXT_RUN_BYTES, at least the largest tile, at most the text)."""
        n_lines, n_bytes, largest = self.format_begin(which)
        cap = min(max(TEXT_RUN_BYTES, largest), max(n_bytes, 1)) if cap is None else cap
        buf = self._ct.create_string_buffer(max(int(cap), 1))                      # one buffer for every run of the list
        more = 1
        while more:
            more, text = self.format_next(cap, buf)
            if text:
                yield text


def check_options(mo: Dict[str, object]):
    """What can be refused before a replicate is read or any GPU asked for -> (contigs, truth files, {contig: upper-cased bases}, motif, k)."""
    truth = [p for p in (mo.get('truth') or []) if p]
    if not truth:
        raise BsLabelsError('bslabels: --truth: the bisulfite bedMethyl replicates, separated by commas, are needed')
    if len(truth) > MAX_REPLICATES:
        raise BsLabelsError('bslabels: --truth: 1 to %d replicate files (got %d)' % (MAX_REPLICATES, len(truth)))
    for p in truth:
        if not os.path.isfile(p):
            raise BsLabelsError('bslabels: --truth: replicate file does not exist (%s)' % p)
    ref = mo.get('Ref')
    if not ref:
        raise BsLabelsError('bslabels: --Ref: the reference FASTA is needed (getfeatures refuses a position that is not in the reference)')
    if not os.path.isfile(ref):
        raise BsLabelsError('bslabels: --Ref: reference file does not exist (%s)' % ref)
    base = str(mo.get('Base') or 'C')
    motif = str(mo.get('motif') or base)
    k = int(mo.get('ModinMotif') or 0)
    check_motif(motif, k, base)
    named = list(mo.get('chr') or [])
    if len(named) > MAX_CONTIGS:
        raise BsLabelsError('bslabels: --chr: 1 to %d contigs (got %d)' % (MAX_CONTIGS, len(named)))
    _check_engine_options(named or ['chr1'], [1] * max(len(named), 1), len(truth), int(mo.get('cov', 5)), int(mo.get('methylated', 90)), int(mo.get('unmethylated', 0)))
    fasta = siteperf.read_fasta(ref)
    if named:
        missing = [ck for ck in named if ck not in fasta]
        if missing:
            raise BsLabelsError('bslabels: --chr: %s holds no contig %s' % (ref, ', '.join(missing)))
        chrkeys = named
    else:
        chrkeys = [ck for ck in merge.CHRKEYS if ck in fasta]
        if not chrkeys:
            raise BsLabelsError('bslabels: --chr: %s holds none of chr1..22, chrX, chrY, chrM: name the contigs' % ref)
    seqs = {ck: fasta[ck].upper() for ck in chrkeys}
    _check_engine_options(chrkeys, [len(seqs[ck]) for ck in chrkeys], len(truth), int(mo.get('cov', 5)), int(mo.get('methylated', 90)), int(mo.get('unmethylated', 0)))
    return chrkeys, truth, seqs, motif, k


def list_path(out_folder: str, fileid: str, which: str, contig: str) -> str:
    return os.path.join(out_folder, '%s.%s.%s.txt' % (fileid, which, contig))


def bslabels(mo: Dict[str, object], device: int = 0, chunk_bytes: int = CHUNK_BYTES) -> Dict[str, object]:
    """The command.  mo: truth (list of replicate files), Ref, Base, outFolder, FileID, chr (list; None: those of chr1..22, X, Y, M the FASTA has),
    motif (None: Base), ModinMotif, cov, methylated, unmethylated.  Writes <outFolder>/<FileID>.fulmod.<chr>.txt / .anymod. / .nomod. per contig
    and <outFolder>/<FileID>_bslabels.json -> the JSON document (with the wall-clock seconds of the phases in 'phase_s', which are not written)."""
    import json
    import time
    chrkeys, truth, seqs, motif, k = check_options(mo)
    base, fileid, out_folder = str(mo.get('Base') or 'C'), str(mo.get('FileID') or 'mod'), str(mo['outFolder'])
    cov, methylated, unmethylated = int(mo.get('cov', 5)), int(mo.get('methylated', 90)), int(mo.get('unmethylated', 0))
    if _lib.load().dm_device_count() < 1:
        raise BsLabelsError('no gfx950 GPU visible (this build has no CPU path)')
    lengths = [len(seqs[ck]) for ck in chrkeys]
    R = len(truth)
    phase = {key: 0.0 for key in ('read', 'parse', 'bucket', 'fill', 'class', 'format')}
    doc = {'inputs': {'truth': truth, 'Ref': mo.get('Ref'), 'Base': base, 'FileID': fileid, 'chr': chrkeys, 'motif': motif, 'ModinMotif': k, 'cov': cov,
                      'methylated': methylated, 'unmethylated': unmethylated},
           'truth': {}, 'contigs': {}, 'notes': []}
    os.makedirs(out_folder, exist_ok=True)
    report = []
    eng = DeviceEngine(chrkeys, lengths, R, cov, methylated, unmethylated, device)
    try:
        records = []
        for r, path in enumerate(truth):
            try:
                by_contig, lines = bsperf.read_truth_device(eng, r, path, chrkeys, lengths, doc['notes'], phase, chunk_bytes)
            except bsperf.BsPerfError as exc:
                raise _renamed(exc)
            records.append(by_contig)
            doc['truth'][path] = dict(zip(LINE_KEYS, (int(v) for v in lines)), lines_seen=int(lines.sum()))
        for c, ck in enumerate(chrkeys):
            have = [records[r].get(c) for r in range(R)]
            t0 = time.perf_counter()
            try:
                eng.open(c, seqs[ck], motif, k)
            except _lib.DeepModHipError as exc:
                if exc.code == _lib.DM_ENOMEM:
                    raise BsLabelsError('bslabels: %s: %s' % (ck, str(exc).split(': ', 2)[-1]))
                raise
            for r, h in enumerate(have):
                if h is not None:
                    try:
                        eng.fill(r, h[0], h[1])
                    except BsLabelsError as exc:
                        raise BsLabelsError('%s: %s: %s' % (truth[r], ck, str(exc)[len('bslabels: '):]))
            t1 = time.perf_counter()
            phase['fill'] += t1 - t0
            counts = eng.classify()
            t2 = time.perf_counter()
            phase['class'] += t2 - t1
            entry = {'length': lengths[c], 'truth_records': [0 if h is None else int(len(h[0])) for h in have], 'files': {}}
            for s, strand in enumerate('+-'):
                entry[strand] = dict(zip(COUNT_KEYS, (int(v) for v in counts[s])))
            for which, code in LISTS.items():
                path = list_path(out_folder, fileid, which, ck)
                with open(path, 'wb') as fh:
                    for text in eng.runs(code):
                        fh.write(text)
                entry['files'][which] = path
            phase['format'] += time.perf_counter() - t2
            doc['contigs'][ck] = entry
            report.append('%s fulmod=%d anymod=%d nomod=%d' % ((ck,) + tuple(int(counts[:, j].sum()) for j in range(3))))
            eng.close_contig()
        doc['kernel_ms'] = dict(zip(('parse', 'fill', 'class', 'format'), (round(v, 4) for v in eng.times())))
    finally:
        eng.close()
    doc['patterns'] = {which: os.path.join(out_folder, '%s.%s.*.txt' % (fileid, which)) for which in LISTS}
    with open(os.path.join(out_folder, fileid + '_bslabels.json'), 'w') as fh:
        json.dump(doc, fh, indent=1)
    for ln in doc['notes'] + report:
        print(ln, flush=True)
    print('getfeatures --motifORPos 2 --fulmod %r --anymod %r --nomod %r' % tuple(doc['patterns'][w] for w in LISTS), flush=True)
    doc['report'] = report
    doc['phase_s'] = phase
    return doc
