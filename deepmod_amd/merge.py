"""Per-chromosome merge of DeepMod BED files from several runs (counterpart of the reference's
/root/reference/DeepMod_tools/sum_chr_mod.py: readbed2 :37-46, mergeMod :48-54, save_mod :56-66, file discovery :77-84).

For one chromosome: every `*.<chr>-.<Base>.bed` and `*.<chr>+.<Base>.bed` one to three directory levels below the
prediction folder is read, coverage (column 10) and modified count (column 12) are summed per (chr, position, strand),
positions whose summed modified count is 0 are dropped, and the rest is written sorted by (chr, position, strand)
in the tool's own dialect (two spaces after the strand column, percentage = int(mod * 100 / cov)).
merge_beds / save_mod / sum_chr_mod are the host statement of that (numpy, no per-row Python dict) and the tool's own path.

`DeepMod.py merge` (merge_runs, DeviceMerge) does the same on one GPU: the text of every file is split into lines and parsed by
kernels (csrc/bedmerge.hip.inc), the records are added into two PositionSummary tables with integer atomics, the merged text is formatted on
the device and leaves it in bounded runs of whole tiles - byte for byte the file save_mod writes - and with --clusterCpG the tables go straight
into ClusterModel.sites.  A file with a line outside the device grammar is parsed by readbed2 and handed over as records.
"""
from __future__ import annotations

import glob
import os
from typing import Iterable, List

import numpy as np

from . import _lib


def find_bed_files(pred_folder: str, ck: str, base: str) -> List[str]:
    files: List[str] = []
    for strand in ('-', '+'):
        for depth in ('*/*/*/', '*/*/', '*/'):
            files.extend(glob.glob(os.path.join(pred_folder, '%s*.%s%s.%s.bed' % (depth, ck, strand, base))))
    return files


def readbed2(bedf: str):
    """-> (chrom str array, pos int64, strand str array, cov int64, mod int64)"""
    chrom, pos, strand, cov, mod = [], [], [], [], []
    with open(bedf) as mr:
        for line in mr:
            lsp = line.split()
            if not lsp:
                continue
            chrom.append(lsp[0])
            pos.append(int(lsp[1]))
            strand.append(lsp[5])
            cov.append(int(lsp[9]))
            mod.append(int(lsp[11]))
    return (np.array(chrom, dtype=object), np.array(pos, np.int64), np.array(strand, dtype=object),
            np.array(cov, np.int64), np.array(mod, np.int64))


def merge_beds(bed_files: Iterable[str]):
    parts = [readbed2(f) for f in bed_files]
    parts = [p for p in parts if len(p[1])]
    if not parts:
        e = np.zeros(0, np.int64)
        return np.zeros(0, object), e, np.zeros(0, object), e, e
    chrom = np.concatenate([p[0] for p in parts])
    pos = np.concatenate([p[1] for p in parts])
    strand = np.concatenate([p[2] for p in parts])
    cov = np.concatenate([p[3] for p in parts])
    mod = np.concatenate([p[4] for p in parts])
    # sort by the tuple (chr, pos, strand) the way Python sorts the reference's dict keys
    order = np.lexsort((strand.astype(str), pos, chrom.astype(str)))
    chrom, pos, strand, cov, mod = chrom[order], pos[order], strand[order], cov[order], mod[order]
    new = np.r_[True, (chrom[1:] != chrom[:-1]) | (pos[1:] != pos[:-1]) | (strand[1:] != strand[:-1])]
    heads = np.flatnonzero(new)
    return chrom[heads], pos[heads], strand[heads], np.add.reduceat(cov, heads), np.add.reduceat(mod, heads)


def save_mod(res_file: str, merged, base: str) -> int:
    chrom, pos, strand, cov, mod = merged
    keep = mod != 0
    with open(res_file, 'w') as mw:
        for c, p, s, cv, md in zip(chrom[keep], pos[keep].tolist(), strand[keep], cov[keep].tolist(), mod[keep].tolist()):
            mw.write('%s %d %d %s %d %s  %d %d 0,0,0 %d %d %d\n' % (c, p, p + 1, base, cv if cv < 1000 else 1000, s, p, p + 1, cv,
                                                                    int(md * 100 / cv) if cv > 0 else 0, md))
    return int(keep.sum())


def sum_chr_mod(pred_folder: str, base: str, sum_fileid: str, chrkeys=None, verbose: bool = True):
    """Merge every chromosome in chrkeys (default chr1..22, X, Y, M) -> {chr: output path}."""
    if chrkeys is None:
        chrkeys = ['chr%d' % i for i in range(1, 23)] + ['chrX', 'chrY', 'chrM']
    out = {}
    for ck in sorted(set(chrkeys)):
        files = find_bed_files(pred_folder, ck, base)
        if verbose:
            print("%s -+ %s: %d" % (ck, base, len(files)), flush=True)
        res_file = "%s/%s.%s.%s.bed" % (pred_folder, sum_fileid, ck, base)
        save_mod(res_file, merge_beds(files), base)
        out[ck] = res_file
    return out


# ---- `merge`: the same sums and the same file on one GPU (csrc/bedmerge.hip.inc) ---------------------------------------------
CHRKEYS = ['chr%d' % i for i in range(1, 23)] + ['chrX', 'chrY', 'chrM']
MAX_LENGTH = 2 ** 31 - 1                     # positions 0 .. 2^31 - 2: position + 1 is an int32
FORMAT_BUFFER = 64 << 20                     # bytes of merged text fetched per run of tiles (a tile is below 1 MB)


class MergeError(ValueError):
    pass


def parse_device_grammar(text: bytes, contig_name: str, table_length: int = -1):
    """The device's line routine compiled for the host (no GPU needed) -> ((pos, strand, cov, mod), flag, first bad line)."""
    import ctypes
    lib = _lib.load()
    flag, bad = ctypes.c_int32(0), ctypes.c_int64(-1)
    buf, name = ctypes.c_char_p(text), contig_name.encode('ascii')
    rows = lib.dm_bedmerge_parse_host(buf, len(text), name, table_length, None, None, None, None, 0, ctypes.byref(flag), ctypes.byref(bad))
    if rows < 0:
        _lib.check(int(rows))
    pos, cov, mod = (np.zeros(rows, np.int32) for _ in range(3))
    strand = np.zeros(rows, np.uint8)
    if rows:
        lib.dm_bedmerge_parse_host(buf, len(text), name, table_length, pos.ctypes.data, strand.ctypes.data, cov.ctypes.data, mod.ctypes.data, rows,
                                   ctypes.byref(flag), ctypes.byref(bad))
    return (pos, strand, cov, mod), flag.value, bad.value


def format_host(contig_name: str, base: str, cov_plus, mod_plus, cov_minus, mod_minus, first_pos: int = 0, cap=None) -> bytes:
    """The device's line routine compiled for the host: the merged text of positions first_pos .. from the four tables (a strand may be None).
    cap: the capacity offered (default: what the sizing call asks for); a text that does not fit raises."""
    import ctypes
    lib = _lib.load()
    tabs = [None if a is None else np.ascontiguousarray(a, np.int32) for a in (cov_plus, mod_plus, cov_minus, mod_minus)]
    length = max([len(a) for a in tabs if a is not None] + [0])
    ptrs = [None if a is None else a.ctypes.data for a in tabs]
    head = (contig_name.encode('ascii'), base.encode('ascii'), int(first_pos), length) + tuple(ptrs)
    lines = ctypes.c_int64(0)
    need = lib.dm_bedmerge_format_host(*head, None, 0, ctypes.byref(lines))
    if need < 0:
        _lib.check(int(need))
    cap = int(need) if cap is None else int(cap)
    out = np.empty(max(cap, 1), np.uint8)
    got = lib.dm_bedmerge_format_host(*head, out.ctypes.data, cap, ctypes.byref(lines))
    if got < 0:
        _lib.check(int(got))
    if got > cap:
        raise MergeError('merge: the text needs %d bytes, %d were offered' % (got, cap))
    return out[:got].tobytes()


def tile_positions() -> int:
    return _lib.load().dm_bedmerge_tile_positions()


class DeviceMerge(_lib.Handle):
    """One contig at a time on one GPU (dm_bedmerge_* of the C ABI): open, add_text / add_records per file, format, optionally the cluster stage on
    .plus / .minus (summary.PositionSummary, the handles ClusterModel.sites takes).  times(): ms of the parse / add / format kernels so far."""
    PREFIX, N_TIMES = 'dm_bedmerge', 3

    def __init__(self, device: int = 0):
        self.device = device
        self._create(device)
        self.plus = self.minus = None
        self._n = 0

    def close(self):
        self.close_contig()
        super().close()

    def close_contig(self):
        for s in (getattr(self, 'plus', None), getattr(self, 'minus', None)):
            if s is not None:
                s.close()
        self.plus = self.minus = None

    def open(self, contig_name: str, length=None):
        """Fresh tables for the contig.  length: the contig's (a line beyond it is outside the grammar); None: the tables grow with the files."""
        from . import summary
        self.close_contig()
        if length is not None and not 1 <= int(length) <= MAX_LENGTH:
            raise MergeError('merge: a contig of %d bases (1 to 2^31 - 1)' % int(length))
        n = 1 if length is None else int(length)
        self.plus, self.minus = summary.PositionSummary(n, self.device), summary.PositionSummary(n, self.device)
        self.name = contig_name
        self._n = 0
        self._libmod.check(self._lib.dm_bedmerge_open(self._h, self.plus._h, self.minus._h, contig_name.encode('ascii'), int(length is not None)))

    def _opened(self):
        if self.plus is None:                                         # (the C handle still names the tables close_contig destroyed)
            raise MergeError('merge: no contig is open')

    def _lengths(self):
        for s in (self.plus, self.minus):
            s.length = int(self._lib.dm_summary_length(s._h))

    def add_text(self, text: bytes):
        """-> (lines, flag, first bad line (1-based, -1: none)); a flagged text adds nothing."""
        self._opened()
        ct = self._ct
        rows, flag, bad = ct.c_int64(0), ct.c_int32(0), ct.c_int64(-1)
        try:
            self._libmod.check(self._lib.dm_bedmerge_add_text(self._h, ct.c_char_p(text), len(text), ct.byref(rows), ct.byref(flag), ct.byref(bad)))
        finally:
            self._lengths()
        self._n = 0 if flag.value else rows.value
        return rows.value, flag.value, bad.value

    def add_records(self, pos, strand, cov, mod):
        r = (np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(strand, np.uint8), np.ascontiguousarray(cov, np.int32), np.ascontiguousarray(mod, np.int32))
        self._opened()
        if len({len(a) for a in r}) != 1:
            raise MergeError('merge: record arrays of different lengths')
        try:
            self._libmod.check(self._lib.dm_bedmerge_add_records(self._h, len(r[0]), *[a.ctypes.data for a in r]))
        finally:
            self._lengths()
        self._n = len(r[0])

    def records(self):
        """(pos, strand, cov, mod) of the last add_text / add_records as they lie on the device."""
        n = self._n
        pos, cov, mod = (np.zeros(n, np.int32) for _ in range(3))
        strand = np.zeros(n, np.uint8)
        self._libmod.check(self._lib.dm_bedmerge_fetch_records(self._h, pos.ctypes.data, strand.ctypes.data, cov.ctypes.data, mod.ctypes.data))
        return pos, strand, cov, mod

    def format_begin(self, base: str):
        """-> (lines, bytes, bytes of the largest tile: the smallest buffer format_next takes)."""
        self._opened()
        ct = self._ct
        lines, nbytes, largest = ct.c_int64(0), ct.c_int64(0), ct.c_int64(0)
        self._libmod.check(self._lib.dm_bedmerge_format_begin(self._h, base.encode('ascii'), ct.byref(lines), ct.byref(nbytes), ct.byref(largest)))
        return lines.value, nbytes.value, largest.value

    def format_next(self, buf: np.ndarray, cap=None):
        """-> (more, the bytes as a view of buf)."""
        self._opened()
        got = self._ct.c_int64(0)
        rc = self._lib.dm_bedmerge_format_next(self._h, buf.ctypes.data, len(buf) if cap is None else int(cap), self._ct.byref(got))
        if rc < 0:
            self._libmod.check(int(rc))
        return rc == 1, buf[:got.value]

    def format(self, base: str, cap: int = FORMAT_BUFFER):
        """The merged text in position order, as views of ONE buffer of `cap` bytes (use each before asking for the next); .formatted = (lines,
        bytes) of the whole text."""
        lines, nbytes, _ = self.format_begin(base)
        self.formatted = (lines, nbytes)
        if nbytes == 0:
            return
        buf = np.empty(max(int(cap), 1), np.uint8)
        more = True
        while more:
            more, part = self.format_next(buf)
            yield part


def host_rows(path: str, contig_name: str, limit: int):
    """A file the device parser passed on: readbed2's rows as records, if they meet the conditions of the device grammar; else MergeError
    `file:line: reason`."""
    with open(path) as fh:
        numbered = [(no, line.split()) for no, line in enumerate(fh, 1)]
    numbered = [(no, lsp) for no, lsp in numbered if lsp]
    for no, lsp in numbered:                                          # what readbed2 would stop at with a bare IndexError / ValueError
        if len(lsp) < 12:
            raise MergeError('%s:%d: %d fields, a mod_pos BED line has at least 12' % (path, no, len(lsp)))
        for k in (1, 9, 11):
            try:
                int(lsp[k])
            except ValueError as exc:
                raise MergeError('%s:%d: %s' % (path, no, exc))
    chrom, pos, strand, cov, mod = readbed2(path)
    assert len(pos) == len(numbered)
    line_of = [no for no, _ in numbered]

    def stop(bad, reason):
        if bad.any():
            i = int(np.argmax(bad))
            raise MergeError('%s:%d: %s' % (path, line_of[i], reason(i)))

    stop(chrom != contig_name, lambda i: 'a line of %s in a file named for %s' % (chrom[i], contig_name))
    stop((strand != '+') & (strand != '-'), lambda i: 'strand %r' % (strand[i],))
    stop((pos < 0) | (cov < 0) | (mod < 0) | (cov > 2 ** 31 - 1) | (mod > cov),
         lambda i: 'position %d, coverage %d, modified %d: outside 0 <= modified <= coverage < 2^31' % (pos[i], cov[i], mod[i]))
    stop(pos >= limit, lambda i: 'position %d is not on %s (%d %s)' % (pos[i], contig_name, limit, 'bases' if limit < MAX_LENGTH else 'positions at most'))
    return pos.astype(np.int32), (strand == '-').astype(np.uint8), cov.astype(np.int32), mod.astype(np.int32)


def check_options(mo):
    """What can be refused before any BED file is read or any GPU asked for -> (contigs, cluster checkpoint prefix or None, {contig: bases} of --Ref)."""
    folder = mo.get('predFolder')
    if not folder or not os.path.isdir(folder):
        raise MergeError('merge: --predFolder: the folder of the runs does not exist (%s)' % folder)
    chrkeys = sorted(set(mo.get('chr') or CHRKEYS))
    ref = mo.get('Ref')
    if ref and not os.path.isfile(ref):
        raise MergeError('merge: --Ref: reference file does not exist (%s)' % ref)
    prefix = None
    if mo.get('clusterCpG') is not None:
        if mo.get('Base') != 'C':
            raise MergeError('merge: --clusterCpG: the CpG-cluster stage is defined for --Base C only (got --Base %s)' % mo.get('Base'))
        if not ref:
            raise MergeError('merge: --clusterCpG: needs --Ref, the reference FASTA whose CG positions are the sites')
        prefix = mo['clusterCpG'] or os.environ.get('DEEPMOD_CLUSTER_MODEL') or ''
        if not prefix:
            raise MergeError('merge: --clusterCpG: no cluster-model checkpoint: give its prefix after the flag or set DEEPMOD_CLUSTER_MODEL')
        if not os.path.isfile(prefix + '.index'):
            raise MergeError('merge: --clusterCpG: no cluster-model checkpoint at %r (no %s.index)' % (prefix, prefix))
    fasta = {}
    if ref:
        from . import siteperf
        fasta = siteperf.read_fasta(ref)
        missing = [ck for ck in chrkeys if ck not in fasta]
        if prefix and missing:
            raise MergeError('merge: --clusterCpG: %s holds no contig %s (name the contigs with --chr)' % (ref, ', '.join(missing)))
    return chrkeys, prefix, fasta


def merge_runs(mo, device: int = 0):
    """The command.  mo: predFolder, Base, FileID, chr (list of contigs; None: chr1..22, X, Y, M), Ref (None: the tables grow with the files),
    clusterCpG (None: no cluster stage; '' : DEEPMOD_CLUSTER_MODEL; else the checkpoint prefix), threads.
    Writes <predFolder>/<FileID>.<chr>.<Base>.bed per contig, <FileID>_clusterCpG.<chr>.C.bed per contig with a site, <FileID>_merge.json.
    -> the JSON document."""
    import json
    from concurrent.futures import ThreadPoolExecutor
    chrkeys, prefix, fasta = check_options(mo)
    folder, base, fileid = mo['predFolder'], str(mo['Base']), str(mo.get('FileID') or 'mod')
    if _lib.load().dm_device_count() < 1:
        raise MergeError('no gfx950 GPU visible (this build has no CPU path)')
    from . import cluster, tables
    dev = DeviceMerge(device)
    model = cluster.ClusterModel.from_checkpoint(prefix, device) if prefix else None
    doc = {'inputs': {'predFolder': folder, 'Base': base, 'FileID': fileid, 'chr': chrkeys, 'Ref': mo.get('Ref'), 'clusterCpG': prefix}, 'contigs': {}}
    out = {}
    try:
        with ThreadPoolExecutor(max(int(mo.get('threads') or 1), 1)) as pool:
            for ck in chrkeys:
                files = find_bed_files(folder, ck, base)
                res_file = '%s/%s.%s.%s.bed' % (folder, fileid, ck, base)
                entry = {'files': files, 'lines_read': 0, 'lines_written': 0, 'bytes_written': 0, 'notes': []}
                before = dev.times()
                if files:
                    seq = fasta.get(ck)
                    dev.open(ck, len(seq) if seq is not None else None)
                    entry['lines_read'] = tables.fill(dev, files, pool, ck, len(seq) if seq is not None else MAX_LENGTH, entry['notes'])
                    with open(res_file, 'wb') as fh:
                        for part in dev.format(base):
                            fh.write(part)
                    entry['lines_written'], entry['bytes_written'] = dev.formatted
                    if model is not None:
                        res = model.sites(dev.plus, dev.minus, seq)
                        entry['sites'] = int(len(res['pos']))
                        if len(res['pos']):
                            cpath = '%s/%s_clusterCpG.%s.C.bed' % (folder, fileid, ck)
                            with open(cpath, 'wb') as fh:
                                fh.write(b''.join(cluster.site_text_parts(ck, base, res)))
                            entry['cluster_file'] = cpath
                    dev.close_contig()
                else:
                    open(res_file, 'wb').close()                                       # sum_chr_mod.py writes an empty file
                    if model is not None:
                        entry['sites'] = 0
                after = dev.times()
                entry['kernel_ms'] = dict(zip(('parse', 'add', 'format'), (round(b - a, 4) for a, b in zip(before, after))))
                doc['contigs'][ck] = entry
                out[ck] = res_file
                print('%s -+ %s: %d files, %d lines read, %d written%s' % (ck, base, len(files), entry['lines_read'], entry['lines_written'],
                                                                          '' if model is None else ', %d CpG sites' % entry['sites']), flush=True)
    finally:
        if model is not None:
            model.close()
        dev.close()
    doc['outputs'] = out
    with open('%s/%s_merge.json' % (folder, fileid), 'w') as fh:
        json.dump(doc, fh, indent=1)
    return doc
