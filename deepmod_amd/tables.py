"""What the table commands share (`merge`, `bsperf`, `motifs`, both tests of `diffmod`): the stranded BED files below a folder and their contigs,
the contigs and lengths of a run from --Ref / --chr / the file names, the host twin of the per-strand tables merge.DeviceMerge fills, the role-keyed
DeviceMerge handles of a device engine, and the read-ahead loop that sums a contig's files into either kind of tables.  The refusals
of this module are TableError without a command's name; a command puts its own in front where it catches them."""
from __future__ import annotations

import glob
import os
import re
from typing import List, Optional

import numpy as np

from . import merge

MAX_LENGTH = merge.MAX_LENGTH


class TableError(ValueError):
    pass


def stranded_beds(folder: str, base: str) -> List[str]:
    """Every *.<contig>+.<Base>.bed / *.<contig>-.<Base>.bed one to three levels below the folder, of whatever contig."""
    found = []
    for depth in ('*/*/*/', '*/*/', '*/'):
        found.extend(glob.glob(os.path.join(folder, '%s*.%s.bed' % (depth, base))))
    return [p for p in found if re.search(r'\.[^/.]*[+-]\.%s\.bed$' % re.escape(base), p)]


def contigs_of(folder: str, base: str) -> List[str]:
    return sorted({re.search(r'\.([^/.]*)[+-]\.%s\.bed$' % re.escape(base), path).group(1) for path in stranded_beds(folder, base)})


def contigs(ref, named, base: str, folders: List[str]):
    """-> (contigs, {contig: length or None}, {contig: bases} of --Ref) from --Ref and --chr, or from the file names below `folders`."""
    from . import siteperf
    if ref and not os.path.isfile(ref):
        raise TableError('--Ref: reference file does not exist (%s)' % ref)
    fasta = siteperf.read_fasta(ref) if ref else {}
    named = list(named or [])
    missing = [ck for ck in named if ck not in fasta] if ref else []
    if missing:
        raise TableError('--chr: %s holds no contig %s' % (ref, ', '.join(missing)))
    chrkeys = named or list(fasta) or sorted({ck for f in folders for ck in contigs_of(f, base)})
    lengths = {ck: (len(fasta[ck]) if ck in fasta else None) for ck in chrkeys}
    for ck in chrkeys:
        if lengths[ck] is not None and not 1 <= lengths[ck] <= MAX_LENGTH:
            raise TableError('--Ref: contig %s has %d bases (1 to 2^31 - 1)' % (ck, lengths[ck]))
    return chrkeys, lengths, fasta


class HostTables:
    """The two tables of a contig on the host, filled as merge.DeviceMerge fills its own: add_text is the device's line routine compiled for the host
    (merge.parse_device_grammar: a text with a line outside the grammar adds nothing and is flagged), add_records takes a host parse.  .plus / .minus:
    (coverage, modified) int64 arrays; length None: they grow with the files."""

    def __init__(self, name: str, length: Optional[int]):
        self.name, self.fixed = name, length is not None
        self.length = int(length) if self.fixed else 1
        self.plus = (np.zeros(self.length, np.int64), np.zeros(self.length, np.int64))
        self.minus = (np.zeros(self.length, np.int64), np.zeros(self.length, np.int64))
        self.cov_bound = 0

    def close(self):
        pass

    def add_text(self, text: bytes):
        rec, flag, bad = merge.parse_device_grammar(text, self.name, self.length if self.fixed else -1)
        if not flag:
            self.add_records(*rec)
        return len(rec[0]), flag, bad

    def add_records(self, pos, strand, cov, mod):
        pos, strand, cov, mod = (np.asarray(a).astype(np.int64) for a in (pos, strand, cov, mod))
        if len(pos) == 0:
            return
        if not self.fixed and int(pos.max()) >= self.length:
            self.length = int(pos.max()) + 1
            self.plus = tuple(np.concatenate([a, np.zeros(self.length - len(a), np.int64)]) for a in self.plus)
            self.minus = tuple(np.concatenate([a, np.zeros(self.length - len(a), np.int64)]) for a in self.minus)
        if (pos < 0).any() or (pos >= self.length).any() or (mod < 0).any() or (mod > cov).any():
            raise TableError('a record outside the contig or outside 0 <= modified <= coverage')
        self.cov_bound += int(cov.max())
        if self.cov_bound >= 2 ** 31:
            raise TableError('the largest coverages of this contig\'s files sum to %d (2^31 or more): the int32 tables cannot hold them' % self.cov_bound)
        for s, tab in enumerate((self.plus, self.minus)):
            sel = strand == s
            np.add.at(tab[0], pos[sel], cov[sel])
            np.add.at(tab[1], pos[sel], mod[sel])


class MergeHandles:
    """For a device engine (with .device): one merge.DeviceMerge per role, kept over the contigs and closed with the engine."""

    def new_tables(self, role: str, name: str, length: Optional[int]):
        """Fresh tables for the contig in the merge handle kept for `role` (the tables of the contig before are closed); length None: they grow."""
        handles = self.__dict__.setdefault('_merge', {})
        if role not in handles:
            handles[role] = merge.DeviceMerge(self.device)
        handles[role].open(name, None if length is None else int(length))
        return handles[role]

    def close(self):
        for dm in self.__dict__.pop('_merge', {}).values():
            dm.close()
        super().close()


def read(path: str) -> bytes:
    with open(path, 'rb') as fh:
        return fh.read()


def fill(tables, paths, pool, name: str, limit: int, notes: List[str]) -> int:
    """The files of one contig into the tables (merge.DeviceMerge or HostTables): the device grammar first, the host parse for a text outside it, which
    is noted.  The pool's threads read ahead.  merge.MergeError (`file:line: reason`) and the tables' own ValueError / RuntimeError pass through, the
    failing file in their .path.  -> lines read"""
    total = 0
    for path, text in zip(paths, pool.map(read, paths)):
        try:
            lines, flag, bad = tables.add_text(text)
            if flag:
                notes.append('%s: line %d is outside the device grammar: the file is parsed on the host' % (path, bad))
                rec = merge.host_rows(path, name, limit)
                tables.add_records(*rec)
                lines = len(rec[0])
        except (ValueError, RuntimeError) as exc:
            exc.path = path
            raise
        total += int(lines)
    return total
