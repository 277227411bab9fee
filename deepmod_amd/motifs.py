"""`motifs`: in which sequence contexts are the modified bases?  De novo motif discovery from a `detect` run and, optionally, control runs
(DESIGN.md 20).  Every other offline command takes the motif from the user (getfeatures --motif, siteperf --motif, bslabels --motif); this one
finds it.  The selection rule below is this project's own, as bslabels' `anymod` is: the reference ships no such tool.

Counting (one sweep per contig: HostEngine here, csrc/motifs.hip.inc on the GPU).  Options: flank (U, D) bases upstream / downstream of the modified
base, 0 <= U, D, U + D <= 8; base; cov c >= 1; min_pct t and max_ctrl_pct u in 0..100.  One contig: its bytes as handed over (the engine does not
change case; the command upper-cases them, as bslabels does), the sample's '+' and '-' tables (coverage, modified count per position) and
optionally the pooled controls' tables, every table of exactly the contig's length.  Each key (strand s, position p) is examined once, and the
first rule that applies decides:
  1  the oriented letter (seq[p] on '+', its complement on '-') is not `base`: off_base if the sample's coverage is > 0 (a BED line on a letter
     the reference does not have there: a wrong --Ref), else ignored
  2  the oriented context, offsets -U..-1 and +1..+D ('+': seq[p + j]; '-': the complement of seq[p - j]), leaves the contig or holds a byte other
     than A, C, G, T: edge
  3  sample coverage < c: shallow (deletion-only positions, coverage 0, land here)
  4  controls are given and their pooled coverage < c: no_control
  5  tested[ctx] += 1; if also 100 mod // cov >= t and (no controls or 100 cmod // ccov <= u): modified[ctx] += 1
The context index ctx has its most significant base-4 digit at offset -U, A < C < G < T.  Results accumulate over contigs until reset: hist int64
[4^(U+D)][2] (tested, modified), counters int64 [2 strands][5] (COUNT_KEYS), off_base [2].

Search (pattern_counts, find_motifs: numpy int64 on the host, no float decides anything).  A pattern gives each of the U + D flank offsets one of
A, C, G, T, N; its counts n, m are the sums of hist over the contexts it matches.  Repeatedly: among the patterns with m >= min_sites and
100 m >= min_frac n take the one with the fewest fixed letters (ties: larger m, larger n, smaller pattern index - digits A < C < G < T < N, most
significant at -U), emit it, zero every context it matches.  Known weakness: on a genome of very skewed composition a general pattern can win over
the specific one, because nothing weighs a pattern against the composition of the genome.
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import numpy as np

from . import _lib, merge, tables

MAX_FLANK = 8
MAX_LENGTH = merge.MAX_LENGTH
COUNT_KEYS = ('tested', 'modified', 'shallow', 'no_control', 'edge')
LETTERS = 'ACGT'
_CODE = np.full(256, 4, np.uint8)                    # A 0, C 1, G 2, T 3 (upper case only), anything else 4; the complement of code c is 3 - c
for _i, _c in enumerate(LETTERS):
    _CODE[ord(_c)] = _i


class MotifsError(ValueError):
    pass


def check_engine_options(up, down, base, cov, min_pct, max_ctrl_pct) -> None:
    if not (0 <= int(up) <= MAX_FLANK and 0 <= int(down) <= MAX_FLANK and int(up) + int(down) <= MAX_FLANK):
        raise MotifsError('motifs: --flank: 0 to %d bases upstream and downstream, %d in all at most (got %s,%s)' % (MAX_FLANK, MAX_FLANK, up, down))
    if not isinstance(base, str) or len(base) != 1 or base not in LETTERS:
        raise MotifsError('motifs: --Base: one of A, C, G, T (got %r)' % (base,))
    if int(cov) < 1 or int(cov) > 2 ** 31 - 1:
        raise MotifsError('motifs: --cov: the least coverage is 1 or more (got %s)' % cov)
    if not 0 <= int(min_pct) <= 100:
        raise MotifsError('motifs: --minPct: a percentage, 0 to 100 (got %s)' % min_pct)
    if not 0 <= int(max_ctrl_pct) <= 100:
        raise MotifsError('motifs: --maxCtrlPct: a percentage, 0 to 100 (got %s)' % max_ctrl_pct)


def _seq_array(seq) -> np.ndarray:
    return np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, np.uint8)


class HostEngine:
    """The semantics in numpy, one contig per count().  A table is a pair (coverage, modified) of integer arrays of the contig's length."""

    def __init__(self, up: int = 3, down: int = 3, base: str = 'A', cov: int = 5, min_pct: int = 50, max_ctrl_pct: int = 10):
        check_engine_options(up, down, base, cov, min_pct, max_ctrl_pct)
        self.up, self.down, self.base, self.cov, self.min_pct, self.max_ctrl_pct = int(up), int(down), base, int(cov), int(min_pct), int(max_ctrl_pct)
        self.bins = 4 ** (self.up + self.down)
        self.reset()

    def close(self):
        pass

    def reset(self):
        self.hist = np.zeros((self.bins, 2), np.int64)
        self.counters = np.zeros((2, len(COUNT_KEYS)), np.int64)
        self.off_base = np.zeros(2, np.int64)

    def new_tables(self, role: str, name: str, length: int) -> tables.HostTables:
        return tables.HostTables(name, length)

    def count(self, seq, plus, minus, ctrl_plus=None, ctrl_minus=None) -> Tuple[np.ndarray, np.ndarray]:
        """-> (counters [2][5], off_base [2]) of this contig; hist, counters and off_base of the engine grow by them."""
        s = _seq_array(seq)
        n = len(s)
        if (ctrl_plus is None) != (ctrl_minus is None):
            raise MotifsError('motifs: the controls are given by both of their tables or by neither')
        tabs = [plus, minus] + ([ctrl_plus, ctrl_minus] if ctrl_plus is not None else [])
        if any(t is None for t in tabs[:2]):
            raise MotifsError('motifs: two sample tables, one per strand')
        tabs = [(np.asarray(t[0]).astype(np.int64), np.asarray(t[1]).astype(np.int64)) for t in tabs]
        for t in tabs:
            if len(t[0]) != n or len(t[1]) != n:
                raise MotifsError('motifs: a table of %d positions for a contig of %d' % (len(t[0]), n))
        code = _CODE[s].astype(np.int64)
        own = LETTERS.index(self.base)
        counters, off_base = np.zeros((2, len(COUNT_KEYS)), np.int64), np.zeros(2, np.int64)
        for strand in range(2):
            cov, mod = tabs[strand]
            is_base = code == (3 - own if strand else own)
            off_base[strand] = int((~is_base & (cov > 0)).sum())
            p = np.nonzero(is_base)[0]
            ctx, bad = np.zeros(len(p), np.int64), np.zeros(len(p), bool)
            for j in [j for j in range(-self.up, self.down + 1) if j != 0]:
                q = p - j if strand else p + j
                inside = (q >= 0) & (q < n)
                v = np.where(inside, code[np.clip(q, 0, max(n - 1, 0))], 4)
                bad |= v == 4
                ctx = ctx * 4 + (3 - (v & 3) if strand else v & 3)
            cv, md = cov[p], mod[p]
            shallow = ~bad & (cv < self.cov)
            rest = ~bad & ~shallow
            if ctrl_plus is not None:
                ccv, cmd = tabs[2 + strand][0][p], tabs[2 + strand][1][p]
                no_control = rest & (ccv < self.cov)
                quiet = (100 * cmd) // np.maximum(ccv, 1) <= self.max_ctrl_pct
            else:
                no_control, quiet = np.zeros(len(p), bool), np.ones(len(p), bool)
            tested = rest & ~no_control
            modified = tested & ((100 * md) // np.maximum(cv, 1) >= self.min_pct) & quiet
            np.add.at(self.hist[:, 0], ctx[tested], 1)
            np.add.at(self.hist[:, 1], ctx[modified], 1)
            counters[strand] = [int(tested.sum()), int(modified.sum()), int(shallow.sum()), int(no_control.sum()), int(bad.sum())]
        self.counters += counters
        self.off_base += off_base
        return counters, off_base

    def fetch(self) -> np.ndarray:
        return self.hist.copy()

    def times(self) -> Tuple[float, float]:
        return 0.0, 0.0


def tile_positions() -> int:
    return _lib.load().dm_motifs_tile_positions()


def count_host_routine(up, down, base, cov, min_pct, max_ctrl_pct, seq, plus, minus, ctrl_plus=None, ctrl_minus=None):
    """The sweep compiled for the host (dm_motifs_count_host: the routine the kernel runs per key; no GPU needed) -> (hist, counters, off_base)."""
    lib = _lib.load()
    s = _seq_array(seq)
    tabs = [plus, minus] + ([ctrl_plus, ctrl_minus] if ctrl_plus is not None else [])
    arrs = [np.ascontiguousarray(a, np.int32) for t in tabs for a in t]
    ptrs = [a.ctypes.data for a in arrs] + [None] * (8 - len(arrs))
    hist = np.zeros((4 ** (up + down), 2), np.int64)
    counters, off_base = np.zeros((2, len(COUNT_KEYS)), np.int64), np.zeros(2, np.int64)
    _lib.check(lib.dm_motifs_count_host(up, down, base.encode('ascii'), cov, min_pct, max_ctrl_pct, s.ctypes.data, len(s), *ptrs, hist.ctypes.data, counters.ctypes.data,
                                        off_base.ctypes.data))
    return hist, counters, off_base


class DeviceEngine(tables.MergeHandles, _lib.Handle):
    """The same on one GPU (dm_motifs_* of the C ABI).  A table is a summary.PositionSummary (the handles merge.DeviceMerge fills).
    times(): ms of the uploads of the contigs' bytes / of the sweeps so far."""
    PREFIX, N_TIMES = 'dm_motifs', 2

    def __init__(self, up: int = 3, down: int = 3, base: str = 'A', cov: int = 5, min_pct: int = 50, max_ctrl_pct: int = 10, device: int = 0):
        check_engine_options(up, down, base, cov, min_pct, max_ctrl_pct)
        self.up, self.down, self.base, self.device = int(up), int(down), base, device
        self.bins = 4 ** (self.up + self.down)
        self._create(device, self.up, self.down, base.encode('ascii'), int(cov), int(min_pct), int(max_ctrl_pct))
        self.counters = np.zeros((2, len(COUNT_KEYS)), np.int64)
        self.off_base = np.zeros(2, np.int64)

    def count(self, seq, plus, minus, ctrl_plus=None, ctrl_minus=None) -> Tuple[np.ndarray, np.ndarray]:
        s = _seq_array(seq)
        counters, off_base = np.zeros((2, len(COUNT_KEYS)), np.int64), np.zeros(2, np.int64)
        hs = [None if t is None else t._h for t in (plus, minus, ctrl_plus, ctrl_minus)]
        self._libmod.check(self._lib.dm_motifs_count(self._h, s.ctypes.data, len(s), *hs, counters.ctypes.data, off_base.ctypes.data))
        self.counters += counters
        self.off_base += off_base
        return counters, off_base

    def fetch(self) -> np.ndarray:
        hist = np.zeros((self.bins, 2), np.int64)
        self._libmod.check(self._lib.dm_motifs_fetch(self._h, hist.ctypes.data))
        return hist

    def reset(self):
        self._libmod.check(self._lib.dm_motifs_reset(self._h))
        self.counters[:] = 0
        self.off_base[:] = 0


# ---- the search ----------------------------------------------------------------------------------------------------------------------------

def pattern_counts(hist, up: int, down: int) -> np.ndarray:
    """int64 [5^(U+D)][2]: (n, m) of every pattern, from one summation per axis.  A pattern's index has base-5 digits A 0, C 1, G 2, T 3, N 4, the
    most significant at offset -U."""
    L = int(up) + int(down)
    h = np.asarray(hist, np.int64).reshape((4,) * L + (2,))
    for axis in range(L):
        h = np.concatenate([h, h.sum(axis=axis, keepdims=True)], axis=axis)
    return h.reshape(5 ** L, 2)


def pattern_digits(index: int, L: int) -> List[int]:
    digits = []
    for _ in range(L):
        digits.append(index % 5)
        index //= 5
    return digits[::-1]


def motif_of(digits, up: int, base: str) -> Tuple[str, int, str]:
    """The flank digits of a pattern (offsets -U..-1, +1..+D) -> (the motif with its outer Ns trimmed and the interior ones kept, ModinMotif: the index
    of the modified base in it, the mixed-case label of the reference's documents, e.g. gAtc)."""
    letters = [(LETTERS + 'N')[d] for d in digits]
    left, right = letters[:up], letters[up:]
    while left and left[0] == 'N':
        left = left[1:]
    while right and right[-1] == 'N':
        right = right[:-1]
    motif, k = ''.join(left) + base + ''.join(right), len(left)
    return motif, k, motif[:k].lower() + base + motif[k + 1:].lower()


def context_string(index: int, up: int, down: int, base: str) -> str:
    """A context index -> its letters, the base upper-case in lower-case flanks."""
    digits = []
    for _ in range(up + down):
        digits.append(index % 4)
        index //= 4
    flank = ''.join(LETTERS[d].lower() for d in digits[::-1])
    return flank[:up] + base + flank[up:]


def find_motifs(hist, up: int, down: int, min_sites: int = 20, min_frac: int = 50, max_motifs: int = 8, base: str = 'A') -> List[Dict[str, object]]:
    """The selection rule of the module's docstring -> [{motif, ModinMotif, label, sites, modified, pass, pattern}] in the order found."""
    L = int(up) + int(down)
    h = np.array(hist, np.int64).reshape((4,) * L + (2,))
    idx = np.arange(5 ** L, dtype=np.int64)
    fixed = np.zeros(5 ** L, np.int64)                                # fixed letters of every pattern, digit by digit
    for _ in range(L):
        fixed += (idx % 5) != 4
        idx //= 5
    index = np.arange(5 ** L, dtype=np.int64)
    out = []
    while len(out) < int(max_motifs):
        pc = pattern_counts(h, up, down)
        n, m = pc[:, 0], pc[:, 1]
        cand = np.nonzero((m >= int(min_sites)) & (100 * m >= int(min_frac) * n))[0]
        if len(cand) == 0:
            break
        best = int(cand[np.lexsort((index[cand], -n[cand], -m[cand], fixed[cand]))[0]])
        digits = pattern_digits(best, L)
        motif, k, label = motif_of(digits, up, base)
        out.append({'motif': motif, 'ModinMotif': k, 'label': label, 'sites': int(n[best]), 'modified': int(m[best]), 'pass': len(out) + 1, 'pattern': best})
        h[tuple(slice(None) if d == 4 else d for d in digits)] = 0
    return out


# ---- the command ----------------------------------------------------------------------------------------------------------------------------

def parse_flank(value) -> Tuple[int, int]:
    if isinstance(value, (tuple, list)) and len(value) == 2:
        return int(value[0]), int(value[1])
    try:
        u, d = (int(v) for v in str(value).split(','))
    except ValueError:
        raise MotifsError('motifs: --flank: two numbers of bases, upstream,downstream (got %r)' % (value,))
    return u, d


def check_options(mo: Dict[str, object]):
    """What can be refused before a BED file is read or any GPU asked for -> (options dict, contigs, {contig: upper-cased bases},
    {contig: sample files}, {contig: control files})."""
    base = str(mo.get('Base') or 'A')
    up, down = parse_flank(mo.get('flank') or (3, 3))
    o = {'Base': base, 'flank': [up, down], 'cov': int(mo.get('cov', 5)), 'minPct': int(mo.get('minPct', 50)), 'maxCtrlPct': int(mo.get('maxCtrlPct', 10)),
         'minFrac': int(mo.get('minFrac', 50)), 'minSites': int(mo.get('minSites', 20)), 'maxMotifs': int(mo.get('maxMotifs', 8))}
    check_engine_options(up, down, base, o['cov'], o['minPct'], o['maxCtrlPct'])
    if not 0 <= o['minFrac'] <= 100:
        raise MotifsError('motifs: --minFrac: a percentage, 0 to 100 (got %d)' % o['minFrac'])
    if o['minSites'] < 1:
        raise MotifsError('motifs: --minSites: 1 or more (got %d)' % o['minSites'])
    if not 1 <= o['maxMotifs'] <= 64:
        raise MotifsError('motifs: --maxMotifs: 1 to 64 (got %d)' % o['maxMotifs'])
    folder = mo.get('predFolder')
    if not folder or not os.path.isdir(folder):
        raise MotifsError('motifs: --predFolder: the folder of the sample\'s runs does not exist (%s)' % folder)
    controls = [c for c in (mo.get('control') or []) if c]
    for c in controls:
        if not os.path.isdir(c):
            raise MotifsError('motifs: --control: no folder %s' % c)
    ref, named = mo.get('Ref'), list(mo.get('chr') or [])
    if not ref:
        raise MotifsError('motifs: --Ref: the reference FASTA is needed (the sequence contexts are read from it)')
    try:
        chrkeys, _, fasta = tables.contigs(ref, named, base, [])
    except tables.TableError as exc:
        raise MotifsError('motifs: %s' % exc)
    if not chrkeys:
        raise MotifsError('motifs: --Ref: %s holds no contig' % ref)
    files = {ck: sorted(merge.find_bed_files(folder, ck, base)) for ck in chrkeys}          # (sorted: the order of the notes)
    ctrl_files = {ck: [p for c in controls for p in sorted(merge.find_bed_files(c, ck, base))] for ck in chrkeys}
    if not named:                                                     # a file of a contig the reference does not hold: the wrong --Ref
        for fld, by_contig in [(folder, files)] + [(c, ctrl_files) for c in controls]:
            known = {p for ps in by_contig.values() for p in ps}
            other = sorted(p for p in tables.stranded_beds(fld, base) if p not in known)
            if other:
                raise MotifsError('motifs: --Ref: %s is the file of a contig that %s does not hold' % (other[0], ref))
    if not any(files.values()):
        raise MotifsError('motifs: --predFolder: no *.<chr>+.%s.bed / *.<chr>-.%s.bed one to three levels below %s' % (base, base, folder))
    if controls and not any(ctrl_files.values()):
        raise MotifsError('motifs: --control: no *.<chr>+.%s.bed / *.<chr>-.%s.bed one to three levels below %s' % (base, base, ', '.join(controls)))
    seqs = {ck: fasta[ck].upper() for ck in chrkeys}
    return o, chrkeys, seqs, files, ctrl_files


def report_text(motifs: List[Dict[str, object]]) -> str:
    rows = ['rank\tmotif\tModinMotif\tlabel\tsites\tmodified\tpercent\targuments']
    for rank, mt in enumerate(motifs, 1):
        args = '-' if 'N' in mt['motif'] else '--motif %s --ModinMotif %d' % (mt['label'], mt['ModinMotif'])
        rows.append('%d\t%s\t%d\t%s\t%d\t%d\t%d\t%s' % (rank, mt['motif'], mt['ModinMotif'], mt['label'], mt['sites'], mt['modified'],
                                                        100 * mt['modified'] // max(mt['sites'], 1), args))
    return ''.join(r + '\n' for r in rows)


def motifs(mo: Dict[str, object], engine=None) -> Dict[str, object]:
    """The command.  mo: predFolder, control (list of folders; empty: none), Ref, Base, outFolder, FileID, chr (list; None: every contig of the FASTA),
    flank ('U,D' or a pair), cov, minPct, maxCtrlPct, minFrac, minSites, maxMotifs, threads.  engine: an object with HostEngine's interface
    (default: DeviceEngine on GPU 0), made with the same options.  Writes <outFolder>/<FileID>_motifs.txt / _motifs.json -> the JSON document."""
    import json
    from concurrent.futures import ThreadPoolExecutor
    o, chrkeys, seqs, files, ctrl_files = check_options(mo)
    base, (up, down) = o['Base'], o['flank']
    controls = [c for c in (mo.get('control') or []) if c]
    own = engine is None
    if own:
        if _lib.load().dm_device_count() < 1:
            raise MotifsError('no gfx950 GPU visible (this build has no CPU path)')
        engine = DeviceEngine(up, down, base, o['cov'], o['minPct'], o['maxCtrlPct'])
    elif (engine.up, engine.down, engine.base) != (up, down, base):
        raise MotifsError('motifs: the engine was made for flank %d,%d base %s' % (engine.up, engine.down, engine.base))

    notes: List[str] = []
    doc = {'inputs': dict(o, predFolder=mo['predFolder'], control=controls, Ref=mo['Ref'], chr=chrkeys, FileID=str(mo.get('FileID') or 'mod'),
                          files=[p for ck in chrkeys for p in files[ck]], control_files=[p for ck in chrkeys for p in ctrl_files[ck]]),
           'contigs': {}}
    try:
        engine.reset()
        with ThreadPoolExecutor(max(int(mo.get('threads') or 1), 1)) as pool:
            for ck in chrkeys:
                if not files[ck]:
                    continue
                seq, n = seqs[ck], len(seqs[ck])
                entry = {'length': n, 'files': len(files[ck]), 'control_files': len(ctrl_files[ck]), 'lines_read': 0, 'control_lines_read': 0}
                tabs = []
                for role, paths, key in (('sample', files[ck], 'lines_read'),) + ((('control', ctrl_files[ck], 'control_lines_read'),) if controls else ()):
                    t = engine.new_tables(role, ck, n)
                    try:
                        entry[key] = tables.fill(t, paths, pool, ck, n, notes)
                    except (merge.MergeError, tables.TableError) as exc:          # `file:line: reason`; the host tables' refusals
                        raise MotifsError('motifs: %s' % exc)
                    except (ValueError, RuntimeError) as exc:                     # the device tables' own (a coverage sum past int32)
                        raise MotifsError('motifs: %s: %s' % (exc.path, exc))
                    tabs.extend([t.plus, t.minus])
                counters, off_base = engine.count(seq, *tabs)
                for s, strand in enumerate('+-'):
                    entry[strand] = dict(zip(COUNT_KEYS, (int(v) for v in counters[s])), off_base=int(off_base[s]))
                    if off_base[s]:
                        notes.append('%s %s: %d lines lie on a letter that is not %s in --Ref: is %s the reference of these runs?' % (ck, strand, int(off_base[s]), base, mo['Ref']))
                doc['contigs'][ck] = entry
        hist = engine.fetch()
        times = engine.times()
    finally:
        if own:
            engine.close()
    found = find_motifs(hist, up, down, o['minSites'], o['minFrac'], o['maxMotifs'], base)
    if not found:
        notes.append('no pattern reached --minSites %d / --minFrac %d' % (o['minSites'], o['minFrac']))
    doc['contexts'] = {context_string(int(i), up, down, base): [int(hist[i, 0]), int(hist[i, 1])] for i in np.nonzero(hist.any(axis=1))[0]}
    doc['motifs'] = [dict(mt, percent=100 * mt['modified'] // max(mt['sites'], 1)) for mt in found]
    doc['notes'] = notes
    doc['times'] = {'upload_ms': round(times[0], 4), 'count_ms': round(times[1], 4)}
    out_folder = str(mo['outFolder'])
    os.makedirs(out_folder, exist_ok=True)
    prefix = os.path.join(out_folder, doc['inputs']['FileID'])
    text = report_text(found)
    with open(prefix + '_motifs.txt', 'w') as fh:
        fh.write(text)
    with open(prefix + '_motifs.json', 'w') as fh:
        json.dump(doc, fh, indent=1)
    for ln in notes:
        print(ln, flush=True)
    print(text, end='', flush=True)
    return doc
