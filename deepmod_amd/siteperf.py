"""Site-level detection performance from BED files: the second half of the headline metric.

The reference evaluates a run per genomic site: every BED line carries coverage and methylation percentage, a site has a truth
label (fully methylated / unmethylated control sample), and `roc_curve(label, pct)` is drawn over the sites with
`Coverage >= k` for k in (1, 5) (DeepMod_tools/cal_EcoliDetPerf.py:255-276: `cov_plot_thr = [1, 5]`, score =
`Methylation_Percentage`).  This module computes those numbers from the BED bytes this package writes; no plotting.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Tuple

import numpy as np

from . import _lib


def bed_sites(bed: bytes) -> Dict[str, np.ndarray]:
    """Columns of a mod_pos.*.bed file (myDetect.py:1112-1120): position (col 2), coverage (col 10), percentage (col 11),
    methylated reads (col 12)."""
    rows = [ln.split() for ln in bed.decode("ascii").splitlines() if ln.strip()]
    col = lambda i: np.array([int(r[i]) for r in rows], np.int64)
    if not rows:
        z = np.zeros(0, np.int64)
        return {"pos": z, "cov": z.copy(), "pct": z.copy(), "mod": z.copy()}
    return {"pos": col(1), "cov": col(9), "pct": col(10), "mod": col(11)}


def roc_auc(label: np.ndarray, score: np.ndarray) -> float:
    """Area under the ROC curve = auc(roc_curve(label, score)) (the Mann-Whitney statistic with midranks); nan if one class is empty."""
    label = np.asarray(label).astype(bool)
    score = np.asarray(score, np.float64)
    npos, nneg = int(label.sum()), int((~label).sum())
    if npos == 0 or nneg == 0:
        return float("nan")
    order = np.argsort(score, kind="mergesort")
    s = score[order]
    lo = np.searchsorted(s, s, "left")
    hi = np.searchsorted(s, s, "right")
    ranks = np.empty(len(s))
    ranks[order] = 0.5 * (lo + hi + 1)
    return float((ranks[label].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))


def site_level_auc(bed: bytes, methylated_positions: Iterable[int], cov_thresholds: Tuple[int, ...] = (1, 5)) -> Dict[int, float]:
    """{k: AUC of the per-site methylation percentage against the truth label over the sites with coverage >= k}.
    methylated_positions: the positions (same strand as the BED) whose truth label is 1; every other site of the BED is 0."""
    sites = bed_sites(bed)
    truth = np.isin(sites["pos"], np.fromiter(methylated_positions, np.int64))
    out = {}
    for k in cov_thresholds:
        sel = sites["cov"] >= k
        out[int(k)] = roc_auc(truth[sel], sites["pct"][sel])
    return out


# ---- `siteperf`: a run against control runs, per site (DeepMod_tools/cal_EcoliDetPerf.py) --------------------------------
# HostEngine below is the numpy statement of the semantics and the yardstick of the kernels (csrc/siteperf.hip.inc, DeviceEngine), as
# cluster.sites_from_counters is for the cluster stage.  Everything counted is an integer; AUC, AP and the curve points are float64 functions
# of the histogram alone (measures), in the arithmetic of sklearn's roc_curve / auc / average_precision_score - which this package never imports.

NCAT, NPCT, MAX_THRESHOLDS, MAX_MOTIF = 7, 101, 8, 16
RUN, CONTROL = 0, 1
NA4COM = {'A': 'T', 'C': 'G', 'T': 'A', 'G': 'C'}
INT32_MAX = 2 ** 31 - 1


class SitePerfError(ValueError):
    pass


def revcomp(pat: str) -> str:
    return ''.join(NA4COM[c] for c in reversed(pat))


def category_names(motif: str, k: int):
    """baseinfo of cal_EcoliDetPerf.py:222, in its order."""
    b = motif[k]
    return [motif, motif + '_n1' + b, motif + '_n2' + b, motif + '_n3' + b, 'Other' + b, motif + '_nb', 'Other']


def check_motif(motif: str, k: int) -> None:
    if not 1 <= len(motif) <= MAX_MOTIF:
        raise SitePerfError('siteperf: a motif has 1 to %d bases (got %r)' % (MAX_MOTIF, motif))
    if any(c not in NA4COM for c in motif.upper()):
        raise SitePerfError('siteperf: the motif %r holds a letter other than A, C, G, T' % motif)
    if not 0 <= k < len(motif):
        raise SitePerfError('siteperf: --ModinMotif %d is no position in the motif %s' % (k, motif))
    if motif[k] != motif[k].upper():
        raise SitePerfError('siteperf: the modified base of %s at offset %d is typed in lower case: the BED files are named mod_pos.*.%s.bed, '
                            'and the reference would look for *.%s.bed and find none' % (motif, k, motif[k].upper(), motif[k]))


def read_fasta(path: str, only: Optional[str] = None) -> Dict[str, bytes]:
    """{contig name (the header up to the first white space): its bytes, case kept} (readFA :39-57); `only`: that contig alone."""
    out, name, parts = {}, None, []
    with open(path, 'rb') as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            if line[:1] == b'>':
                if name is not None and (only is None or name == only):
                    out[name] = b''.join(parts)
                sp = line[1:].split()
                name, parts = (sp[0].decode('ascii', 'replace') if sp else ''), []
            elif name is not None and (only is None or name == only):
                parts.append(line)
    if name is not None and (only is None or name == only):
        out[name] = b''.join(parts)
    return out


def site_codes(seq, motif: str, k: int, start: Optional[int] = None, end: Optional[int] = None) -> np.ndarray:
    """uint8 [len]: bit 0 = '+' site, bit 1 = '-' site (readFA :60-72).  Position i is a '+' site if seq[i-k : i-k+m] == motif.upper(), a '-' site
    if seq[i-(m-1-k) : ...+m] == revcomp(motif.upper()), compared on the FASTA bytes as they are; only start <= i <= end can be a site."""
    s = np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else seq.astype(np.uint8, copy=False)
    n, m = len(s), len(motif)
    code = np.zeros(n, np.uint8)
    pat = motif.upper()
    for bit, p, off in ((1, pat, k), (2, revcomp(pat), m - 1 - k)):
        if n < m:
            continue
        hit = np.ones(n - m + 1, bool)                       # hit[j]: seq[j : j + m] == p
        for j, c in enumerate(p.encode('ascii')):
            hit &= s[j:j + n - m + 1] == c
        code[off:off + n - m + 1] |= np.where(hit, bit, 0).astype(np.uint8)
    lo = 0 if start is None or start < 0 else start
    hi = n - 1 if end is None or end < 0 else min(end, n - 1)
    code[:min(lo, n)] = 0
    code[max(hi + 1, 0):] = 0
    return code


def categories(code: np.ndarray, pos: np.ndarray, strand: np.ndarray, is_b: np.ndarray) -> np.ndarray:
    """Index into category_names of every (strand, position, line base == B) (:111-125): a site is 0; else the first of the offsets
    -3, -2, -1, 1, 2, 3 with a site of the same strand decides n|offset|; with B 1..3 / 4 (OtherB), with another base 5 (M_nb) / 6 (Other)."""
    pos = np.asarray(pos, np.int64)
    bit = (1 << np.asarray(strand, np.int64)).astype(np.uint8)
    n = len(code)
    near = np.zeros(len(pos), np.int64)
    for off in (-3, -2, -1, 1, 2, 3):
        q = pos + off
        ok = (q >= 0) & (q < n)
        hit = np.zeros(len(pos), bool)
        hit[ok] = (code[q[ok]] & bit[ok]) != 0
        near = np.where((near == 0) & hit, abs(off), near)
    cat = np.where(is_b, np.where(near > 0, near, 4), np.where(near > 0, 5, 6))
    return np.where((code[pos] & bit) != 0, 0, cat).astype(np.int64)


def _seq_array(seq) -> np.ndarray:
    return np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, np.uint8)


_COMP = np.zeros(256, np.uint8)
for _a, _b in NA4COM.items():
    _COMP[ord(_a)] = ord(_b)


def _check_thresholds(thresholds) -> Tuple[int, ...]:
    t = tuple(int(v) for v in thresholds)
    if not 1 <= len(t) <= MAX_THRESHOLDS:
        raise SitePerfError('siteperf: 1 to %d coverage thresholds (got %d)' % (MAX_THRESHOLDS, len(t)))
    if any(v < 0 for v in t) or any(b <= a for a, b in zip(t, t[1:])):
        raise SitePerfError('siteperf: the coverage thresholds are non-negative and strictly ascending (got %s)' % (t,))
    return t


def _records(pos, strand, base, cov, pct, mod):
    r = (np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(strand, np.uint8), np.ascontiguousarray(base, np.uint8),
         np.ascontiguousarray(cov, np.int32), np.ascontiguousarray(pct, np.int32), np.ascontiguousarray(mod, np.int32))
    if len({len(a) for a in r}) != 1:
        raise SitePerfError('siteperf: record arrays of different lengths')
    return r


class HostEngine:
    """The semantics in numpy: one contig at a time, the counters accumulate over contigs.
    hist int64 [7 categories][2 labels][thresholds][101 percentages]: an entry with coverage c counts in bucket (thresholds <= c) - 1, none below
    the smallest; counts = tp, fp, tn, fn over all entries (:126-131, :170-175)."""

    def __init__(self, thresholds=(1, 5)):
        self.thresholds = _check_thresholds(thresholds)
        self.hist = np.zeros((NCAT, 2, len(self.thresholds), NPCT), np.int64)
        self.counts = np.zeros(4, np.int64)
        self.lines_seen = self.lines_skipped = self.base_mismatch = 0
        self.code = None

    def close(self):
        pass

    def set_contig(self, seq, motif: str, k: int, start: Optional[int] = None, end: Optional[int] = None):
        check_motif(motif, k)
        self.seq = _seq_array(seq)
        if len(self.seq) < 1:
            raise SitePerfError('siteperf: an empty contig')
        self.B = ord(motif[k])
        self.code = site_codes(self.seq, motif, k, start, end)
        n = len(self.seq)
        self.lo = 0 if start is None or start < 0 else start
        self.hi = n - 1 if end is None or end < 0 else min(end, n - 1)
        self.ctl_cov = np.zeros((n, 2), np.int64)
        self.ctl_mod = np.zeros((n, 2), np.int64)
        self.ctl_base = np.zeros((n, 2), np.uint8)
        self.ctl_seen = np.zeros((n, 2), bool)
        self.ctl_bound = 0

    def codes(self) -> np.ndarray:
        return self.code.copy()

    def _count(self, cat, label, cov, pct, mod):
        bucket = np.searchsorted(np.asarray(self.thresholds, np.int64), cov, 'right')          # thresholds <= coverage
        sel = bucket > 0
        np.add.at(self.hist, (cat[sel], label[sel], bucket[sel] - 1, pct[sel]), 1)
        one = label == 1
        self.counts += np.array([mod[one].sum(), mod[~one].sum(), (cov - mod)[~one].sum(), (cov - mod)[one].sum()], np.int64)

    def add_records(self, role: int, pos, strand, base, cov, pct, mod):
        if self.code is None:
            raise SitePerfError('siteperf: no contig')
        pos, strand, base, cov, pct, mod = (a.astype(np.int64) for a in _records(pos, strand, base, cov, pct, mod))
        n = len(self.seq)
        bad = (pos < 0) | (pos >= n) | (strand > 1) | (cov < 0) | (mod < 0) | (mod > cov) | (pct < 0) | (pct > 100)
        if bad.any():
            raise SitePerfError('siteperf: record %d is outside the contig or the value ranges' % int(np.argmax(bad)))
        self.lines_seen += len(pos)
        inside = (pos >= self.lo) & (pos <= self.hi)
        self.lines_skipped += int((~inside).sum())
        pos, strand, base, cov, pct, mod = (a[inside] for a in (pos, strand, base, cov, pct, mod))
        refb = np.where(strand == 1, _COMP[self.seq[pos]], self.seq[pos])
        self.base_mismatch += int(((base != self.B) | (base != refb)).sum())                    # :96, :153
        if role == RUN:
            cat = categories(self.code, pos, strand, base == self.B)
            self._count(cat, (cat == 0).astype(np.int64), cov, pct, mod)
        elif role == CONTROL:
            if len(pos):
                self.ctl_bound += int(cov.max())
                if self.ctl_bound >= 2 ** 31:
                    raise SitePerfError('siteperf: the largest coverages of this contig\'s control files sum to %d (2^31 or more)' % self.ctl_bound)
            np.add.at(self.ctl_cov, (pos, strand), cov)
            np.add.at(self.ctl_mod, (pos, strand), mod)
            for i in np.nonzero(~self.ctl_seen[pos, strand])[0]:                                # the base is that of the first line seen (:100)
                if not self.ctl_seen[pos[i], strand[i]]:
                    self.ctl_seen[pos[i], strand[i]] = True
                    self.ctl_base[pos[i], strand[i]] = base[i]
        else:
            raise SitePerfError('siteperf: role %r' % (role,))

    def finish_contig(self):
        if self.code is None:
            raise SitePerfError('siteperf: no contig')
        pos, strand = np.nonzero(self.ctl_seen)
        cov, mod = self.ctl_cov[pos, strand], self.ctl_mod[pos, strand]
        pct = np.where(cov > 0, (100 * mod) // np.maximum(cov, 1), 0)                          # int(mod * 100 / cov) of the sums (:104)
        cat = categories(self.code, pos, strand, self.ctl_base[pos, strand] == self.B)
        self._count(cat, np.zeros(len(pos), np.int64), cov, pct, mod)
        self.code = None

    def fetch(self) -> Dict[str, object]:
        return {'hist': self.hist.copy(), 'counts': self.counts.copy(), 'lines_seen': int(self.lines_seen), 'lines_skipped': int(self.lines_skipped),
                'base_mismatch': int(self.base_mismatch)}


class DeviceEngine(_lib.Handle):
    """The same interface on one GPU (dm_siteperf_* of the C ABI); add_text is the device parser."""
    PREFIX, N_TIMES = 'dm_siteperf', 2

    def __init__(self, thresholds=(1, 5), device: int = 0):
        self.thresholds = _check_thresholds(thresholds)
        t = np.asarray(self.thresholds, np.int32)
        self._create(device, len(t), t.ctypes.data)
        self.length = -1

    def set_contig(self, seq, motif: str, k: int, start: Optional[int] = None, end: Optional[int] = None):
        check_motif(motif, k)
        s = _seq_array(seq)
        self.length = -1
        self._libmod.check(self._lib.dm_siteperf_set_contig(self._h, s.ctypes.data, len(s), motif.encode('ascii'), len(motif), k,
                                                            -1 if start is None else int(start), -1 if end is None else int(end)))
        self.length = len(s)

    def codes(self) -> np.ndarray:
        code = np.empty(max(self.length, 0), np.uint8)
        self._libmod.check(self._lib.dm_siteperf_fetch_codes(self._h, code.ctypes.data))
        return code

    def add_text(self, text: bytes, role: int, contig_name: str) -> Tuple[int, int, int]:
        """-> (lines, flag, first bad line (1-based, -1: none)); a flagged text is not counted."""
        ct = self._ct
        rows, flag, bad = ct.c_int64(0), ct.c_int32(0), ct.c_int64(-1)
        self._libmod.check(self._lib.dm_siteperf_add_text(self._h, ct.c_char_p(text), len(text), role, contig_name.encode('ascii'), ct.byref(rows), ct.byref(flag),
                                                          ct.byref(bad)))
        self._n = 0 if flag.value else rows.value
        return rows.value, flag.value, bad.value

    def add_records(self, role: int, pos, strand, base, cov, pct, mod):
        pos, strand, base, cov, pct, mod = _records(pos, strand, base, cov, pct, mod)
        self._libmod.check(self._lib.dm_siteperf_add_records(self._h, role, len(pos), pos.ctypes.data, strand.ctypes.data, base.ctypes.data, cov.ctypes.data,
                                                             pct.ctypes.data, mod.ctypes.data))
        self._n = len(pos)

    def records(self):
        """(pos, strand, base, cov, pct, mod) of the last add_text / add_records as they lie on the device."""
        n = self._n
        pos, cov, pct, mod = (np.zeros(n, np.int32) for _ in range(4))
        strand, base = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self._libmod.check(self._lib.dm_siteperf_fetch_records(self._h, pos.ctypes.data, strand.ctypes.data, base.ctypes.data, cov.ctypes.data, pct.ctypes.data,
                                                               mod.ctypes.data))
        return pos, strand, base, cov, pct, mod

    def finish_contig(self):
        self.length = -1
        self._libmod.check(self._lib.dm_siteperf_finish_contig(self._h))

    def fetch(self) -> Dict[str, object]:
        ct = self._ct
        hist = np.zeros((NCAT, 2, len(self.thresholds), NPCT), np.int64)
        counts = np.zeros(4, np.int64)
        seen, skipped, mism = ct.c_int64(0), ct.c_int64(0), ct.c_int64(0)
        self._libmod.check(self._lib.dm_siteperf_fetch(self._h, hist.ctypes.data, counts.ctypes.data, ct.byref(seen), ct.byref(skipped), ct.byref(mism)))
        return {'hist': hist, 'counts': counts, 'lines_seen': seen.value, 'lines_skipped': skipped.value, 'base_mismatch': mism.value}


def tile_bytes() -> int:
    return _lib.load().dm_siteperf_tile_bytes()


def parse_device_grammar(text: bytes, contig_name: str, contig_len: int):
    """The device's line routine compiled for the host (no GPU needed) -> ((pos, strand, base, cov, pct, mod), flag, first bad line)."""
    import ctypes
    lib = _lib.load()
    flag, bad = ctypes.c_int32(0), ctypes.c_int64(-1)
    buf, name = ctypes.c_char_p(text), contig_name.encode('ascii')
    rows = lib.dm_siteperf_parse_host(buf, len(text), name, contig_len, None, None, None, None, None, None, 0, ctypes.byref(flag), ctypes.byref(bad))
    if rows < 0:
        _lib.check(int(rows))
    pos, cov, pct, mod = (np.zeros(rows, np.int32) for _ in range(4))
    strand, base = np.zeros(rows, np.uint8), np.zeros(rows, np.uint8)
    if rows:
        lib.dm_siteperf_parse_host(buf, len(text), name, contig_len, pos.ctypes.data, strand.ctypes.data, base.ctypes.data, cov.ctypes.data, pct.ctypes.data,
                                   mod.ctypes.data, rows, ctypes.byref(flag), ctypes.byref(bad))
    return (pos, strand, base, cov, pct, mod), flag.value, bad.value


def parse_bed_host(text: bytes, fn: str = '<text>') -> Dict[str, Tuple[np.ndarray, ...]]:
    """The host parser, the reference's own reading of a line (:81-90): white-space split, at least 12 fields, int() of fields 1, 9, 10, 11; empty
    lines are passed over.  -> {contig: (pos, strand, base, cov, pct, mod)} in the order of the lines.  What no engine can hold is refused with
    file and line."""
    rows: Dict[str, list] = {}
    for no, line in enumerate(text.split(b'\n'), 1):
        lsp = line.split()
        if not lsp:
            continue
        if len(lsp) < 12:
            raise SitePerfError('%s:%d: %d fields, a mod_pos BED line has at least 12' % (fn, no, len(lsp)))
        try:
            pos, cov, pct, mod = int(lsp[1]), int(lsp[9]), int(lsp[10]), int(lsp[11])
        except ValueError as exc:
            raise SitePerfError('%s:%d: %s' % (fn, no, exc))
        if lsp[5] not in (b'+', b'-'):
            raise SitePerfError('%s:%d: strand %r' % (fn, no, lsp[5].decode('ascii', 'replace')))
        if not (0 <= pos <= INT32_MAX and 0 <= mod <= cov <= INT32_MAX and 0 <= pct <= 100):
            raise SitePerfError('%s:%d: position %d, coverage %d, percentage %d, modified %d: outside 0 <= modified <= coverage < 2^31, percentage <= 100'
                                % (fn, no, pos, cov, pct, mod))
        base = lsp[3][0] if len(lsp[3]) == 1 else 0                   # a longer field equals no base
        rows.setdefault(lsp[0].decode('ascii', 'replace'), []).append((pos, 1 if lsp[5] == b'-' else 0, base, cov, pct, mod, no))
    out = {}
    for name, r in rows.items():
        a = np.array(r, np.int64).reshape(-1, 7)
        out[name] = (a[:, 0].astype(np.int32), a[:, 1].astype(np.uint8), a[:, 2].astype(np.uint8), a[:, 3].astype(np.int32), a[:, 4].astype(np.int32),
                     a[:, 5].astype(np.int32), a[:, 6])
    return out


def curve_points(pos: np.ndarray, neg: np.ndarray):
    """Entries per percentage of either label -> (percentages descending, tps, fps): _binary_clf_curve of sklearn on the histogram."""
    pos, neg = np.asarray(pos, np.int64), np.asarray(neg, np.int64)
    pcts = np.nonzero((pos + neg) > 0)[0][::-1]
    return pcts, np.cumsum(pos[pcts]).astype(np.float64), np.cumsum(neg[pcts]).astype(np.float64)


def roc_from_hist(pos, neg):
    """-> (auc, fpr, tpr, percentages): auc(roc_curve(label, pct)) in sklearn's arithmetic (collinear points dropped, trapezoid rule); nan when a
    class is empty."""
    pcts, tps, fps = curve_points(pos, neg)
    if len(pcts) == 0 or tps[-1] <= 0 or fps[-1] <= 0:
        return float('nan'), [], [], []
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, pcts = fps[keep], tps[keep], pcts[keep]
    tps, fps = np.r_[0, tps], np.r_[0, fps]
    fpr, tpr = fps / fps[-1], tps / tps[-1]
    area = float((np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0).sum())
    return area, fpr.tolist(), tpr.tolist(), [None] + [int(p) for p in pcts]


def pr_from_hist(pos, neg):
    """-> (ap, precision, recall, percentages): average_precision_score(label, pct) in sklearn's arithmetic; without a positive the recall is 1
    at every threshold (ap 0.0), without any entry nan."""
    pcts, tps, fps = curve_points(pos, neg)
    if len(pcts) == 0:
        return float('nan'), [], [], []
    precision = tps / (tps + fps)
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    precision, recall = np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0))
    ap = float(max(0.0, -np.sum(np.diff(recall) * precision[:-1])))
    return ap, precision.tolist(), recall.tolist(), [int(p) for p in pcts[::-1]]


SETS = (('all_mp', tuple(range(NCAT))), ('motif_mp', (0,)))


def measures(hist: np.ndarray, thresholds) -> Dict[str, Dict[int, Dict[str, object]]]:
    """{set: {threshold: positives, negatives, auc, ap and the curve points}} over the entries with coverage >= threshold."""
    out = {}
    for name, cats in SETS:
        out[name] = {}
        for j, t in enumerate(thresholds):
            h = hist[list(cats)][:, :, j:].sum(axis=(0, 2))           # [label][pct]
            area, fpr, tpr, roc_pct = roc_from_hist(h[1], h[0])
            ap, precision, recall, pr_pct = pr_from_hist(h[1], h[0])
            out[name][int(t)] = {'positives': int(h[1].sum()), 'negatives': int(h[0].sum()), 'auc': area, 'ap': ap,
                                 'roc': {'fpr': fpr, 'tpr': tpr, 'pct': roc_pct}, 'pr': {'precision': precision, 'recall': recall, 'pct': pr_pct}}
    return out


def report_lines(figure_folder: str, motif: str, k: int, thresholds, meas) -> list:
    """The lines cal_EcoliDetPerf.py prints from :247 on, in its order and formats.  The PNG names are labels: nothing is drawn."""
    names = category_names(motif, k)
    lines = []
    for (name, cats) in SETS:
        lines.append('basetype={} classify_measure={}'.format([names[c] for c in cats], 'Methylation_Percentage'))
        for t in thresholds:
            area = meas[name][int(t)]['auc']
            if not np.isnan(area):
                lines.append('\t\t %s %d %.7f' % (figure_folder + '/roc_plot_met_roc_' + name + '.png', t, area))
        for t in thresholds:
            lines.append('\t\t %s %d ap=%.5f' % (figure_folder + '/ap_plot_met_pr_' + name + '.png', t, meas[name][int(t)]['ap']))
    return lines


def find_bed_files(folder: str, base: str, control: bool = False) -> list:
    """mod_pos.*.<B>.bed in the folder, one and two levels down (:194-207; the order of the levels as the reference lists them, names sorted)."""
    import glob
    import os
    levels = ['', '*', os.path.join('*', '*')]
    out = []
    for lv in (reversed(levels) if control else levels):
        out.extend(sorted(glob.glob(os.path.join(folder, lv, 'mod_pos.*.' + base + '.bed'))))
    return out


def _first_contig(text: bytes) -> Optional[str]:
    for line in text.split(b'\n', 64):
        sp = line.split()
        if sp:
            return sp[0].decode('ascii', 'replace')
    return None


def _single_contig(text: bytes, name: str) -> bool:
    """Every line of the text starts with the name and one separator (counted at C speed): the text may go to the device whole."""
    nb = name.encode('ascii', 'replace')
    lines = text.count(b'\n') + (0 if text.endswith(b'\n') else 1)
    starts = sum(text.count(b'\n' + nb + sep) for sep in (b'\t', b' ')) + (1 if text.startswith(nb + b'\t') or text.startswith(nb + b' ') else 0)
    return starts == lines


def check_options(mo: Dict[str, object]):
    """What can be refused before any file is read or any GPU asked for -> (motif, k, thresholds, chr, start, end, [(role, path)])."""
    import os
    motif, k = str(mo['motif']), int(mo['ModinMotif'])
    check_motif(motif, k)
    thresholds = _check_thresholds(mo.get('cov') or (1, 5))
    chrom, start, end = mo.get('chr') or None, mo.get('start'), mo.get('end')
    start = None if start is None or start < 0 else int(start)
    end = None if end is None or end < 0 else int(end)
    if chrom is None and (start is not None or end is not None):
        raise SitePerfError('siteperf: --start / --end need --chr (a region lies on one contig)')
    if not mo.get('Ref') or not os.path.isfile(mo['Ref']):
        raise SitePerfError('siteperf: --Ref: reference file does not exist (%s)' % mo.get('Ref'))
    base = motif[k]
    files = []                                                        # (role, path)
    for role, folders in ((CONTROL, list(mo['control'])), (RUN, [mo['predFolder']])):
        for folder in folders:
            if not folder or not os.path.isdir(folder):
                raise SitePerfError('siteperf: no prediction folder %s' % folder)
            found = find_bed_files(folder, base, control=role == CONTROL)
            if not found:
                raise SitePerfError('siteperf: no mod_pos.*.%s.bed in %s (nor one or two levels below)' % (base, folder))
            files.extend((role, p) for p in found)
    return motif, k, thresholds, chrom, start, end, files


def siteperf(mo: Dict[str, object], engine=None) -> Dict[str, object]:
    """The command.  mo: predFolder, control (list of folders), Ref, motif, ModinMotif, chr (None: every contig of the FASTA), start, end (None:
    none), cov (thresholds), outFolder, FileID, threads, figure_folder (the folder the printed PNG labels name; default outFolder).
    engine: an object with HostEngine's interface (default: DeviceEngine on GPU 0).  -> the JSON document; writes <FileID>_siteperf.txt / .json."""
    import json
    import os
    from concurrent.futures import ThreadPoolExecutor
    motif, k, thresholds, chrom, start, end, files = check_options(mo)
    fasta = read_fasta(mo['Ref'], chrom)
    if not fasta:
        raise SitePerfError('siteperf: %s holds no contig%s' % (mo['Ref'], '' if chrom is None else ' named ' + chrom))

    def read(path):
        with open(path, 'rb') as fh:
            return fh.read()

    own = engine is None
    if own:
        engine = DeviceEngine(thresholds)
    notes, other_contig_lines = [], 0
    work: Dict[str, list] = {}                                        # contig -> [(order, role, path or None, records or None)]
    try:
        with ThreadPoolExecutor(max(int(mo.get('threads') or 1), 1)) as pool:
            # bucket the files by the contig of their first line; a file of several contigs is split here
            for order, ((role, path), text) in enumerate(zip(files, pool.map(read, [p for _, p in files]))):
                name = _first_contig(text)
                if name is None:
                    continue
                if _single_contig(text, name):
                    if name in fasta:
                        work.setdefault(name, []).append((order, role, path, None))
                    else:
                        other_contig_lines += text.count(b'\n') + (0 if text.endswith(b'\n') else 1)
                    continue
                for cname, rec in parse_bed_host(text, path).items():
                    if cname in fasta:
                        work.setdefault(cname, []).append((order, role, path, rec))
                    else:
                        other_contig_lines += len(rec[0])
            for name in sorted(work):
                seq = fasta[name]
                engine.set_contig(seq, motif, k, start, end)
                items = work[name]
                texts = pool.map(lambda it: read(it[2]) if it[3] is None else None, items)       # the threads read ahead
                for (order, role, path, rec), text in zip(items, texts):
                    if rec is None:
                        flag, bad = 1, -1
                        if hasattr(engine, 'add_text'):
                            _, flag, bad = engine.add_text(text, role, name)
                            if flag:
                                notes.append('%s: line %d is outside the device grammar: the file is parsed on the host' % (path, bad))
                        if not flag:
                            continue
                        rec = parse_bed_host(text, path).get(name)
                        if rec is None:
                            continue
                    over = np.nonzero(rec[0] >= len(seq))[0]
                    if len(over):
                        raise SitePerfError('%s:%d: position %d is not on %s (%d bases)' % (path, int(rec[6][over[0]]), int(rec[0][over[0]]), name, len(seq)))
                    engine.add_records(role, *rec[:6])
                engine.finish_contig()
        got = engine.fetch()
    finally:
        if own:
            engine.close()
    hist = got['hist']
    meas = measures(hist, thresholds)
    out_folder = str(mo['outFolder'])
    figure_folder = str(mo.get('figure_folder') or out_folder)
    lines = report_lines(figure_folder, motif, k, thresholds, meas)
    names = category_names(motif, k)

    def clean(v):
        return None if isinstance(v, float) and np.isnan(v) else v

    doc = {
        'inputs': {'predFolder': mo['predFolder'], 'control': list(mo['control']), 'Ref': mo['Ref'], 'motif': motif, 'ModinMotif': k, 'chr': chrom, 'start': start,
                   'end': end, 'cov': list(thresholds), 'files': [p for _, p in files]},
        'categories': {names[c]: {'label0': int(hist[c, 0].sum()), 'label1': int(hist[c, 1].sum())} for c in range(NCAT)},
        'measures': {s: {str(t): {key: (clean(v) if not isinstance(v, dict) else v) for key, v in m.items()} for t, m in by_t.items()} for s, by_t in meas.items()},
        'read_level': dict(zip(('tp', 'fp', 'tn', 'fn'), (int(v) for v in got['counts']))),
        'lines_seen': got['lines_seen'], 'lines_outside_region': got['lines_skipped'], 'lines_other_contig': int(other_contig_lines),
        'base_mismatch_lines': got['base_mismatch'], 'notes': notes,
        'histogram': {'axes': ['category', 'label', 'coverage bucket (thresholds <= coverage, minus one)', 'percentage'], 'category_names': names,
                      'counts': hist.tolist()},
    }
    os.makedirs(out_folder, exist_ok=True)
    prefix = os.path.join(out_folder, str(mo.get('FileID') or 'mod'))
    with open(prefix + '_siteperf.txt', 'w') as fh:
        fh.write(''.join(ln + '\n' for ln in lines))
    with open(prefix + '_siteperf.json', 'w') as fh:
        json.dump(doc, fh, indent=1)
    for ln in notes + lines:
        print(ln)
    doc['lines'] = lines
    return doc


def shim_options(argv) -> Dict[str, object]:
    """The nine positional arguments of DeepMod_tools/cal_EcoliDetPerf.py (:179-201) -> the options of siteperf()."""
    if len(argv) != 9:
        raise SitePerfError('usage: cal_EcoliDetPerf.py run-folder genome.fa motif offset contig-or-\'\' start-or--1 end-or--1 figure-folder control[,control..]')
    run, ref, motif, k, chrom, start, end, fig, controls = argv
    return {'predFolder': run, 'Ref': ref, 'motif': motif, 'ModinMotif': int(k), 'chr': chrom if chrom != '' else None,
            'start': None if int(start) < 0 else int(start), 'end': None if int(end) < 0 else int(end), 'outFolder': fig, 'figure_folder': fig,
            'FileID': 'cal_EcoliDetPerf', 'control': controls.split(','), 'cov': (1, 5), 'threads': 1}
