"""CpG-cluster second stage: counterpart of
/root/reference/DeepMod_tools/hm_cluster_predict.py.

For every CpG-motif C with coverage in a DeepMod BED: 14 features
  [own methylation fraction, partner-strand fraction (0 if absent), #neighbours,
   11-bin histogram of the neighbours' fractions (0.1 bins) normalised by #neighbours]
over the CpG sites within +-25 bp that are present in the BED (hm_cluster_predict.py:128-154), then the
MLP 14->100->20->1 on the GPU (dm_cluster_predict) and the original BED line with int(p*100) appended (:170).
Feature extraction is vectorised numpy on the host (searchsorted and per-bin prefix counts instead of dict probes).
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import numpy as np

from . import _lib, tfbundle

NBSIZE = 25          # hm_cluster_predict.py:83
BATCH_SIZE = 4096    # hm_cluster_predict.py:16
WEIGHT_ORDER = ("W_1", "b_1", "W_2", "b_2", "W_O", "b_O")
CHRKEYS = ["chr%d" % i for i in range(1, 23)] + ["chrX", "chrY", "chrM"]   # :86-91


def flatten_cluster_weights(tensors: Dict[str, np.ndarray]) -> np.ndarray:
    shapes = {"W_1": (14, 100), "b_1": (100,), "W_2": (100, 20), "b_2": (20,), "W_O": (20, 1), "b_O": (1,)}
    parts = []
    for name in WEIGHT_ORDER:
        a = np.asarray(tensors[name], np.float32)
        if a.shape != shapes[name]:
            raise ValueError("cluster tensor %s has shape %s, expected %s" % (name, a.shape, shapes[name]))
        parts.append(a.ravel())
    return np.ascontiguousarray(np.concatenate(parts))


class ClusterModel:
    def __init__(self, tensors: Dict[str, np.ndarray], device: int = 0):
        self._lib = _lib.load()
        flat = flatten_cluster_weights(tensors)
        self._h = self._lib.dm_cluster_create(device, flat.ctypes.data, flat.size)
        if not self._h:
            raise _lib.DeepModHipError("dm_cluster_create: " + _lib.last_error())

    @classmethod
    def from_checkpoint(cls, prefix: str, device: int = 0) -> "ClusterModel":
        return cls(tfbundle.load_bundle(prefix, names=WEIGHT_ORDER), device)

    def predict(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)     # the placeholder casts the float64 feed to fp32
        if x.ndim != 2 or x.shape[1] != 14:
            raise ValueError("expected [n,14] features, got %s" % (x.shape,))
        out = np.empty(x.shape[0], np.float32)
        _lib.check(self._lib.dm_cluster_predict(self._h, x.ctypes.data, x.shape[0], out.ctypes.data))
        return out

    def sites(self, plus, minus, seq, first: int = 0, count=None, from_slice: bool = False, halo=None, seq_first: int = 0,
              want_features: bool = False) -> Dict[str, np.ndarray]:
        """The cluster stage of one contig from its two PositionSummary objects, on the device (dm_cluster_sites; the numpy twin is
        sites_from_counters): either summary may be None (all zero).  from_slice: the summaries hold [first, first + count) after
        reduce_scatter, `halo` (halo_from_edges) the counters 26 positions to either side (whole tables without one: read from the tables), `seq` the
        bases from seq_first on.
        -> {'n_plus', 'pos', 'cov', 'mod', 'new'[, 'features']}: '+' sites ascending, then '-' sites ascending."""
        import ctypes
        seq = _seq_bytes(seq)
        if count is None:
            count = max([s.length for s in (plus, minus) if s is not None] + [0]) - int(first)
        if halo is not None:
            halo = np.ascontiguousarray(halo, np.int32)
            if halo.shape != (2, 2, 2, HALO):
                raise ValueError("halo: expected [2 sides][2 strands][cov|mod][%d], got %s" % (HALO, halo.shape,))
        n_plus = ctypes.c_int64()
        n = self._lib.dm_cluster_sites(self._h, plus._h if plus is not None else None, minus._h if minus is not None else None, int(bool(from_slice)),
                                       seq.ctypes.data if seq.size else None, int(seq_first), seq.size, int(first), max(int(count), 0),
                                       halo.ctypes.data if halo is not None else None, ctypes.byref(n_plus))
        if n < 0:
            _lib.check(int(n))
        out = {"n_plus": int(n_plus.value), "pos": np.empty(n, np.int64), "cov": np.empty(n, np.int32), "mod": np.empty(n, np.int32),
               "new": np.empty(n, np.int32)}
        feats = np.empty((n, 14), np.float32) if want_features else None
        _lib.check(self._lib.dm_cluster_sites_fetch(self._h, out["pos"].ctypes.data, out["cov"].ctypes.data, out["mod"].ctypes.data,
                                                    out["new"].ctypes.data, feats.ctypes.data if want_features else None))
        if want_features:
            out["features"] = feats
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dm_cluster_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------
# the stage from the counters (detect --clusterCpG): numpy twin of csrc/cluster_sites.hip.inc
# ---------------------------------------------------------------------------------------------
HALO = NBSIZE + 1    # counters a slice needs from either side: the 25 neighbour positions + the partner C of the outermost


def _seq_bytes(seq) -> np.ndarray:
    if isinstance(seq, str):
        seq = seq.encode("ascii")
    if isinstance(seq, (bytes, bytearray, memoryview)):
        return np.frombuffer(seq, dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


def slice_edges(cov_p, mod_p, cov_m, mod_m) -> list:
    """What a rank publishes of its slice: the first and the last 26 values of cov and mod of both strands, [strand][cov|mod][head|tail]
    as plain lists (a few hundred integers; a strand the rank holds nothing of: None arrays)."""
    out = []
    for cv, md in ((cov_p, mod_p), (cov_m, mod_m)):
        out.append([[np.asarray(a)[:HALO].tolist(), np.asarray(a)[-HALO:].tolist()] if a is not None and len(a) else [[], []] for a in (cv, md)])
    return out


def halo_from_edges(first: int, count: int, everyone) -> np.ndarray:
    """int32 [2 sides][2 strands][cov|mod][26] for the slice [first, first + count): the counters of positions first - 26 .. first - 1 and
    first + count .. first + count + 25, taken from the edges the ranks published: everyone = [{'first', 'count', 'edges': slice_edges(...)}].
    Slices are contiguous, so a position within 26 of this slice lies within 26 of its owner's nearer end (also when slices are
    shorter than 26 positions and the halo spans several ranks); positions nobody owns are zero."""
    halo = np.zeros((2, 2, 2, HALO), np.int32)
    for side, q0 in ((0, first - HALO), (1, first + count)):
        for e in everyone:
            f, c = int(e["first"]), int(e["count"])
            for k in range(HALO):
                q = q0 + k
                if not (f <= q < f + c) or first <= q < first + count:
                    continue
                for s in range(2):
                    for kind in range(2):
                        head, tail = e["edges"][s][kind]
                        if q - f < len(head):
                            halo[side, s, kind, k] = head[q - f]
                        elif f + c - q <= len(tail):
                            halo[side, s, kind, k] = tail[len(tail) - (f + c - q)]
    return halo


def sites_from_counters(seq, cov_p, mod_p, cov_m, mod_m, first: int = 0, halo=None, seq_first: int = 0) -> Dict[str, np.ndarray]:
    """The CpG-cluster stage of `detect --clusterCpG` from the counters of positions [first, first + len): what the three tools compute
    through their files (sum_chr_mod.py -> generate_motif_pos.py -> hm_cluster_predict.py), and what csrc/cluster_sites.hip.inc computes.
      site      position q with mod > 0 on a CpG C: '+' where the upper-cased sequence reads C at q and G at q + 1, '-' where it reads G at
                q and C at q - 1 (generate_motif_pos.py:62-63); pct = (100 * mod) // cov, frac = pct / 100.0
      partner   the other strand's C of the same CpG (q + 1 for '+', q - 1 for '-'): feature 1 is its frac if it is a site, else 0
      neighbours  the sites of either strand within [q - 25, q + 25] but the site itself and its partner: feature 2 is their number n,
                features 3..13 rint(1000 * (cnt[b] / n)) / 1000 with b = int(frac / 0.1 + 0.5), all 0 when n == 0
    cov_* / mod_* None: all zero.  halo (halo_from_edges): the counters 26 positions to either side; their sites count as neighbours and
    partners and are not output.  `seq` holds the bases from position seq_first on; positions outside it hold no base.
    -> {'n_plus', 'pos', 'cov', 'mod', 'features' float64 [n, 14]}: '+' sites ascending, then '-' sites ascending."""
    s = _seq_bytes(seq)
    s = np.where((s >= 97) & (s <= 122), s - 32, s).astype(np.uint8)
    count = max([len(a) for a in (cov_p, mod_p, cov_m, mod_m) if a is not None] + [0])
    ext = count + 2 * HALO                                       # index e <-> position first - HALO + e
    q = first - HALO + np.arange(ext, dtype=np.int64)

    def base(at):
        j = at - seq_first
        ok = (j >= 0) & (j < len(s)) & (at >= 0)
        return np.where(ok, s[np.clip(j, 0, max(len(s) - 1, 0))] if len(s) else 0, 0)

    b0, bn, bp = base(q), base(q + 1), base(q - 1)
    is_site = [(b0 == ord("C")) & (bn == ord("G")), (b0 == ord("G")) & (bp == ord("C"))]
    halo = np.zeros((2, 2, 2, HALO), np.int64) if halo is None else np.asarray(halo, np.int64)
    code = np.zeros(ext, np.int64)                               # 0: no site, else pct + 1; strand[e] tells which
    strand = np.zeros(ext, np.int64)
    covs, mods = np.zeros(ext, np.int64), np.zeros(ext, np.int64)
    for st, (cv, md) in enumerate(((cov_p, mod_p), (cov_m, mod_m))):
        c = np.zeros(ext, np.int64)
        m = np.zeros(ext, np.int64)
        if cv is not None:
            c[HALO:HALO + len(cv)] = cv
            m[HALO:HALO + len(md)] = md
        c[:HALO], m[:HALO] = halo[0, st, 0], halo[0, st, 1]
        c[HALO + count:], m[HALO + count:] = halo[1, st, 0], halo[1, st, 1]
        hit = is_site[st] & (m > 0) & (c > 0)
        pct = np.minimum((100 * m[hit]) // c[hit], 100)          # (mod <= cov by construction)
        code[hit] = pct + 1
        strand[hit] = st
        covs[hit], mods[hit] = c[hit], m[hit]
    frac_of = np.arange(101) / 100.0
    bin_of = (frac_of / 0.1 + 0.5).astype(np.int64)
    core = np.zeros(ext, bool)
    core[HALO:HALO + count] = True
    out = {"pos": [], "cov": [], "mod": [], "features": []}
    for st in range(2):
        e = np.flatnonzero(core & (code > 0) & (strand == st))
        partner = e + (1 if st == 0 else -1)
        x = np.zeros((len(e), 14))
        x[:, 0] = frac_of[code[e] - 1]
        x[:, 1] = np.where(code[partner] > 0, frac_of[np.maximum(code[partner] - 1, 0)], 0.0)
        cnt = np.zeros((len(e), 11), np.int64)
        for d in range(-NBSIZE, NBSIZE + 1):
            v = code[e + d]
            use = (v > 0) & (d != 0) & (e + d != partner)
            np.add.at(cnt, (np.flatnonzero(use), bin_of[v[use] - 1]), 1)
        n = cnt.sum(axis=1)
        x[:, 2] = n
        has = n > 0
        x[has, 3:] = np.rint(cnt[has] / n[has, None].astype(np.float64) * 1000.0) / 1000.0
        out["pos"].append(q[e])
        out["cov"].append(covs[e])
        out["mod"].append(mods[e])
        out["features"].append(x)
    n_plus = len(out["pos"][0])
    res = {k: np.concatenate(v) for k, v in out.items()}
    res["n_plus"] = n_plus
    return res


def site_lines_py(chrom: str, base: str, res, new=None) -> List[str]:
    """The rows sum_chr_mod.py:63 writes for the sites of sites_from_counters / ClusterModel.sites (with `new`: + ' <new>')."""
    lines = []
    for i, (p, cv, md) in enumerate(zip(res["pos"].tolist(), res["cov"].tolist(), res["mod"].tolist())):
        ln = '%s %d %d %s %d %s  %d %d 0,0,0 %d %d %d' % (chrom, p, p + 1, base, cv if cv < 1000 else 1000, '+' if i < res["n_plus"] else '-', p, p + 1, cv,
                                                          int(md * 100 / cv) if cv > 0 else 0, md)
        lines.append(ln if new is None else '%s %d' % (ln, int(new[i])))
    return lines


def site_text_parts(chrom: str, base: str, res) -> List[bytes]:
    """The file's bytes for the records of ClusterModel.sites: dm_cluster_bed_format per strand -> ['+' rows, '-' rows]."""
    lib = _lib.load()
    n, n_plus = len(res["pos"]), int(res["n_plus"])
    parts = []
    for strand, lo, hi in (("+", 0, n_plus), ("-", n_plus, n)):
        cols = [np.ascontiguousarray(res[k][lo:hi], dt) for k, dt in (("pos", np.int64), ("cov", np.int32), ("mod", np.int32), ("new", np.int32))]
        args = (chrom.encode("ascii"), strand.encode("ascii"), base.encode("ascii")) + tuple(c.ctypes.data for c in cols) + (hi - lo,)
        bound = lib.dm_cluster_bed_format(*args, None, 0)
        if bound < 0:
            raise _lib.DeepModHipError("dm_cluster_bed_format: " + _lib.last_error())
        buf = np.empty(max(int(bound), 1), np.uint8)
        got = lib.dm_cluster_bed_format(*args, buf.ctypes.data, int(bound))
        if got < 0 or got > bound:
            raise _lib.DeepModHipError("dm_cluster_bed_format: " + _lib.last_error())
        parts.append(buf[:got].tobytes())
    return parts


def read_motif(path: str) -> Dict[str, np.ndarray]:
    """motif_<chr>_C.bed rows `chr pos strand ...` -> sorted position arrays per strand (:117-123)."""
    pos = {"+": [], "-": []}
    with open(path) as fh:
        for line in fh:
            lsp = line.split()
            if len(lsp) >= 3:
                pos[lsp[2]].append(int(lsp[1]))
    return {s: np.unique(np.array(v, dtype=np.int64)) for s, v in pos.items()}


def read_pred(path: str, chrom: str, motif: Dict[str, np.ndarray]):
    """readpredmod (:43-72): keep rows of `chrom` that are CpG-motif sites with coverage > 0.
    Returns per strand: sorted positions, fraction round(pct/100, 3), and the stripped lines."""
    rows = {"+": {}, "-": {}}
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            lsp = line.split()
            c, p, s = lsp[0], int(lsp[1]), lsp[5]
            if s not in motif or c != chrom:
                continue
            i = np.searchsorted(motif[s], p)
            if i >= len(motif[s]) or motif[s][i] != p:
                continue
            cov, pct, mc = int(lsp[9]), int(lsp[10]), int(lsp[11])
            if cov == 0:
                continue
            if p not in rows[s]:
                rows[s][p] = [cov, round(pct / 100.0, 3), mc, line]
            else:                                           # duplicate row: counts add (:67-72)
                r = rows[s][p]
                r[0] += cov
                r[2] += mc
                if r[0] > 0:
                    r[1] = round(r[2] / float(r[0]), 3)
    out = {}
    for s in "+-":
        keys = sorted(rows[s])
        out[s] = (np.array(keys, dtype=np.int64), np.array([rows[s][k][1] for k in keys], dtype=np.float64),
                  [rows[s][k][3] for k in keys])
    return out


def cluster_features(pred) -> Tuple[np.ndarray, List[str]]:
    """14 features per site in the reference's key order (all '+' sites ascending, then all '-')."""
    pos_all = np.concatenate([pred["+"][0], pred["-"][0]])
    frac_all = np.concatenate([pred["+"][1], pred["-"][1]])
    order = np.argsort(pos_all, kind="stable")
    spos, sfrac = pos_all[order], frac_all[order]           # a position is a CpG C on at most one strand
    bins = (sfrac / 0.1 + 0.5).astype(np.int64)             # int(frac/0.1+0.5)  (:144)
    cum = np.zeros((11, len(spos) + 1), np.int64)
    for b in range(11):
        cum[b, 1:] = np.cumsum(bins == b)
    feats, lines = [], []
    for s in "+-":
        pos, frac, ln = pred[s]
        n = len(pos)
        x = np.zeros((n, 14))
        x[:, 0] = frac
        o = "-" if s == "+" else "+"
        ppos = pos + (1 if s == "+" else -1)
        opos, ofrac, _ = pred[o]
        if len(opos):
            j = np.clip(np.searchsorted(opos, ppos), 0, len(opos) - 1)
            hit = opos[j] == ppos
            x[hit, 1] = ofrac[j[hit]]
        # neighbourhood histogram without a per-site loop: per-bin prefix counts over the position-sorted sites give the
        # counts of any [pos - 25, pos + 25] range as a difference; the site itself and its partner C are taken out again
        lo = np.searchsorted(spos, pos - NBSIZE, side="left")
        hi = np.searchsorted(spos, pos + NBSIZE, side="right")
        cnt = cum[:, hi] - cum[:, lo]                                         # [11, n]
        for v in (pos, ppos):
            l, r = np.searchsorted(spos, v, side="left"), np.searchsorted(spos, v, side="right")
            cnt -= cum[:, r] - cum[:, l]
        nkeep = cnt.sum(axis=0)
        has = nkeep > 0
        x[:, 2] = nkeep
        x[has, 3:] = np.round(cnt[:, has].T / nkeep[has, None].astype(np.float64), 3)
        feats.append(x)
        lines.extend(ln)
    return np.concatenate(feats) if feats else np.zeros((0, 14)), lines


def hm_cluster_predict(pred_prefix: str, motif_folder: str, model_prefix: str, chrkeys=None, device: int = 0) -> List[str]:
    """Same file conventions as the reference script: reads `<pred_prefix>.<chr>.C.bed` and
    `<motif_folder>/motif_<chr>_C.bed`, writes `<pred_prefix>_clusterCpG.<chr>.C.bed`."""
    model = ClusterModel.from_checkpoint(model_prefix, device)
    written = []
    for chrom in (chrkeys or CHRKEYS):
        motif_path = "%s/motif_%s_C.bed" % (motif_folder, chrom)
        pred_path = "%s.%s.C.bed" % (pred_prefix, chrom)
        if not os.path.isfile(motif_path):
            print("Warning_motif!!! no file {}".format(motif_path))
            continue
        if not os.path.isfile(pred_path):
            print("Warning_pred!!! no file {}".format(pred_path))
            continue
        pred = read_pred(pred_path, chrom, read_motif(motif_path))
        x, lines = cluster_features(pred)
        if len(lines) == 0:
            continue
        p = model.predict(x)
        new_pct = (p * np.float32(100)).astype(np.int64)       # int(float32 p * 100)   (:170)
        out_path = "%s_clusterCpG.%s.C.bed" % (pred_prefix, chrom)
        with open(out_path, "w") as fh:
            for ln, v in zip(lines, new_pct.tolist()):
                fh.write("{} {}\n".format(ln, v))
        written.append(out_path)
    model.close()
    return written
