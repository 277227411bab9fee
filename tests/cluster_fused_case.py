"""TEST INFRASTRUCTURE for tests/test_cluster_fused.py and tests/test_gpu_cluster_fused.py (detect --clusterCpG): synthetic contigs with their
per-position counters, and the CHAIN the new stage is held to - the BED text of the counters (summary.bed_lines_py, the reference's writer) through
merge.sum_chr_mod -> motif.generate_motif_pos -> cluster.read_motif / read_pred / cluster_features, on files, as the three tools run."""
import atexit
import functools
import os
import shutil
import tempfile

import numpy as np

from deepmod_amd import cluster, merge, motif, summary

CHROM = 'chrT'
LENGTHS = (1, 2, 26, 51, 52, 255, 256, 257, 70001)     # 70,001: 69 tiles of the kernels (1,024 positions) and no multiple of one


def make_case(length: int, tail: str = 'CG', seed: int = 3, drop_minus: bool = False):
    """-> (seq, cov_p, mod_p, cov_m, mod_m).  CG-rich random bases with lower-case and N bases; `CG` at positions 0-1; at the end `CG`
    (tail 'CG') or an isolated C as the last base (tail 'C'); from 255 positions on a CGCG... run of 130 bases (its middle sites have the
    maximum of 49 neighbours: 51 positions less the site and its partner) and, from 70,001, runs across the kernels' tile boundaries at 1,024 and 2,048, a CpG without any neighbour whose
    partner has mod == 0, one row for every pct 0..100 (pct 0 as mod 1 of cov 200), cov > 1000, mod == 0 with cov > 0 next to sites, and
    counters on positions that are no site of their strand."""
    rng = np.random.default_rng(seed + length)
    s = rng.choice(np.frombuffer(b'ACGT', np.uint8), length, p=[0.15, 0.35, 0.35, 0.15])
    if length >= 2:
        s[0:2] = (ord('C'), ord('G'))
    runs = []
    if length >= 255:
        runs.append((60, 130))
    if length >= 70001:
        runs += [(960, 140), (2048 - 61, 122)]
        s[5000:5130] = ord('A')                          # a lone CpG: nothing within 25 positions
        s[5060:5062] = (ord('C'), ord('G'))
    for start, n in runs:
        s[start:start + n] = np.tile(np.frombuffer(b'CG', np.uint8), n // 2)
    if tail == 'CG' and length >= 4:
        s[-2:] = (ord('C'), ord('G'))
    elif tail == 'C':
        s[-1] = ord('C')
        if length >= 3:
            s[-2] = ord('A')
    low = rng.random(length) < 0.1
    s = np.where(low, s + 32, s).astype(np.uint8)
    if length >= 26:
        s[rng.integers(10, length - 3, max(1, length // 100))] = ord('N')
        for start, n in runs:                            # (the runs stay whole)
            s[start:start + n] = np.where(low[start:start + n], 32, 0) + np.tile(np.frombuffer(b'CG', np.uint8), n // 2)
    up = np.where(s >= 97, s - 32, s)
    plus_site = np.r_[(up[:-1] == ord('C')) & (up[1:] == ord('G')), False]
    minus_site = np.r_[False, plus_site[:-1]]
    out = []
    for st, site in enumerate((plus_site, minus_site)):
        cov = np.zeros(length, np.int64)
        mod = np.zeros(length, np.int64)
        idx = np.flatnonzero(site)
        cov[idx] = rng.integers(1, 60, len(idx))
        mod[idx] = (cov[idx] * rng.random(len(idx)) ** 0.7 + rng.random(len(idx))).astype(np.int64).clip(0, cov[idx])
        gone = rng.random(len(idx)) < 0.12
        mod[idx[gone]] = 0                               # covered, never called modified: no row after sum_chr_mod, no site, no neighbour
        cov[idx[rng.random(len(idx)) < 0.04]] = 0
        mod = np.minimum(mod, cov)
        if runs:                                         # the first run is modified throughout: 49 neighbours for the sites in its middle
            full = idx[(idx >= runs[0][0]) & (idx < runs[0][0] + runs[0][1])]
            cov[full] = np.maximum(cov[full], 2)
            mod[full] = np.maximum(mod[full], 1)
        if length >= 70001:
            pick = idx[(idx > 6000) & (idx < 60000)][st::7][:104]
            assert len(pick) == 104
            cov[pick[:101]], mod[pick[:101]] = 100, np.arange(101)
            cov[pick[0]], mod[pick[0]] = 200, 1          # a site with frac 0
            cov[pick[101:]], mod[pick[101:]] = (1500, 1001, 4000), (700, 1001, 39)
            if st == 1:
                cov[5061], mod[5061] = 9, 0              # the lone CpG: '+' site at 5060 without partner
            else:
                cov[5060], mod[5060] = 7, 3
        other = np.flatnonzero(~site)                    # rows that are no CpG C of this strand (on any base, also on the other strand's sites)
        other = other[rng.random(len(other)) < 0.3]
        cov[other] = rng.integers(0, 9, len(other))
        mod[other] = (cov[other] * rng.random(len(other))).astype(np.int64)
        if tail == 'C':
            cov[-1], mod[-1] = 5, 4                      # modified, but no G follows: not a site
        out += [cov.astype(np.int32), mod.astype(np.int32)]
    if drop_minus:
        out[2][:] = 0
        out[3][:] = 0
    return (s.tobytes().decode('ascii'),) + tuple(out)


def touch_of(cov, mod):
    """Counters as dm_summary_add leaves them: every covered position is touched; some more are touched only."""
    touch = cov.copy()
    touch[::5] += 1
    return touch


@functools.lru_cache(maxsize=None)
def chain(length: int, tail: str = 'CG', drop_minus: bool = False):
    """The case and what the three tools make of it, computed once: {'case', 'x' float64 [n, 14], 'lines', 'pred_text', 'motif_text', 'folder'
    (holds run/mod_pos.*, run.<chr>.C.bed, motif/ and genome.fa for cluster.hm_cluster_predict)}.  Nobody changes the result."""
    case = make_case(length, tail, drop_minus=drop_minus)
    seq, cov_p, mod_p, cov_m, mod_m = case
    folder = tempfile.mkdtemp(prefix='dm_cluster_chain_')
    atexit.register(shutil.rmtree, folder, True)
    os.makedirs(os.path.join(folder, 'run'))
    for strand, cov, mod in (('+', cov_p, mod_p), ('-', cov_m, mod_m)):
        text = summary.bed_lines_py(CHROM, strand, 'C', touch_of(cov, mod), cov, mod)
        if text:                                          # detect writes no file for an empty table
            with open(os.path.join(folder, 'run', 'mod_pos.%s%s.C.bed' % (CHROM, strand)), 'wb') as fh:
                fh.write(text)
    fasta = os.path.join(folder, 'genome.fa')
    with open(fasta, 'w') as fh:
        fh.write('>%s synthetic\n' % CHROM)
        fh.write(''.join(seq[i:i + 60] + '\n' for i in range(0, len(seq), 60)))
    merge.sum_chr_mod(folder, 'C', 'run', chrkeys=[CHROM], verbose=False)
    motif.generate_motif_pos(fasta, os.path.join(folder, 'motif'), 'C', 'CG', 0, [CHROM])
    motif_path = os.path.join(folder, 'motif', 'motif_%s_C.bed' % CHROM)
    pred_path = os.path.join(folder, 'run.%s.C.bed' % CHROM)
    pred = cluster.read_pred(pred_path, CHROM, cluster.read_motif(motif_path))
    x, lines = cluster.cluster_features(pred)
    return {'case': case, 'x': x, 'lines': lines, 'n_plus': len(pred['+'][0]), 'pred_text': open(pred_path).read(), 'motif_text': open(motif_path).read(),
            'folder': folder, 'fasta': fasta}


def records_of(lines):
    """(pos, cov, mod) of the chain's rows."""
    cols = [ln.split() for ln in lines]
    return (np.array([int(c[1]) for c in cols], np.int64), np.array([int(c[9]) for c in cols], np.int64), np.array([int(c[11]) for c in cols], np.int64))


def assert_run_is_no_empty_comparison(ch):
    """The conditions the 70,001-position run has to meet, on the chain's own output."""
    x = ch['x']
    assert len(x) >= 1000
    assert (x[:, 2] >= 1).sum() * 2 >= len(x)
    pos, _, _ = records_of(ch['lines'])
    plus, minus = set(pos[:ch['n_plus']].tolist()), set(pos[ch['n_plus']:].tolist())
    assert sum(1 for p in plus if p + 1 in minus) >= 100
    assert (x[:, 3:] > 0).any(axis=0).all()                              # all 11 bins hold neighbours
    # the CGCG run's maximum: all 51 positions of the window are sites, less the site itself and its partner; and a site without neighbours
    assert x[:, 2].max() == 49 and (x[:, 2] == 0).any()
    own_bins = set((x[:, 0] / 0.1 + 0.5).astype(int).tolist())
    assert own_bins == set(range(11)) and (x[:, 0] == 0).any()            # a site with frac 0 (mod 1 of cov 200)
    assert set(range(101)) <= set(np.rint(x[:, 0] * 100).astype(int).tolist())
    assert any(int(ln.split()[9]) > 1000 for ln in ch['lines'])


def slices_of(length: int, world: int):
    """[(first, count)] as dm_summary_reduce_scatter cuts a table of `length` positions over `world` ranks."""
    chunk = -(-length // world)
    return [(min(length, r * chunk), min(length, (r + 1) * chunk) - min(length, r * chunk)) for r in range(world)]
