"""TEST INFRASTRUCTURE - not part of the product.  The long inputs of the table commands: shapes past the point where a grid capped at
MAX_BLOCKS wraps and a one-workgroup scan takes a second group and carries its running total.  tests/test_long_cases.py holds, with the oracles
alone, the conditions that make the GPU tests of these inputs meaningful; the GPU tests (tests/test_gpu_diffmod.py, test_gpu_diffrep.py,
test_gpu_motifs.py, test_gpu_cluster_fused.py, test_gpu_bsperf.py, test_gpu_siteperf.py) run them on the device.

Everything long is built vectorised in numpy.  Builders and oracle results are cached: the CPU and the GPU tests of one process share them and
leave them unchanged.

The literal counts below mirror constants of the kernels; a GPU test asserts with them that it crossed its threshold, so raising a constant makes
the test fail on that assertion and not pass emptily:
    SWEEP_BLOCKS   dfk::MAX_BLOCKS = mok::MAX_BLOCKS = 2048   the grid of the tile sweeps of diffmod, diffmod --replicates and motifs
    SCAN_GROUP     dfk::THREADS = 256                         counts per group of dfk::scan_kernel; also dfk::CHUNK, the work items per chunk
    LARGE_BLOCKS   dfk::LARGE_BLOCKS = 1024                   the grid of fisher_kernel<true>
    SITE_SCAN      csites::SCAN_THREADS = 1024                values per pass of csites::site_scan_kernel
    RECORD_GRID    bsk::MAX_BLOCKS * bsk::THREADS = spk::MAX_BLOCKS * spk::THREADS = bmk::MAX_BLOCKS * bmk::THREADS = 1024 * 256
                                                              the threads of the record and sweep kernels of bsperf, siteperf and merge
    LABEL_GRID     blk::MAX_BLOCKS * blk::THREADS = 2048 * 256   the threads of bl_class_kernel
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffmod_synth  # noqa: E402
import diffrep_synth  # noqa: E402

SWEEP_BLOCKS = 2048
SCAN_GROUP = 256
LARGE_BLOCKS = 1024
SITE_SCAN = 1024
RECORD_GRID = 1024 * 256
LABEL_GRID = 2048 * 256

WRAP_TILES = SWEEP_BLOCKS + 1                       # whole tiles of the long contig; its ragged last tile is tile WRAP_TILES
WRAP_TILE_SET = (0, SCAN_GROUP - 1, SCAN_GROUP, SCAN_GROUP + 1, SWEEP_BLOCKS - 1, SWEEP_BLOCKS, SWEEP_BLOCKS + 1)
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}


def wrap_length(tile: int) -> int:
    """2,050 tiles: workgroup 0 takes tiles 0 and 2,048, workgroup 1 tile 1 and the ragged 2,049."""
    return WRAP_TILES * tile + 5


def carry_length(tile: int) -> int:
    """258 tiles: the scan of the tile counts takes a second group, no grid wraps."""
    return (SCAN_GROUP + 1) * tile + 1


def tiles_holding(pos, tile: int) -> set:
    return set((np.asarray(pos, np.int64) // tile).tolist())


def _as_records(rows):
    return tuple(np.ascontiguousarray(a, np.int64) for a in rows)


# ---- diffmod ------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def diffmod_wrap(tile: int, small_support: int, max_total: int, phase: int = 0):
    """1a: the sweep keys of diffmod_synth on both sides of every tile edge of the long contig -> (n, recs)."""
    n = wrap_length(tile)
    return n, diffmod_synth.layout(diffmod_synth.sweep_keys(small_support, max_total), n, tile, phase)


@functools.lru_cache(maxsize=None)
def diffmod_wrap_oracle(tile: int, small_support: int, max_total: int):
    """HostEngine under alpha 1 on diffmod_wrap -> (counters, records)."""
    from deepmod_amd import diffmod
    n, recs = diffmod_wrap(tile, small_support, max_total)
    return diffmod.HostEngine(diffmod_synth.COV, 1.0).run(*(diffmod_synth.host_tables(recs['sample'], n) + diffmod_synth.host_tables(recs['control'], n)))


CHUNK_DISTINCT = 60
CHUNK_PLACED = 96000


@functools.lru_cache(maxsize=None)
def diffmod_chunks(tile: int):
    """1b: CHUNK_DISTINCT small random keys (coverages <= 40, on-edge keys dropped by random_keys) on CHUNK_PLACED distinct random (position, strand)
    of the long contig -> (n, recs, keys, dropped, tested): `tested` the number of placed keys deep enough in the sample and in the controls."""
    n = wrap_length(tile)
    keys, dropped = diffmod_synth.random_keys(31, CHUNK_DISTINCT, 40)
    rng = np.random.default_rng(32)
    at = rng.choice(2 * n, CHUNK_PLACED, replace=False)
    which = rng.integers(0, len(keys), CHUNK_PLACED)
    k = np.array(keys, np.int64)[which]
    pos, strand = at >> 1, at & 1
    recs = {'sample': _as_records((pos, strand, k[:, 0], k[:, 1])), 'control': _as_records((pos, strand, k[:, 2], k[:, 3]))}
    tested = int(((k[:, 0] >= diffmod_synth.COV) & (k[:, 2] >= diffmod_synth.COV)).sum())
    return n, recs, keys, dropped, tested


@functools.lru_cache(maxsize=None)
def diffmod_chunks_oracle(tile: int):
    from deepmod_amd import diffmod
    n, recs = diffmod_chunks(tile)[:2]
    return diffmod.HostEngine(diffmod_synth.COV, 1.0).run(*(diffmod_synth.host_tables(recs['sample'], n) + diffmod_synth.host_tables(recs['control'], n)))


LARGE_KEYS = ((5000, 2600, 5000, 2400), (5000, 5000, 5000, 0), (700, 10, 900, 600))      # the second underflows
LARGE_POSITIONS = 1200


def support_of(cA, mA, cB, mB) -> int:
    return min(cA, mA + mB) - max(0, mA + mB - cB) + 1


@functools.lru_cache(maxsize=None)
def diffmod_large():
    """1c: element e = 2 position + strand holds LARGE_KEYS[(e / 2) % 3] where e is even and a small key where it is odd -> (n, recs, large keys placed)."""
    n = LARGE_POSITIONS
    small, _ = diffmod_synth.random_keys(33, 24, 40)
    small = [k for k in small if k[0] >= diffmod_synth.COV and k[2] >= diffmod_synth.COV]
    e = np.arange(2 * n)
    big = np.array(LARGE_KEYS, np.int64)[(e // 2) % len(LARGE_KEYS)]
    little = np.array(small, np.int64)[(e // 2) % len(small)]
    k = np.where((e % 2 == 0)[:, None], big, little)
    pos, strand = e >> 1, e & 1
    recs = {'sample': _as_records((pos, strand, k[:, 0], k[:, 1])), 'control': _as_records((pos, strand, k[:, 2], k[:, 3]))}
    return n, recs, n


# ---- diffmod --replicates ---------------------------------------------------------------------------------------------------------------------------

REP_CASES = (((2, 2), 'wrap', 3), ((8, 8), 'carry', 0))       # (shape, which length, phase: odd takes the least counts one below the default)


def rep_device_keys(keys):
    """The keys a table filled from files can hold: 0 <= m <= c, and no coverage near 2^31 (merge refuses sums past int32)."""
    return [diffrep_synth.held(k) for k in keys if max(k[0]) < 2 ** 30]


@functools.lru_cache(maxsize=None)
def diffrep_case(shape, which: str, phase: int, tile: int):
    """-> (n, (a, b), recs per replicate) of diffrep_synth.layout on the long contig ('wrap') or on the one of 258 tiles ('carry')."""
    KA, KB = shape
    n = wrap_length(tile) if which == 'wrap' else carry_length(tile)
    a, b = diffrep_synth.low_min_reps(KA, KB) if phase % 2 else (KA, KB)
    keys = rep_device_keys(diffrep_synth.sweep_keys(KA, KB, a, b))
    return n, (a, b), diffrep_synth.layout(keys, KA + KB, n, tile, phase)


def diffrep_host_tables(shape, which: str, phase: int, tile: int):
    n, _, recs = diffrep_case(shape, which, phase, tile)
    return [diffrep_synth.host_tables(rec, n) for rec in recs]


@functools.lru_cache(maxsize=None)
def diffrep_oracle(shape, which: str, phase: int, tile: int):
    """RepHostEngine under alpha 1 -> (counters, records)."""
    from deepmod_amd import diffmod
    (a, b) = diffrep_case(shape, which, phase, tile)[1]
    tabs = diffrep_host_tables(shape, which, phase, tile)
    return diffmod.RepHostEngine(diffrep_synth.COV, 1.0, a, b).run(tabs[:shape[0]], tabs[shape[0]:])


# ---- motifs -----------------------------------------------------------------------------------------------------------------------------------------

MOTIF_BASE = 'A'
MOTIF_CONTEXT = 'CGTCACTGA'                         # planted with its A at SHARED_OFFSET of tile 0 and of tile SWEEP_BLOCKS: one bin, one workgroup, two tiles
SHARED_OFFSET = 500
MOTIF_SITE_SHARE = 0.2
MOTIF_OFF_SHARE = 0.01


@functools.lru_cache(maxsize=None)
def motifs_case(tile: int, rule_edges: tuple):
    """Random letters of the long contig; sites planted as test_gpu_motifs.make_sequence plants them (variant 0, flank (4, 4)) at the tile edges
    2,047 | 2,048 and 2,048 | 2,049 and at both contig ends; MOTIF_CONTEXT in tile 0 and in tile 2,048.  Records: rule_edges in turn on a random
    fifth of the sites of either strand and on every planted site, and off-base records on a hundredth of the other positions
    -> (seq bytes, recs, planted: {'edges': [positions], 'ends': [positions], 'shared': [positions]})."""
    n = wrap_length(tile)
    rng = np.random.default_rng(41)
    seq = rng.choice(np.frombuffer(b'ACGT', np.uint8), n)
    own, other = ord(MOTIF_BASE), ord(COMP[MOTIF_BASE])
    up = down = 4
    edges = []
    for edge in (SWEEP_BLOCKS * tile, (SWEEP_BLOCKS + 1) * tile):
        seq[edge - 2], seq[edge + 1], seq[edge - 1], seq[edge] = other, other, own, own
        edges += [edge - 2, edge - 1, edge, edge + 1]
    plus, minus = [up, up - 1, n - 1 - down, n - down, 1], [down, down - 1, n - 1 - up, n - up, 2]       # (1 and 2: a context that leaves the contig under (3, 3) too)
    for positions, letter in ((plus, own), (minus, other)):           # where both want a position, the later one has it
        for p in positions:
            seq[p] = letter
    ctx = np.frombuffer(MOTIF_CONTEXT.encode(), np.uint8)
    mid = MOTIF_CONTEXT.index(MOTIF_BASE, 3)
    shared = [SHARED_OFFSET, SWEEP_BLOCKS * tile + SHARED_OFFSET]
    for p in shared:
        seq[p - mid:p - mid + len(ctx)] = ctx
    planted = {'edges': edges, 'ends': sorted(set(plus + minus)), 'shared': shared}
    must = np.zeros(n, bool)
    must[edges + planted['ends']] = True
    rows = {'sample': [], 'control': []}
    edge_table = np.array(rule_edges, np.int64)
    for s, letter in enumerate((own, other)):
        is_site = seq == letter
        taken = is_site & (must | (rng.random(n) < MOTIF_SITE_SHARE))
        taken[shared] = False
        p = np.nonzero(taken)[0]
        v = edge_table[(np.arange(len(p)) + s) % len(edge_table)]
        off = np.nonzero(~is_site & (rng.random(n) < MOTIF_OFF_SHARE))[0]
        for role, cv, md, off_row in (('sample', v[:, 0], v[:, 1], (7, 3)), ('control', v[:, 2], v[:, 3], (9, 0))):
            have = cv > 0
            rows[role].append((p[have], np.full(int(have.sum()), s), cv[have], md[have]))
            rows[role].append((off, np.full(len(off), s), np.full(len(off), off_row[0]), np.full(len(off), off_row[1])))
    for role, row in (('sample', (30, 30)), ('control', (30, 0))):    # the shared context on '+': tested and modified under every rule here
        rows[role].append((np.array(shared), np.zeros(2, np.int64), np.full(2, row[0]), np.full(2, row[1])))
    recs = {role: _as_records(np.concatenate([r[j] for r in parts]) for j in range(4)) for role, parts in rows.items()}
    return seq.tobytes(), recs, planted


def motif_host_tables(rec, n: int):
    tabs = [(np.zeros(n, np.int64), np.zeros(n, np.int64)) for _ in range(2)]
    pos, strand, cov, mod = rec
    for s in range(2):
        sel = strand == s
        tabs[s][0][pos[sel]] = cov[sel]
        tabs[s][1][pos[sel]] = mod[sel]
    return tabs


def motif_bin_of(seq: bytes, recs, p: int, up: int, down: int, rule) -> int:
    """The bin the '+' key at position p is tested in (-1: it is not tested): HostEngine on the window of p alone."""
    from deepmod_amd import motifs
    lo, hi = p - 8, p + 9
    host = motifs.HostEngine(up, down, MOTIF_BASE, *rule)
    tabs = []
    for role in ('sample', 'control'):
        pos, strand, cov, mod = recs[role]
        sel = (pos == p) & (strand == 0)
        tabs += motif_host_tables((pos[sel] - lo, strand[sel], cov[sel], mod[sel]), hi - lo)
    host.count(seq[lo:hi], *tabs)
    hit = np.nonzero(host.fetch()[:, 0])[0]
    return int(hit[0]) if len(hit) == 1 else -1


# ---- the CpG-cluster site stage -----------------------------------------------------------------------------------------------------------------------

SITE_TILE = 1024                                    # csites::TILE
SITE_TILES = SITE_SCAN + 6                          # 1,030 tiles: 2,060 scanned values in three passes
SITE_COUNT = (SITE_TILES - 1) * SITE_TILE + 7
SITE_CUT = 512 * SITE_TILE
SITE_PLANTED_TILES = (0, SITE_SCAN - 7, SITE_SCAN - 6, SITE_SCAN - 1, SITE_SCAN, SITE_TILES - 1)
SITE_COVERED = 0.08


@functools.lru_cache(maxsize=None)
def cluster_case():
    """Random bases of SITE_COUNT positions, coverage (<= 12, mostly with modified reads) on SITE_COVERED of the positions of either strand, and a CpG
    with modified reads on both strands planted at offset 100 of SITE_PLANTED_TILES: '+' tiles SITE_SCAN - 1 | SITE_SCAN lie on both sides of scanned
    index 1,024, '-' tiles SITE_SCAN - 7 | SITE_SCAN - 6 on both sides of scanned index 2,048 -> (seq bytes, cov_p, mod_p, cov_m, mod_m) int64."""
    rng = np.random.default_rng(51)
    n = SITE_COUNT
    seq = rng.choice(np.frombuffer(b'ACGT', np.uint8), n, p=[0.2, 0.3, 0.3, 0.2])               # a CpG on 9 % of the positions
    tabs = []
    for _ in range(2):
        cov = np.where(rng.random(n) < SITE_COVERED, rng.integers(1, 13, n), 0)
        mod = np.where(rng.random(n) < 0.8, (cov * rng.random(n) + 0.5).astype(np.int64), 0)
        tabs += [cov.astype(np.int64), np.minimum(mod, cov).astype(np.int64)]
    for t in SITE_PLANTED_TILES:
        p = min(t * SITE_TILE + 100, n - 3)
        seq[p], seq[p + 1] = ord('C'), ord('G')
        tabs[0][p], tabs[1][p] = 10, 7
        tabs[2][p + 1], tabs[3][p + 1] = 9, 3
    return (seq.tobytes(),) + tuple(tabs)


@functools.lru_cache(maxsize=None)
def cluster_oracle():
    from deepmod_amd import cluster
    return cluster.sites_from_counters(*cluster_case())


def scanned_indices(got) -> set:
    """The indices into [tiles of '+' | tiles of '-'] of site_scan_kernel that hold a site."""
    n_plus = got['n_plus']
    pos = np.asarray(got['pos'], np.int64)
    return tiles_holding(pos[:n_plus], SITE_TILE) | {SITE_TILES + t for t in tiles_holding(pos[n_plus:], SITE_TILE)}


# ---- bsperf -------------------------------------------------------------------------------------------------------------------------------------------

BSPERF_LENGTH = 300001                              # 2 * length: three passes of the RECORD_GRID threads of bs_count_kernel
BSPERF_KEYS = 400000
BSPERF_SCORES = 300000
BSPERF_RULE = ((1, 5, 10), 90, 0, 1)                # thresholds, methylated, unmethylated, pred_cov


@functools.lru_cache(maxsize=None)
def bsperf_case():
    """test_gpu_bsperf._random_case on BSPERF_LENGTH positions with BSPERF_KEYS keys, two replicates, and BSPERF_SCORES distinct scored keys
    -> (cov, mod, recs, scores)."""
    from test_gpu_bsperf import _random_case
    rng = np.random.default_rng(61)
    cov, mod, recs = _random_case(rng, BSPERF_LENGTH, 2, *BSPERF_RULE, BSPERF_KEYS)
    keys = rng.choice(2 * BSPERF_LENGTH, BSPERF_SCORES, replace=False)
    return cov, mod, recs, (keys % BSPERF_LENGTH, keys // BSPERF_LENGTH, rng.integers(0, 101, len(keys)))


def bsperf_joined_elements():
    """e = strand * length + position of the sites with truth in every replicate and a prediction of kind 0 (coverage >= pred_cov)."""
    cov, mod, recs, _ = bsperf_case()
    has = np.ones(2 * BSPERF_LENGTH, bool)
    for pos, strand, _, _ in recs:
        mine = np.zeros(2 * BSPERF_LENGTH, bool)
        mine[strand * BSPERF_LENGTH + pos] = True
        has &= mine
    return np.nonzero(has & (cov.reshape(-1) >= BSPERF_RULE[3]))[0]


# ---- siteperf -----------------------------------------------------------------------------------------------------------------------------------------

SITEPERF_LENGTH = 150001                            # 2 * len: two passes of the RECORD_GRID threads of sp_walk_kernel
SITEPERF_BATCH = 300000


@functools.lru_cache(maxsize=None)
def siteperf_case():
    """-> (seq, [(role, records)]): one RUN batch and one CONTROL batch of SITEPERF_BATCH random records, and a second CONTROL batch of 20,000."""
    from deepmod_amd import siteperf as sp
    from test_gpu_siteperf import random_records, random_seq
    rng = np.random.default_rng(71)
    seq = random_seq(rng, SITEPERF_LENGTH, 'CG', 12)
    batches = [(sp.RUN, random_records(rng, SITEPERF_BATCH, SITEPERF_LENGTH)), (sp.CONTROL, random_records(rng, SITEPERF_BATCH, SITEPERF_LENGTH)),
               (sp.CONTROL, random_records(rng, 20000, SITEPERF_LENGTH))]
    return seq, batches
