"""The long inputs of tests/long_cases.py, held on the CPU with the oracles alone: the conditions that make the GPU tests of the table commands past
their grid wraps and scan carries meaningful.  Each count is past the constant it has to cross; every fate and counter is non-zero
on both strands; no key on the edge of the inclusion rule is kept; the planted contexts and sites lie in the tiles and element ranges the GPU tests
name."""
import numpy as np
import pytest

import diffmod_synth
import diffrep_synth
import long_cases
from deepmod_amd import diffmod, motifs

COV, FDR = diffmod_synth.COV, diffmod_synth.FDR
MOTIF_RULE = (5, 50, 10)                            # COV, T_PCT, U_PCT of tests/test_gpu_motifs.py


@pytest.fixture(scope='module')
def tile():
    t = diffmod.tile_positions()
    assert t == motifs.tile_positions() == 1024
    return t


def test_the_long_contig_wraps_the_sweep_grid_and_the_tile_scan(tile):
    n = long_cases.wrap_length(tile)
    tiles = (n + tile - 1) // tile
    assert tiles == 2050 > long_cases.SWEEP_BLOCKS and tiles > long_cases.SCAN_GROUP and n % tile == 5
    carry = long_cases.carry_length(tile)
    assert long_cases.SCAN_GROUP < (carry + tile - 1) // tile == 258 <= long_cases.SWEEP_BLOCKS


def test_diffmod_sweep_keys_on_the_long_contig(tile):
    small = diffmod.small_support()
    n, recs = long_cases.diffmod_wrap(tile, small, diffmod.MAX_TOTAL)
    counters, rec = long_cases.diffmod_wrap_oracle(tile, small, diffmod.MAX_TOTAL)
    assert (counters > 0).all() and counters[:, 0].sum() == len(rec['p']) > 5000                # every fate on both strands
    held = long_cases.tiles_holding(rec['pos'], tile)
    assert set(long_cases.WRAP_TILE_SET) == {0, 255, 256, 257, 2047, 2048, 2049} <= held
    for lo, hi in ((255, 257), (2047, 2049)):                         # keys of both strands around the first scan-group edge and around the wrap edge
        around = (rec['pos'] // tile >= lo) & (rec['pos'] // tile <= hi)
        assert set(rec['strand'][around].tolist()) == {0, 1}
    keep = rec['p'] <= FDR
    assert 0 < keep.sum() < len(keep)


def test_diffmod_chunk_keys(tile):
    n, recs, keys, dropped, tested = long_cases.diffmod_chunks(tile)
    assert n == long_cases.wrap_length(tile)
    assert tested > long_cases.SCAN_GROUP * long_cases.SCAN_GROUP + long_cases.SCAN_GROUP == 65792
    assert len(set(keys)) == len(keys) == long_cases.CHUNK_DISTINCT and max(max(k[0], k[2]) for k in keys) <= 40
    assert not any(diffmod_synth.on_edge(*k) for k in keys) and dropped <= 0.01 * (len(keys) + dropped)
    for role in ('sample', 'control'):
        pos, strand = recs[role][:2]
        assert len(np.unique(2 * pos + strand)) == len(pos) == long_cases.CHUNK_PLACED and pos.max() < n
    counters, rec = long_cases.diffmod_chunks_oracle(tile)
    assert counters[:, 0].sum() == tested == len(rec['p']) and (counters[:, :3] > 0).all()
    group = long_cases.SCAN_GROUP * long_cases.SCAN_GROUP             # work items of one group of chunk counts
    keep = rec['p'] <= FDR
    assert keep[:group].any() and keep[group:].any() and not keep.all()
    assert (np.diff(keep.astype(np.int64)) != 0).sum() > 1000         # the records to compact are scattered among the others


def test_diffmod_large_keys():
    n, recs, n_large = long_cases.diffmod_large()
    small = diffmod.small_support()
    pos, strand, cA, mA = recs['sample']
    cB, mB = recs['control'][2:]
    large = np.array([long_cases.support_of(*k) > small for k in zip(cA.tolist(), mA.tolist(), cB.tolist(), mB.tolist())])
    assert large.sum() == n_large >= 1100 > long_cases.LARGE_BLOCKS and large[0::2].all() and not large[1::2].any()
    assert {tuple(k) for k in np.stack([cA, mA, cB, mB], axis=1)[large].tolist()} == set(long_cases.LARGE_KEYS)
    assert not any(diffmod_synth.on_edge(*k) for k in set(zip(cA.tolist(), mA.tolist(), cB.tolist(), mB.tolist())))
    assert (np.minimum(cA, cB) >= COV).all()                          # every key is tested


@pytest.mark.parametrize('shape,which,phase', long_cases.REP_CASES)
def test_diffrep_keys_on_the_long_contigs(tile, shape, which, phase):
    n, (a, b), recs = long_cases.diffrep_case(shape, which, phase, tile)
    tiles = (n + tile - 1) // tile
    assert tiles > long_cases.SCAN_GROUP and (which != 'wrap' or tiles > long_cases.SWEEP_BLOCKS) and len(recs) == sum(shape)
    counters, rec = long_cases.diffrep_oracle(shape, which, phase, tile)
    assert (counters > 0).all() and counters[:, 0].sum() == len(rec['p'])                        # every fate on both strands
    held = long_cases.tiles_holding(rec['pos'], tile)
    assert {0, 255, 256, 257, tiles - 1} <= held and (which != 'wrap' or set(long_cases.WRAP_TILE_SET) <= held)
    keep = rec['p'] <= diffrep_synth.FDR
    assert 0 < keep.sum() < len(keep) and (rec['p'] == 1.0).sum() >= 2


def test_motif_sites_of_the_long_contig(tile):
    from test_gpu_motifs import RULE_EDGES
    seq, recs, planted = long_cases.motifs_case(tile, tuple(RULE_EDGES))
    n = len(seq)
    assert n == long_cases.wrap_length(tile) and (n + tile - 1) // tile > long_cases.SWEEP_BLOCKS
    assert {p // tile for p in planted['edges']} == {2047, 2048, 2049} and {p // tile for p in planted['ends']} == {0, 2049}
    assert [p // tile for p in planted['shared']] == [0, long_cases.SWEEP_BLOCKS]               # one workgroup's two tiles
    for up, down in ((3, 3), (4, 4)):
        bins = [long_cases.motif_bin_of(seq, recs, p, up, down, MOTIF_RULE) for p in planted['shared']]
        assert bins[0] == bins[1] >= 0, (up, down, bins)
    host = motifs.HostEngine(4, 4, long_cases.MOTIF_BASE, *MOTIF_RULE)
    tabs = long_cases.motif_host_tables(recs['sample'], n) + long_cases.motif_host_tables(recs['control'], n)
    counters, off_base = host.count(seq, *tabs)
    assert (counters > 0).all() and (off_base > 0).all() and counters[:, 0].min() > 50000       # every counter on both strands
    own = {0: ord(long_cases.MOTIF_BASE), 1: ord(long_cases.COMP[long_cases.MOTIF_BASE])}
    letters = np.frombuffer(seq, np.uint8)
    pos, strand = recs['sample'][:2]
    for s in (0, 1):                                                  # records on the planted sites beside both tile edges and at both ends
        on = set(pos[(strand == s) & (letters[pos] == own[s])].tolist())
        assert {p for p in planted['edges'] + planted['ends'] if letters[p] == own[s]} <= on


def test_cluster_sites_of_the_long_contig():
    seq, cov_p, mod_p, cov_m, mod_m = long_cases.cluster_case()
    tiles = (len(seq) + long_cases.SITE_TILE - 1) // long_cases.SITE_TILE
    assert len(seq) == 1029 * 1024 + 7 and tiles == long_cases.SITE_TILES and 2 * tiles == 2060 > 2 * long_cases.SITE_SCAN
    assert all((m <= c).all() and c.max() <= 12 and m.min() >= 0 for c, m in ((cov_p, mod_p), (cov_m, mod_m)))
    assert 0.05 < (cov_p > 0).mean() < 0.1                            # sparse: the rows of the fill stay a few MB
    want = long_cases.cluster_oracle()
    n_plus = want['n_plus']
    assert 8000 < len(want['pos']) < 20000 and 4000 < n_plus < len(want['pos']) - 4000
    held = long_cases.scanned_indices(want)
    assert {0, 1023, 1024, tiles - 1, tiles, 2047, 2048, 2 * tiles - 1} <= held                 # both sides of index 1,024 and of index 2,048
    assert (want['pos'][:n_plus] // long_cases.SITE_TILE >= long_cases.SITE_SCAN).any()
    cut = long_cases.SITE_CUT
    assert cut % long_cases.SITE_TILE == 0 and (want['pos'] < cut).any() and (want['pos'] >= cut).any()


def test_bsperf_records_and_elements():
    cov, mod, recs, scores = long_cases.bsperf_case()
    length, grid = cov.shape[1], long_cases.RECORD_GRID
    assert length == long_cases.BSPERF_LENGTH and 2 * grid < 2 * length < 3 * grid               # three passes of the sweep
    assert len(recs) == 2 and all(len(r[0]) > grid for r in recs) and len(scores[0]) > grid
    for pos, strand, _, _ in list(recs) + [scores[:2] + (None, None)]:
        assert len(np.unique(strand * length + pos)) == len(pos)      # distinct keys: no replicate is refused
    e = long_cases.bsperf_joined_elements()
    assert all(((e >= lo) & (e < hi)).sum() > 1000 for lo, hi in ((0, grid), (grid, 2 * grid), (2 * grid, 2 * length)))


def test_siteperf_records_and_elements():
    seq, batches = long_cases.siteperf_case()
    grid = long_cases.RECORD_GRID
    assert len(seq) == long_cases.SITEPERF_LENGTH and grid < 2 * len(seq) < 2 * grid
    assert [len(rec[0]) for _, rec in batches] == [300000, 300000, 20000] and [role for role, _ in batches] == [0, 1, 1]
    for _, rec in batches[:2]:
        e = 2 * rec[0] + rec[1]
        assert (e < grid).sum() > 1000 and (e >= grid).sum() > 1000 and rec[0].max() < len(seq)
