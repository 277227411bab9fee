"""GPU (-m gpu): the CpG-cluster stage from the counters on the device (detect --clusterCpG; csrc/cluster_sites.hip.inc) against the chain of the three
tools on files (tests/cluster_fused_case.py): counters filled through dm_summary_add, features bit-equal to cluster.cluster_features on the chain's
inputs, records equal, file bytes equal to cluster.hm_cluster_predict's - with the real checkpoint and with the synthetic weights of tests/test_cluster.py.
Then the command: `detect --clusterCpG` on feature containers against the four documented steps, with one rank, one rank through the scatter merge,
and two and three ranks over the shared-memory stand-in for the collective library (tests/shim)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_fused_case as cf
import long_cases
from conftest import ROOT
from deepmod_amd import _lib, cluster, merge, motif, summary, synth, synth_reads, tfbundle
from test_cluster import REAL, _synthetic_cluster_weights

pytestmark = pytest.mark.gpu

CASES = [(n, tail, False) for n in cf.LENGTHS[:-1] for tail in ('CG', 'C')] + [(70001, 'CG', False), (257, 'CG', True), (70001, 'CG', True)]


def filled(cov, mod, device):
    """A PositionSummary holding touch | cov | mod of the case, through dm_summary_add: per position `mod` rows called modified, `cov - mod` covered
    rows, and the rows of cf.touch_of that are touched only."""
    cov, mod = cov.astype(np.int64), mod.astype(np.int64)
    only = cf.touch_of(cov, mod) - cov
    idx = np.arange(len(cov), dtype=np.int64)
    pos = np.concatenate([np.repeat(idx, mod), np.repeat(idx, cov - mod), np.repeat(idx, only)])
    flags = np.concatenate([np.full(int(mod.sum()), 7, np.uint8), np.full(int((cov - mod).sum()), 3, np.uint8), np.full(int(only.sum()), 1, np.uint8)])
    s = summary.PositionSummary(len(cov), device)
    s.add(pos, flags)
    return s


@pytest.fixture(scope="module")
def models(gpu_device, tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp('cluster_model') / 'synthetic')
    tfbundle.write_bundle(prefix, _synthetic_cluster_weights())
    made = {'real': (REAL, cluster.ClusterModel.from_checkpoint(REAL, gpu_device)), 'synthetic': (prefix, cluster.ClusterModel.from_checkpoint(prefix, gpu_device))}
    yield made
    for _, m in made.values():
        m.close()


@pytest.mark.parametrize("length,tail,drop_minus", CASES)
def test_sites_features_records_and_file_equal_the_chain(gpu_device, models, length, tail, drop_minus):
    ch = cf.chain(length, tail, drop_minus)
    if length == 70001 and not drop_minus:
        cf.assert_run_is_no_empty_comparison(ch)
    seq, cov_p, mod_p, cov_m, mod_m = ch['case']
    plus = filled(cov_p, mod_p, gpu_device)
    minus = None if drop_minus else filled(cov_m, mod_m, gpu_device)            # one strand's summary absent
    t, c, m = plus.fetch()
    assert np.array_equal(t, cf.touch_of(cov_p, mod_p)) and np.array_equal(c, cov_p) and np.array_equal(m, mod_p)
    pos, cov, mod = cf.records_of(ch['lines'])
    for name, (prefix, model) in models.items():
        got = model.sites(plus, minus, seq, want_features=True)
        assert got['n_plus'] == ch['n_plus'] and got['features'].shape == (len(ch['lines']), 14)
        assert np.array_equal(got['features'], ch['x'].astype(np.float32))                     # bit-equal to the chain's feed
        assert np.array_equal(got['pos'], pos) and np.array_equal(got['cov'], cov) and np.array_equal(got['mod'], mod)
        written = cluster.hm_cluster_predict(os.path.join(ch['folder'], 'run'), os.path.join(ch['folder'], 'motif'), prefix, chrkeys=[cf.CHROM], device=gpu_device)
        text = b''.join(cluster.site_text_parts(cf.CHROM, 'C', got))
        if len(ch['lines']) == 0:
            assert written == [] and text == b''                                               # the chain writes no file: neither does the stage
        else:
            assert open(written[0], 'rb').read() == text
            os.remove(written[0])
    plus.close()
    if minus is not None:
        minus.close()


def joined(parts):
    out = {k: np.concatenate([p[k][:p['n_plus']] for p in parts] + [p[k][p['n_plus']:] for p in parts]) for k in ('pos', 'cov', 'mod', 'new', 'features')}
    out['n_plus'] = sum(p['n_plus'] for p in parts)
    return out


def test_slices_with_halos_join_to_the_whole_contig(gpu_device, models, tmp_path):
    """Ranges of the tables with the 26 counters beyond either end handed in as a rank receives them (cluster.halo_from_edges) and only the range +-27
    of the sequence: joined as rank 0 joins the parts they are the whole contig's result.  Cuts at thirds, between the C and the G of a pair, inside
    the CGCG run, at tile boundaries +-1; then the slice form after a reduce-scatter (a communicator of one rank: the slice is the table)."""
    from deepmod_amd import comm
    ch = cf.chain(70001)
    seq, cov_p, mod_p, cov_m, mod_m = ch['case']
    model = models['synthetic'][1]
    plus, minus = filled(cov_p, mod_p, gpu_device), filled(cov_m, mod_m, gpu_device)
    whole = model.sites(plus, minus, seq, want_features=True)
    assert np.array_equal(whole['features'], ch['x'].astype(np.float32))
    pair = next(p for p in whole['pos'][:whole['n_plus']].tolist() if p > 30000 and p + 1 in set(whole['pos'][whole['n_plus']:].tolist()))
    for cuts in ([f for f, _ in cf.slices_of(70001, 3)] + [70001], [0, 120, 1023, 1024, 1025, 2048, pair + 1, 69999, 70001]):
        slices = list(zip(cuts[:-1], np.diff(cuts).tolist()))
        everyone = [{"first": f, "count": c, "edges": cluster.slice_edges(*[a[f:f + c] for a in (cov_p, mod_p, cov_m, mod_m)])} for f, c in slices]
        parts = []
        for f, c in slices:
            lo, hi = max(0, f - 27), min(len(seq), f + c + 27)
            parts.append(model.sites(plus, minus, seq[lo:hi], f, c, halo=cluster.halo_from_edges(f, c, everyone), seq_first=lo, want_features=True))
        got = joined(parts)
        assert got['n_plus'] == whole['n_plus'] and all(np.array_equal(got[k], whole[k]) for k in ('pos', 'cov', 'mod', 'new', 'features'))
        # whole tables without a halo: the counters beside the range are read from the tables themselves
        got = joined([model.sites(plus, minus, seq, f, c, want_features=True) for f, c in slices])
        assert got['n_plus'] == whole['n_plus'] and all(np.array_equal(got[k], whole[k]) for k in ('pos', 'cov', 'mod', 'new', 'features'))
    with pytest.raises(_lib.DeepModHipError, match='no reduce-scatter result'):
        model.sites(plus, minus, seq, 0, 70001, from_slice=True)
    c = comm.Communicator.from_rendezvous(gpu_device, comm.FileRendezvous(str(tmp_path / 'rdv'), 0, 1))
    assert plus.reduce_scatter(c) == (0, 70001) and minus.reduce_scatter(c) == (0, 70001)
    got = model.sites(plus, minus, seq, 0, 70001, from_slice=True, want_features=True)
    assert got['n_plus'] == whole['n_plus'] and all(np.array_equal(got[k], whole[k]) for k in ('pos', 'cov', 'mod', 'new', 'features'))
    with pytest.raises(_lib.DeepModHipError, match='holds the slice'):
        model.sites(plus, minus, seq, 5, 100, from_slice=True)
    c.close()
    empty = model.sites(None, None, seq)
    assert len(empty['pos']) == 0 and empty['n_plus'] == 0
    plus.close()
    minus.close()


def test_site_scan_carries_over_three_passes(gpu_device, models):
    """1,030 tiles (long_cases.cluster_case): site_scan_kernel walks 2,060 values [tiles of '+' | tiles of '-'] in three passes of 1,024 and carries
    its total twice; against cluster.sites_from_counters, which tests/test_cluster_fused.py pins to the chain of the three tools.  Then as two ranges
    without a halo, cut at tile 512 (first > 0), joined."""
    seq, cov_p, mod_p, cov_m, mod_m = long_cases.cluster_case()
    count, tiles = len(seq), (len(seq) + 1023) // 1024
    assert count == long_cases.SITE_COUNT and 2 * tiles > 2 * 1024 and tiles > 1024        # csites::SCAN_THREADS: a third pass; '+' tiles in a second one
    want = long_cases.cluster_oracle()
    model = models['synthetic'][1]
    plus, minus = filled(cov_p, mod_p, gpu_device), filled(cov_m, mod_m, gpu_device)
    try:
        whole = model.sites(plus, minus, seq, want_features=True)
        assert whole['n_plus'] == want['n_plus'] and whole['features'].shape == (len(want['pos']), 14) and len(want['pos']) > 8000
        assert np.array_equal(whole['features'], want['features'].astype(np.float32))          # bit-equal to the float32 cast
        assert all(np.array_equal(whole[k], want[k]) for k in ('pos', 'cov', 'mod'))
        held = long_cases.scanned_indices(whole)
        assert {1023, 1024, 2047, 2048, 2 * tiles - 1} <= held          # sites on both sides of either pass boundary, '+' sites in tiles >= 1,024 among them
        assert (whole['pos'][:whole['n_plus']] // 1024 >= 1024).any() and any(i < 2047 for i in held if i >= tiles)
        cut = long_cases.SITE_CUT
        got = joined([model.sites(plus, minus, seq, f, c, want_features=True) for f, c in ((0, cut), (cut, count - cut))])
        assert got['n_plus'] == whole['n_plus'] and all(np.array_equal(got[k], whole[k]) for k in ('pos', 'cov', 'mod', 'new', 'features'))
    finally:
        plus.close()
        minus.close()


# ---- the command ----
def _chain_of_a_run(out: str, fasta: str, prefix: str, contigs, device: int):
    """Steps 2-4 of the documented workflow on the BED files of a detect run under `out`/run -> {file name: bytes} of hm_cluster_predict's output."""
    merge.sum_chr_mod(out, 'C', 'run', chrkeys=contigs, verbose=False)
    motif.generate_motif_pos(fasta, os.path.join(out, 'motif'), 'C', 'CG', 0, contigs)
    written = cluster.hm_cluster_predict(os.path.join(out, 'run'), os.path.join(out, 'motif'), prefix, contigs, device)
    return {os.path.basename(f): open(f, 'rb').read() for f in written}


@pytest.fixture(scope="module")
def command_case(gpu_device, tmp_path_factory):
    """Feature containers of two contigs (the generator of tests/test_gpu_e2e.py), their FASTA, a classifier checkpoint - and the reference result:
    `detect` without the flag, then the three tools."""
    tmp = tmp_path_factory.mktemp('cluster_cmd')
    wrk = tmp / 'reads'
    seqs = {}
    for k, (chrom, n) in enumerate((('chrM2', 110), ('chrQ', 50))):
        synth_reads.write_synthetic_run(str(wrk / chrom), n_reads=n, reads_per_file=5, genome_len=20000 - 7001 * k, seed=5 + k, chrom=chrom, min_len=300, max_len=1200)
        seqs[chrom] = synth_reads.synthetic_genome(20000 - 7001 * k, 5 + k)
    seqs['chrUnseen'] = 'ACGCGT' * 20                                # a contig of the reference without reads: no file from either side
    fasta = str(tmp / 'genome.fa')
    with open(fasta, 'w') as fh:
        for name, s in seqs.items():
            s = s[:100].lower() + s[100:]
            fh.write('>%s\n' % name + ''.join(s[i:i + 70] + '\n' for i in range(0, len(s), 70)))
    prefix = str(tmp / 'model' / 'm')
    os.makedirs(os.path.dirname(prefix))
    synth.write_synthetic_checkpoint(prefix, seed=26, scale=4.0)
    base = [sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'detect', '--wrkBase', str(wrk), '--modfile', prefix, '--FileID', 'run', '--threads', '4',
            '--Base', 'C', '--Ref', fasta]
    out = str(tmp / 'out_plain')
    res = subprocess.run(base + ['--outFolder', out], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert glob.glob(out + '/*clusterCpG*') == []                       # nothing of the stage without the flag
    beds = {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(out + '/run/*.bed'))}
    want = _chain_of_a_run(out, fasta, REAL, ['chrM2', 'chrQ'], gpu_device)
    assert sorted(want) == ['run_clusterCpG.chrM2.C.bed', 'run_clusterCpG.chrQ.C.bed'] and all(v.count(b'\n') >= 100 for v in want.values())
    assert len(beds) == 4
    return {'tmp': tmp, 'base': base, 'beds': beds, 'want': want, 'fasta': fasta, 'prefix': prefix, 'wrk': str(wrk)}


def _cluster_files(out):
    files = sorted(glob.glob(out + '/run_clusterCpG.*'))
    return {os.path.basename(f): open(f, 'rb').read() for f in files}


@pytest.mark.parametrize("world", [1, 2, 3])
def test_command_writes_the_files_of_the_three_tools(command_case, world):
    """`detect --clusterCpG CKPT` = detect, sum_chr_mod, generate_motif_pos, hm_cluster_predict: byte for byte, with the mod_pos.* files unchanged by
    the flag and no part file left; with 2 and 3 ranks every rank computes its slice with the edges of its neighbours."""
    from shim import build as shim_build
    out = str(command_case['tmp'] / ('out_%d' % world))
    env = dict(os.environ)
    more = []
    if world > 1:
        env.update(DEEPMOD_RCCL_LIBRARY=shim_build.library(), DEEPMOD_ONE_DEVICE='1')
        env.pop("DM_BENCH_FORCE_DIST", None)
        more = ['--gpus', str(world)]
    res = subprocess.run(command_case['base'] + ['--outFolder', out, '--clusterCpG', REAL] + more, capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert _cluster_files(out) == command_case['want']
    assert {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(out + '/run/*.bed'))} == command_case['beds']
    assert glob.glob(out + '/*.part*') == [] and glob.glob(out + '/run/*.part*') == []


def test_one_rank_through_the_scatter_merge(command_case, gpu_device):
    """StreamEngine.finalize's multi-rank form forced onto one rank (force_scatter_merge, as tests/test_gpu_summary.py runs it), with the checkpoint
    taken from the variable's place in the options: slices from dm_summary_reduce_scatter, part files, the join."""
    from deepmod_amd import comm, readmap, stream
    out = str(command_case['tmp'] / 'out_scatter')
    os.makedirs(out + '/run')
    prefix = command_case['prefix']
    mo = {'fnum': 7, 'hidden': 100, 'windowsize': 21, 'modfile': [prefix, os.path.dirname(prefix) + '/'], 'outFolder': out + '/run', 'Base': 'C',
          'force_scatter_merge': True, 'Ref': command_case['fasta'], 'clusterCpG': REAL}
    files = sorted(glob.glob(command_case['wrk'] + '/*/*'))
    backend = stream.HipBackend(mo, gpu_device)
    eng = stream.StreamEngine(mo, backend)
    eng.set_reference_lengths({c: len(s) for c, s in readmap.read_fasta(mo['Ref']).items()})
    eng.run(iter([files[:9], files[9:]]), feeders=1)
    c = comm.Communicator.from_rendezvous(gpu_device, comm.FileRendezvous(str(command_case['tmp'] / 'rdv'), 0, 1))
    eng.finalize(None, lambda s: s.reduce_scatter(c))
    c.close()
    backend.close()
    assert _cluster_files(out) == command_case['want']
    assert {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(out + '/run/*.bed'))} == command_case['beds']
    assert glob.glob(out + '/*.part*') == []
    assert eng.stats['cluster_sites'] == sum(v.count(b'\n') for v in command_case['want'].values())
