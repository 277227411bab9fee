"""CPU: the CpG-cluster stage from the counters (detect --clusterCpG).  cluster.sites_from_counters - the numpy twin of csrc/cluster_sites.hip.inc and the
statement of its semantics - against the chain of the three tools on files (tests/cluster_fused_case.py) and against the loop-level oracle pinned to the
reference run; the twin on rank slices with halos; the refusals of the command line; the host formatter under AddressSanitizer as a program."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cluster_fused_case as cf
from conftest import ROOT
from deepmod_amd import cluster
from oracle import cluster_oracle

CASES = [(n, tail) for n in cf.LENGTHS[:-1] for tail in ('CG', 'C')] + [(70001, 'CG')]


@pytest.mark.parametrize("length,tail", CASES)
def test_twin_equals_the_chain_on_files(length, tail):
    """Features equal after the fp32 cast (the feed of the MLP), site order and line text equal; the loop-level oracle agrees with both."""
    ch = cf.chain(length, tail)
    if length == 70001:
        cf.assert_run_is_no_empty_comparison(ch)
    got = cluster.sites_from_counters(*ch['case'])
    assert got['features'].shape == ch['x'].shape and got['n_plus'] == ch['n_plus']
    assert np.array_equal(got['features'].astype(np.float32), ch['x'].astype(np.float32))
    assert cluster.site_lines_py(cf.CHROM, 'C', got) == ch['lines']
    pos, cov, mod = cf.records_of(ch['lines'])
    assert np.array_equal(got['pos'], pos) and np.array_equal(got['cov'], cov) and np.array_equal(got['mod'], mod)
    if len(ch['lines']):
        x, lines = cluster_oracle.features_loop(ch['motif_text'], ch['pred_text'], cf.CHROM)
        assert lines == ch['lines']
        assert np.array_equal(got['features'].astype(np.float32), x.astype(np.float32))


def test_twin_with_one_strand_absent():
    ch = cf.chain(257, 'CG', True)
    seq, cov_p, mod_p, _, _ = ch['case']
    got = cluster.sites_from_counters(seq, cov_p, mod_p, None, None)
    assert got['n_plus'] == len(got['pos']) == len(ch['lines']) > 20 and (ch['x'][:, 1] == 0).all()
    assert np.array_equal(got['features'].astype(np.float32), ch['x'].astype(np.float32))
    assert cluster.site_lines_py(cf.CHROM, 'C', got) == ch['lines']


def sliced_twin(case, slices):
    """The twin per rank slice - each with the halo assembled from the edges all ranks publish and its slice +-27 of the sequence - joined as rank 0
    joins the part files: all '+' parts in rank order, then all '-' parts."""
    seq, cov_p, mod_p, cov_m, mod_m = case
    everyone = [{"first": f, "count": c, "edges": cluster.slice_edges(*[a[f:f + c] for a in (cov_p, mod_p, cov_m, mod_m)])} for f, c in slices]
    parts = []
    for f, c in slices:
        lo, hi = max(0, f - 27), min(len(seq), f + c + 27)
        parts.append(cluster.sites_from_counters(seq[lo:max(lo, hi)], *[a[f:f + c] for a in (cov_p, mod_p, cov_m, mod_m)], first=f,
                                                 halo=cluster.halo_from_edges(f, c, everyone), seq_first=lo))
    out = {k: np.concatenate([p[k][:p['n_plus']] for p in parts] + [p[k][p['n_plus']:] for p in parts]) for k in ('pos', 'cov', 'mod', 'features')}
    out['n_plus'] = sum(p['n_plus'] for p in parts)
    return out


def assert_same_sites(got, want):
    assert got['n_plus'] == want['n_plus']
    for k in ('pos', 'cov', 'mod', 'features'):
        assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("world", [2, 3, 8])
def test_twin_on_rank_slices_with_halos_equals_the_whole_contig(world):
    ch = cf.chain(70001)
    whole = cluster.sites_from_counters(*ch['case'])
    assert_same_sites(sliced_twin(ch['case'], cf.slices_of(70001, world)), whole)


def test_cuts_between_the_c_and_the_g_of_a_pair_and_inside_a_dense_run():
    ch = cf.chain(70001)
    seq, cov_p, mod_p, cov_m, mod_m = ch['case']
    whole = cluster.sites_from_counters(*ch['case'])
    plus, minus = set(whole['pos'][:whole['n_plus']].tolist()), set(whole['pos'][whole['n_plus']:].tolist())
    pair = next(p for p in sorted(plus) if p > 30000 and p + 1 in minus)          # '+' site at pair, its partner at pair + 1: cut between them
    cuts = [0, 120, pair + 1, 70001]                                              # 120: inside the modified CGCG run of positions 60 .. 189
    assert seq[118:122].upper() == 'CGCG' and 119 in minus and 120 in plus
    slices = list(zip(cuts[:-1], np.diff(cuts).tolist()))
    assert_same_sites(sliced_twin(ch['case'], slices), whole)
    # without the halos the slices lose neighbours and partners at their edges: the comparison above is not empty
    for f, c in slices[1:]:
        bare = cluster.sites_from_counters(seq, *[a[f:f + c] for a in (cov_p, mod_p, cov_m, mod_m)], first=f)
        keep = (whole['pos'] >= f) & (whole['pos'] < f + c)
        assert np.array_equal(bare['pos'], whole['pos'][keep]) and not np.array_equal(bare['features'], whole['features'][keep])
    # slices shorter than the halo: a rank's 26 positions come from several neighbours, and some ranks own nothing
    small = cf.chain(52)
    for world in (2, 3, 8, 64):
        assert_same_sites(sliced_twin(small['case'], cf.slices_of(52, world)), cluster.sites_from_counters(*small['case']))


def _detect(args, env=None):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'detect'] + args, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, **(env or {})))


def test_command_line_refusals(tmp_path):
    """One clear line each, before any device is opened."""
    fasta = tmp_path / 'genome.fa'
    fasta.write_text('>chrT\nACGT\n')
    ckpt = str(tmp_path / 'Cg')
    (tmp_path / 'Cg.index').write_text('')
    common = ['--wrkBase', str(tmp_path), '--outFolder', str(tmp_path / 'out')]
    env = {'DEEPMOD_CLUSTER_MODEL': ''}
    for args, words in (
            (['--Base', 'A', '--Ref', str(fasta), '--clusterCpG', ckpt], ['--Base C only']),
            (['--Base', 'C', '--clusterCpG', ckpt], ['needs --Ref']),
            (['--Base', 'C', '--Ref', str(tmp_path / 'missing.fa'), '--clusterCpG', ckpt], ['needs --Ref']),
            (['--Base', 'C', '--Ref', str(fasta), '--clusterCpG'], ['no cluster-model checkpoint', 'DEEPMOD_CLUSTER_MODEL']),
            (['--Base', 'C', '--Ref', str(fasta), '--clusterCpG', str(tmp_path / 'nothing')], ['no cluster-model checkpoint at']),
            (['--Base', 'C', '--Ref', str(fasta), '--clusterCpG', ckpt, '--storePred', '1'], ['sum_chr_mod.py', 'generate_motif_pos.py', 'hm_cluster_predict.py']),
            (['--Base', 'C', '--Ref', str(fasta), '--clusterCpG', ckpt, '--predDet', '0'], ['sum_chr_mod.py', 'generate_motif_pos.py', 'hm_cluster_predict.py'])):
        res = _detect(common + args, env)
        assert res.returncode != 0 and 'Traceback' not in res.stderr, res.stderr[-2000:]
        last = res.stderr.strip().splitlines()[-1]
        assert last.startswith('Error: --clusterCpG: ') and all(w in last for w in words), res.stderr[-2000:]
    # the variable names the checkpoint when the flag has no value; a missing file behind it is refused the same way
    res = _detect(common + ['--Base', 'C', '--Ref', str(fasta), '--clusterCpG'], {'DEEPMOD_CLUSTER_MODEL': str(tmp_path / 'nothing')})
    assert res.returncode != 0 and 'no cluster-model checkpoint at' in res.stderr.strip().splitlines()[-1]
    from deepmod_amd import detect
    mo = {'Base': 'C', 'Ref': str(fasta), 'storePred': 0, 'predDet': 1}
    assert detect.cluster_cpg_prefix(ckpt, mo) == ckpt
    os.environ['DEEPMOD_CLUSTER_MODEL'], before = ckpt, os.environ.get('DEEPMOD_CLUSTER_MODEL')
    try:
        assert detect.cluster_cpg_prefix('', mo) == ckpt
    finally:
        if before is None:
            del os.environ['DEEPMOD_CLUSTER_MODEL']
        else:
            os.environ['DEEPMOD_CLUSTER_MODEL'] = before
    assert not os.path.exists(str(tmp_path / 'out'))


def test_host_formatter_under_address_sanitizer(tmp_path):
    """tests/cluster_asan_driver.cpp: dm_cluster_bed_format as tests/asan/host_shim.cpp restates the host part of the ABI (included, not changed), built as
    a PROGRAM with -fsanitize=address,undefined and the sanitizer runtime linked in statically - columns and text in heap blocks of exactly their
    size; zero sites, one site, cov > 1000, the longest accepted values, refused records."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'cluster_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'cluster_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'CLUSTER-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]


def test_formatter_equals_the_tools_lines(hip_lib):
    """dm_cluster_bed_format through the product library: the chain's lines + ' <new>'."""
    ch = cf.chain(257)
    got = cluster.sites_from_counters(*ch['case'])
    got['new'] = (np.arange(len(got['pos'])) * 7) % 101
    want = ''.join('%s %d\n' % (ln, v) for ln, v in zip(ch['lines'], got['new'].tolist()))
    assert b''.join(cluster.site_text_parts(cf.CHROM, 'C', got)).decode() == want and len(want) > 1000
