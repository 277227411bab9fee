#!/usr/bin/env python
"""`DeepMod.py getfeatures` on one synthetic input: the whole command (a fresh process, wall clock) and the per-stage times of one in-process run
(deepmod_amd.getfeatures keeps them in moptions['times']) -> a markdown table for profiles/getfeatures/README.md.  Recorded, not gated.

    python tools/getfeatures_rate.py [--input DIR | --reads N] [--threads T] [--posneg 0|1] [--move] [--out FILE]

--input DIR: raw containers + side-car .sam files + genome.fa written earlier (synth_reads.write_synthetic_raw_run); else they are generated first
(slow: the generator is a per-base Python loop) under a temporary folder.
"""
import argparse
import glob
import gzip
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--input')
    ap.add_argument('--reads', type=int, default=120)
    ap.add_argument('--threads', type=int, default=8)
    ap.add_argument('--posneg', type=int, default=1)
    ap.add_argument('--move', action='store_true')
    ap.add_argument('--out')
    a = ap.parse_args()
    from deepmod_amd import getfeatures, synth_reads
    work = tempfile.mkdtemp(prefix='gf_rate_')
    wrk = a.input
    if not wrk:
        wrk = os.path.join(work, 'wrk')
        synth_reads.write_synthetic_raw_run(wrk, n_reads=a.reads, reads_per_file=20, genome_len=200000, seed=3, chrom='chrS', min_len=3000, max_len=5000, move=a.move)
    fasta = os.path.join(wrk, 'genome.fa')
    n_files = len(glob.glob(os.path.join(wrk, '*.dmraw.npz')))
    raw_bytes = sum(os.path.getsize(f) for f in glob.glob(os.path.join(wrk, '*.dmraw.npz')))
    # the whole command, twice (the second run finds the files in the page cache)
    walls = []
    for k in range(2):
        cmd = [sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'getfeatures', '--wrkBase', wrk, '--Ref', fasta, '--outFolder', os.path.join(work, 'cmd%d' % k),
               '--posneg', str(a.posneg), '--threads', str(a.threads), '--files_per_thread', '1000'] + (['--move'] if a.move else [])
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, text=True)
        walls.append(time.perf_counter() - t0)
        if r.returncode != 0:
            sys.exit(r.stdout[-2000:] + r.stderr[-2000:])
    # one in-process run for the stage times
    mo = {'outLevel': 2, 'wrkBase': wrk, 'FileID': 'mod', 'outFolder': os.path.join(work, 'stages') + '/', 'recursive': 1, 'threads': a.threads, 'files_per_thread': 1000,
          'windowsize': 21, 'alignStr': 'minimap2', 'SignalGroup': 'simple', 'move': a.move, 'posneg': a.posneg, 'fnum': 7, 'size_per_batch': 1, 'Ref': fasta,
          'motifORPos': 1, 'motif': ['CG', 0], 'region': [None, None, None]}
    t0 = time.perf_counter()
    getfeatures.getFeature_manager(mo)
    wall_in = time.perf_counter() - t0
    times = mo['times']
    files = sorted(glob.glob(os.path.join(mo['outFolder'], '*', '*.xy.gz')))
    gz_bytes = sum(os.path.getsize(f) for f in files)
    text_bytes = rows = 0
    for f in files:
        data = gzip.open(f, 'rb').read()
        text_bytes += len(data)
        rows += data.count(b'\n')
    reads = sum(len(open(f[:-3] + '.ind').readlines()) for f in files)
    lines = ['| input | %d containers, %.1f MB, %d reads with rows, %s |' % (n_files, raw_bytes / 1e6, reads, 'move tables' if a.move else 'event tables'),
             '| output | %d rows, %.1f MB of text, %.1f MB gzip level %d, %d files |' % (rows, text_bytes / 1e6, gz_bytes / 1e6, getfeatures.GZIP_LEVEL, len(files)),
             '| whole command (fresh process) | %.2f s, second run %.2f s = %.0f rows/s |' % (walls[0], walls[1], rows / walls[1]),
             '| in process, --threads %d | %.2f s |' % (a.threads, wall_in)]
    for k in ('load', 'signal', 'align', 'walk', 'xy_keep', 'xy_text', 'download', 'gzip', 'write'):
        note = {'gzip': ' (summed over the host threads)', 'write': ' (summed over the host threads)', 'download': ' (uploads, host checks and copies of the dm_xy_rows call)',
                'xy_keep': ' (HIP events)', 'xy_text': ' (HIP events)'}.get(k, '')
        lines.append('| %s | %.4f s%s |' % (k, times.get(k, 0.0), note) if not k.startswith('xy_') else '| %s | %.3f ms%s |' % (k, 1e3 * times.get(k, 0.0), note))
    lines.append('| batches through the host formatter | %d |' % times.get('host_text_batches', 0))
    text = '| | |\n|---|---|\n' + '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write(text)


if __name__ == '__main__':
    main()
