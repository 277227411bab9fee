#!/usr/bin/env python
"""Lines per second of `merge` on a synthetic bacterial genome: one 4.6-Mb contig, three runs, both strands, the files as detect writes them (single
spaces, one before the newline; a line for about half of the C positions of a strand).

    python tools/merge_rate.py [--length 4600000] [--keep 0.5] [--repeat 3] [--out merge_rate.json]

Reported (medians of --repeat timed passes after one untimed pass):
  parse_* / add_* / format_*   the kernels alone (HIP events around them, dm_bedmerge_times): lines read per second of the first two, lines
                               written per second of the third
  command_*                    the whole command: files found and read from disk, uploaded, parsed, added, the merged file formatted, fetched
                               and written, the JSON (wall clock, same process, GPU already initialised)
  host_*                       merge.sum_chr_mod on the same files on the same machine in the same run (wall clock, one pass)
Wall-clock figures include the host; only the first three are device times.  The tool asserts that the command's file equals sum_chr_mod's byte
for byte."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmod_amd import merge  # noqa: E402

NAME = 'genome'


def bed_text(rng, seq, strand, keep, max_cov):
    """One detect file of one strand: the C positions of '+' / the G positions of '-', thinned to `keep`."""
    pos = np.nonzero(seq == (ord('C') if strand == '+' else ord('G')))[0]
    pos = pos[rng.random(len(pos)) < keep]
    cov = rng.integers(0, max_cov + 1, len(pos))
    mod = rng.binomial(cov, np.where(rng.random(len(pos)) < 0.4, 0.0, rng.random(len(pos))))
    pct = np.where(cov > 0, (100 * mod) // np.maximum(cov, 1), 0)
    return ''.join('%s %d %d C %d %s %d %d 0,0,0 %d %d %d \n' % (NAME, q, q + 1, min(c, 1000), strand, q, q + 1, c, pc, m)
                   for q, c, pc, m in zip(pos.tolist(), cov.tolist(), pct.tolist(), mod.tolist())).encode('ascii')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--length', type=int, default=4600000)
    ap.add_argument('--keep', type=float, default=0.5)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    rng = np.random.default_rng(5)
    seq = rng.choice(np.frombuffer(b'ACGT', np.uint8), args.length).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        texts = []
        for sub, max_cov in (('runA', 40), ('runB/sub', 20), ('runC/x/y', 12)):
            os.makedirs(os.path.join(tmp, sub))
            for strand in '+-':
                texts.append(bed_text(rng, seq, strand, args.keep, max_cov))
                with open(os.path.join(tmp, sub, 'mod_pos.%s%s.C.bed' % (NAME, strand)), 'wb') as fh:
                    fh.write(texts[-1])
        lines = sum(t.count(b'\n') for t in texts)
        nbytes = sum(len(t) for t in texts)
        mo = {'predFolder': tmp, 'Base': 'C', 'FileID': 'device', 'chr': [NAME], 'Ref': None, 'clusterCpG': None, 'threads': 4}
        quiet, stdout = open(os.devnull, 'w'), sys.stdout

        # the kernels alone: the texts are in memory, the table has the contig's length
        parse_ms, add_ms, format_ms, lines_out, bytes_out = [], [], [], 0, 0
        buf = np.empty(merge.FORMAT_BUFFER, np.uint8)
        for rep in range(args.repeat + 1):
            dev = merge.DeviceMerge()
            dev.open(NAME, args.length)
            for t in texts:
                _, flag, _ = dev.add_text(t)
                assert flag == 0
            lines_out, bytes_out, _ = dev.format_begin('C')
            more = bytes_out > 0
            while more:
                more, _ = dev.format_next(buf)
            p, a, f = dev.times()
            dev.close()
            if rep:
                parse_ms.append(p)
                add_ms.append(a)
                format_ms.append(f)
        # the whole command
        wall = []
        for rep in range(args.repeat + 1):
            sys.stdout = quiet
            try:
                t0 = time.perf_counter()
                doc = merge.merge_runs(mo)
                t = time.perf_counter() - t0
            finally:
                sys.stdout = stdout
            if rep:
                wall.append(t)
        assert doc['contigs'][NAME]['notes'] == [] and doc['contigs'][NAME]['lines_read'] == lines and doc['contigs'][NAME]['lines_written'] == lines_out
        # the host path on the same files
        t0 = time.perf_counter()
        host = merge.sum_chr_mod(tmp, 'C', 'host', chrkeys=[NAME], verbose=False)
        host_wall = time.perf_counter() - t0
        with open(host[NAME], 'rb') as a, open(doc['outputs'][NAME], 'rb') as b:
            want, got = a.read(), b.read()
        assert got == want and len(got) == bytes_out and got.count(b'\n') == lines_out, 'the command and merge.sum_chr_mod wrote different files'
    med = statistics.median
    out = {'contig_bases': args.length, 'files': len(texts), 'lines_read': lines, 'text_bytes_read': nbytes, 'lines_written': lines_out, 'text_bytes_written': bytes_out,
           'repeat': args.repeat, 'parse_ms': med(parse_ms), 'add_ms': med(add_ms), 'format_ms': med(format_ms), 'command_s': med(wall), 'host_s': host_wall,
           'parse_lines_per_s': lines / (med(parse_ms) * 1e-3), 'parse_bytes_per_s': nbytes / (med(parse_ms) * 1e-3), 'add_lines_per_s': lines / (med(add_ms) * 1e-3),
           'format_lines_per_s': lines_out / (med(format_ms) * 1e-3), 'format_bytes_per_s': bytes_out / (med(format_ms) * 1e-3),
           'command_lines_per_s': lines / med(wall), 'host_lines_per_s': lines / host_wall, 'all_parse_ms': parse_ms, 'all_add_ms': add_ms, 'all_format_ms': format_ms,
           'all_command_s': wall, 'files_equal': True}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
