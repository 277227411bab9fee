#!/usr/bin/env python
"""Lines per second of `siteperf` on a synthetic bacterial genome: one 4.6-Mb contig, one run and two control runs (one BED file each, a line for
about half of the C positions of both strands).

    python tools/siteperf_rate.py [--length 4600000] [--keep 0.5] [--repeat 3] [--out siteperf_rate.json]

Reported (medians of --repeat timed passes after one untimed pass):
  parse_lines_per_s    the parse kernels alone (HIP events around them, dm_siteperf_times)
  count_lines_per_s    the classify-and-count, scatter and table-walk kernels alone (HIP events)
  command_lines_per_s  the whole command: files read from disk, uploaded, parsed and counted, measures and both output files written (wall clock)
  twin_*               the numpy twin (siteperf.HostEngine) on the same machine: its counting alone, fed parsed arrays, and the whole command
                       through the host parser
Wall-clock figures include the host; only the first two are device times."""
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
from deepmod_amd import siteperf as sp  # noqa: E402


def bed_text(rng, name, seq, keep, methylated, max_cov):
    """One file: the C positions of '+' and the G positions of '-' (as C), thinned to `keep`; vectorised."""
    parts = []
    site = sp.site_codes(seq, 'Cg', 0)
    for strand, letter, bit in ((b'+', ord('C'), 1), (b'-', ord('G'), 2)):
        pos = np.nonzero(seq == letter)[0]
        pos = pos[rng.random(len(pos)) < keep]
        cov = rng.integers(0, max_cov + 1, len(pos))
        p = np.where(((site[pos] & bit) != 0) & methylated, 0.55 + 0.45 * rng.random(len(pos)), 0.25 * rng.random(len(pos)) ** 2)
        mod = rng.binomial(cov, p)
        pct = np.where(cov > 0, (100 * mod) // np.maximum(cov, 1), 0)
        s = strand.decode()
        parts.extend('%s\t%d\t%d\tC\t%d\t%s\t%d\t%d\t0,0,0\t%d\t%d\t%d\n' % (name, q, q + 1, min(c, 1000), s, q, q + 1, c, pc, m)
                     for q, c, pc, m in zip(pos.tolist(), cov.tolist(), pct.tolist(), mod.tolist()))
    return ''.join(parts).encode('ascii')


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
        texts = {}
        for folder, methylated, max_cov in (('run', True, 40), ('control1', False, 20), ('control2', False, 12)):
            os.makedirs(os.path.join(tmp, folder))
            texts[folder] = bed_text(rng, 'genome', seq, args.keep, methylated, max_cov)
            with open(os.path.join(tmp, folder, 'mod_pos.%s.C.bed' % folder), 'wb') as fh:
                fh.write(texts[folder])
        with open(os.path.join(tmp, 'genome.fa'), 'wb') as fh:
            fh.write(b'>genome synthetic\n')
            for i in range(0, args.length, 70):
                fh.write(seq[i:i + 70].tobytes() + b'\n')
        lines = sum(t.count(b'\n') for t in texts.values())
        nbytes = sum(len(t) for t in texts.values())
        mo = {'predFolder': os.path.join(tmp, 'run'), 'control': [os.path.join(tmp, 'control1'), os.path.join(tmp, 'control2')], 'Ref': os.path.join(tmp, 'genome.fa'),
              'motif': 'Cg', 'ModinMotif': 0, 'chr': None, 'start': None, 'end': None, 'cov': (1, 5), 'outFolder': os.path.join(tmp, 'out'), 'FileID': 'rate', 'threads': 4}
        quiet = open(os.devnull, 'w')
        stdout = sys.stdout

        def command(engine=None):
            sys.stdout = quiet
            try:
                t0 = time.perf_counter()
                doc = sp.siteperf(mo, engine=engine)
                return time.perf_counter() - t0, doc
            finally:
                sys.stdout = stdout

        # the device: kernels alone, then the whole command
        parse_ms, count_ms = [], []
        for rep in range(args.repeat + 1):
            dev = sp.DeviceEngine((1, 5))
            dev.set_contig(seq, 'Cg', 0)
            for folder, role in (('control1', sp.CONTROL), ('control2', sp.CONTROL), ('run', sp.RUN)):
                _, flag, _ = dev.add_text(texts[folder], role, 'genome')
                assert flag == 0
            dev.finish_contig()
            p, c = dev.times()
            dev.close()
            if rep:
                parse_ms.append(p)
                count_ms.append(c)
        wall, doc = [], None
        for rep in range(args.repeat + 1):
            t, doc = command()
            if rep:
                wall.append(t)
        # the numpy twin on the same machine
        recs = {f: sp.parse_device_grammar(t, 'genome', args.length)[0] for f, t in texts.items()}
        t0 = time.perf_counter()
        host = sp.HostEngine((1, 5))
        host.set_contig(seq, 'Cg', 0)
        for folder, role in (('control1', sp.CONTROL), ('control2', sp.CONTROL), ('run', sp.RUN)):
            host.add_records(role, *recs[folder])
        host.finish_contig()
        twin_count = time.perf_counter() - t0
        twin_wall, twin_doc = command(sp.HostEngine((1, 5)))
        assert twin_doc['histogram']['counts'] == doc['histogram']['counts'] and twin_doc['lines'] == doc['lines']
        assert np.array_equal(host.fetch()['hist'], np.array(doc['histogram']['counts']))
    med = statistics.median
    out = {'contig_bases': args.length, 'files': 3, 'lines': lines, 'text_bytes': nbytes, 'repeat': args.repeat,
           'parse_ms': med(parse_ms), 'count_ms': med(count_ms), 'command_s': med(wall), 'twin_count_s': twin_count, 'twin_command_s': twin_wall,
           'parse_lines_per_s': lines / (med(parse_ms) * 1e-3), 'parse_bytes_per_s': nbytes / (med(parse_ms) * 1e-3), 'count_lines_per_s': lines / (med(count_ms) * 1e-3),
           'command_lines_per_s': lines / med(wall), 'twin_count_lines_per_s': lines / twin_count, 'twin_command_lines_per_s': lines / twin_wall,
           'all_parse_ms': parse_ms, 'all_count_ms': count_ms, 'all_command_s': wall, 'auc_all_cov1': doc['measures']['all_mp']['1']['auc']}
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
