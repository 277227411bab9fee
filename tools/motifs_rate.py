#!/usr/bin/env python
"""The sweep of `motifs` alone, and the whole command, on a synthetic contig.

    python tools/motifs_rate.py LENGTH [--repeat 5] [--command-positions 4000000] [--out motifs_rate.json]

One random contig of LENGTH bases; a sample and a control table pair with a record on every A and T (the keys of --Base A on either strand), filled
on the device.  Reported:
  sweep       per flank (3,3: the histogram in LDS; 4,4: in global memory), with controls: the kernel's time (HIP events, median and all of --repeat
              sweeps after one untimed sweep), positions per second, and GB/s on the algorithmic bytes of a position: 1 reference byte + 4 tables x
              (coverage, modified) x 4 bytes = 33 (the touch column of a table is not read); the share of the measured 6.3 TB/s HBM copy rate of an
              MI355X.  The device's counters are checked against motifs.HostEngine on the first 2,000,000 positions' worth of the same input.
  command     the whole command (files found, read, parsed, summed, swept, searched, written) on a contig of --command-positions bases (at most
              LENGTH) written as mod_pos BED files of one sample run and one control run: wall clock of the second of two runs, and its kernel times.
The input is generated in this process and is not part of any figure."""
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

HBM_COPY_TB_S = 6.3
BYTES_PER_POSITION = 33
CHUNK = 8 << 20


def make_input(length, seed=3):
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b'ACGT', np.uint8), length)
    recs = {}
    for role, covs in (('sample', (3, 6, 12, 30)), ('control', (4, 8, 20))):
        pos = np.nonzero((seq == ord('A')) | (seq == ord('T')))[0]
        strand = (seq[pos] == ord('T')).astype(np.uint8)
        cov = rng.choice(np.array(covs, np.int32), len(pos))
        frac = rng.choice(np.array([0.0, 0.1, 0.6, 1.0]), len(pos), p=(0.5, 0.2, 0.1, 0.2) if role == 'sample' else (0.8, 0.15, 0.05, 0.0))
        recs[role] = (pos.astype(np.int32), strand, cov, (cov * frac).astype(np.int32))
    return seq, recs


def fill(dm, recs, length):
    dm.open('chr1', length)
    pos, strand, cov, mod = recs
    for lo in range(0, len(pos), CHUNK):                              # bounded uploads
        dm.add_records(pos[lo:lo + CHUNK], strand[lo:lo + CHUNK], cov[lo:lo + CHUNK], mod[lo:lo + CHUNK])


def write_beds(folder, seq_len, recs):
    os.makedirs(folder, exist_ok=True)
    pos, strand, cov, mod = (a[:int(np.searchsorted(recs[0], seq_len))] for a in recs)
    for s, sign in enumerate('+-'):
        sel = strand == s
        with open(os.path.join(folder, 'mod_pos.chr1%s.A.bed' % sign), 'w') as fh:
            fh.write(''.join('chr1 %d %d A %d %s %d %d 0,0,0 %d %d %d \n' % (p, p + 1, c, sign, p, p + 1, c, 100 * m // c, m)
                             for p, c, m in zip(pos[sel].tolist(), cov[sel].tolist(), mod[sel].tolist())))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('length', type=int)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--command-positions', type=int, default=4000000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from deepmod_amd import merge, motifs

    def say(what):
        print('[motifs_rate] %s' % what, file=sys.stderr, flush=True)

    length = args.length
    seq, recs = make_input(length)
    say('%d positions, %d sample and %d control records' % (length, len(recs['sample'][0]), len(recs['control'][0])))
    out = {'positions': length, 'bytes_per_position': BYTES_PER_POSITION, 'repeat': args.repeat, 'sweep': {}}
    sample, control = merge.DeviceMerge(0), merge.DeviceMerge(0)
    fill(sample, recs['sample'], length)
    fill(control, recs['control'], length)
    head = min(length, 2000000)
    for up, down in ((3, 3), (4, 4)):
        dev = motifs.DeviceEngine(up, down, 'A')
        ms = []
        for rep in range(args.repeat + 1):
            before = dev.times()[1]
            counters, off_base = dev.count(seq, sample.plus, sample.minus, control.plus, control.minus)
            if rep:
                ms.append(dev.times()[1] - before)
        hist = dev.fetch()
        assert hist[:, 0].sum() == (args.repeat + 1) * counters[:, 0].sum() and hist[:, 1].sum() == (args.repeat + 1) * counters[:, 1].sum()
        dev.close()
        t = statistics.median(ms) * 1e-3
        out['sweep']['%d,%d' % (up, down)] = {'histogram': 'LDS' if up + down <= 6 else 'global', 'kernel_ms': statistics.median(ms), 'all_kernel_ms': ms,
                                              'positions_per_s': length / t, 'GB_per_s': length * BYTES_PER_POSITION / t / 1e9,
                                              'share_of_hbm_copy_rate': length * BYTES_PER_POSITION / t / (HBM_COPY_TB_S * 1e12),
                                              'counters': {s: dict(zip(motifs.COUNT_KEYS, counters[i].tolist())) for i, s in enumerate('+-')}}
        say('flank %d,%d: %.3f ms, %.1f GB/s' % (up, down, statistics.median(ms), out['sweep']['%d,%d' % (up, down)]['GB_per_s']))
        # the same rule on the host, on the head of the input
        small_dev, host = motifs.DeviceEngine(up, down, 'A'), motifs.HostEngine(up, down, 'A')
        hs, hc = merge.DeviceMerge(0), merge.DeviceMerge(0)
        tabs = []
        for dm, role in ((hs, 'sample'), (hc, 'control')):
            cut = int(np.searchsorted(recs[role][0], head))
            fill(dm, tuple(a[:cut] for a in recs[role]), head)
            t_host = [(np.zeros(head, np.int64), np.zeros(head, np.int64)) for _ in range(2)]
            for s in range(2):
                sel = recs[role][1][:cut] == s
                t_host[s][0][recs[role][0][:cut][sel]] = recs[role][2][:cut][sel]
                t_host[s][1][recs[role][0][:cut][sel]] = recs[role][3][:cut][sel]
            tabs += t_host
        got, want = small_dev.count(seq[:head], hs.plus, hs.minus, hc.plus, hc.minus), host.count(seq[:head], *tabs)
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and np.array_equal(small_dev.fetch(), host.fetch()), 'device and host disagree'
        for h in (small_dev, hs, hc):
            h.close()
    sample.close(), control.close()
    out['equal_to_host_on_positions'] = head
    n_cmd = min(length, args.command_positions)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, 'genome.fa'), 'wb') as fh:
            fh.write(b'>chr1\n' + seq[:n_cmd].tobytes() + b'\n')
        write_beds(os.path.join(tmp, 'sample', 'run1'), n_cmd, recs['sample'])
        write_beds(os.path.join(tmp, 'control', 'run1'), n_cmd, recs['control'])
        mo = {'predFolder': os.path.join(tmp, 'sample'), 'control': [os.path.join(tmp, 'control')], 'Ref': os.path.join(tmp, 'genome.fa'), 'Base': 'A',
              'outFolder': os.path.join(tmp, 'out'), 'FileID': 'rate', 'threads': 4}
        quiet, stdout = open(os.devnull, 'w'), sys.stdout
        for rep in range(2):
            sys.stdout = quiet
            try:
                t0 = time.perf_counter()
                doc = motifs.motifs(mo)
                wall = time.perf_counter() - t0
            finally:
                sys.stdout = stdout
            say('pass %d of the command: %.2f s' % (rep, wall))
        out['command'] = {'positions': n_cmd, 'lines_read': doc['contigs']['chr1']['lines_read'] + doc['contigs']['chr1']['control_lines_read'], 'wall_s': wall,
                          'times': doc['times'], 'motifs': [m['motif'] for m in doc['motifs']], 'notes': doc['notes']}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
