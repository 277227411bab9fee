"""GPU (-m gpu): the sweep of `motifs` on the device (csrc/motifs.hip.inc) against motifs.HostEngine: histogram, counters and off_base equal exactly,
at the wave, workgroup and tile edges, at both contig ends, on both sides of the LDS / global switch of the histogram, at every edge of the rules and
with every key of a strand in one bin; accumulation and reset; the refusals of the C ABI; and the command on the device against the command under
HostEngine on the synthetic case of tests/motifs_synth.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import _lib, merge, motifs, summary

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import long_cases  # noqa: E402
import motifs_synth  # noqa: E402

pytestmark = pytest.mark.gpu

COV, T_PCT, U_PCT = 5, 50, 10
BIG = 2 ** 31 - 1
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
FLANKS = [(0, 0), (1, 0), (0, 1), (3, 3), (2, 3), (3, 4), (4, 4), (8, 0), (0, 8)]
# (coverage, modified, control coverage, control modified) on consecutive sites of a strand: sample coverage c - 1 and c; 100 mod == t cov exactly and
# one modified read fewer; the control percentage exactly u, the smallest step above it, and both sides of u where only the integer division decides;
# control coverage c - 1; coverage = modified = 2^31 - 1 in sample and control, and the two sides of t at that coverage
RULE_EDGES = [(COV - 1, COV - 1, 30, 0), (COV, COV, 30, 0), (6, 3, 30, 0), (6, 2, 30, 0), (30, 30, 100, 10), (30, 30, 100, 11), (30, 30, 28, 3), (30, 30, 27, 3),
              (30, 30, COV - 1, 0), (30, 30, COV, 0), (BIG, BIG, BIG, BIG), (BIG, BIG, BIG, 0), (BIG, BIG // 2, 30, 0), (BIG, BIG // 2 + 1, 30, 0), (0, 0, 30, 0), (30, 0, 0, 0)]


def tile():
    return motifs.tile_positions()


def lengths_of(up, down):
    t = tile()
    # (a table has at least one position - dm_summary_create refuses 0 - so the contig of U + D = 0 bases exists only for the host twin: the sanitizer driver)
    return sorted({n for n in (1, up + down, up + down + 1, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 3 * t + 7) if n >= 1})


def make_sequence(rng, length, up, down, base, variant):
    """Random letters with a site of one strand (variant 0: '+', 1: '-') on the last and the first position of every tile and beside them a site of the
    other strand, and sites whose flank ends exactly at position 0 and at length - 1 and one short of them, on both strands."""
    seq = np.array(list(rng.choice(list('ACGT'), length)))
    own, other = (base, COMP[base]) if variant == 0 else (COMP[base], base)

    def put(p, letter):
        if 0 <= p < length:
            seq[p] = letter

    t = tile()
    for edge in range(t, length + 1, t):
        put(edge - 2, other), put(edge + 1, other), put(edge - 1, own), put(edge, own)
    plus = [up, up - 1, length - 1 - down, length - down]             # '+': upstream towards position 0
    minus = [down, down - 1, length - 1 - up, length - up]            # '-': downstream towards position 0
    order = [(plus, base), (minus, COMP[base])]
    for positions, letter in (order if variant == 0 else order[::-1]):                               # where both want a position, the later one has it
        for p in positions:
            put(p, letter)
    return ''.join(seq)


def records_for(rng, seq, base, phase):
    """Sample and control records: RULE_EDGES in turn on the sites of either strand, lines on letters that are not the base now and then."""
    n = len(seq)
    recs = {'sample': [], 'control': []}
    for s, letter in enumerate((base, COMP[base])):
        k = phase
        for p in range(n):
            if seq[p] == letter:
                cv, md, ccv, cmd = RULE_EDGES[k % len(RULE_EDGES)]
                k += 1
                if cv:
                    recs['sample'].append((p, s, cv, md))
                if ccv:
                    recs['control'].append((p, s, ccv, cmd))
            elif rng.random() < 0.1:
                recs['sample'].append((p, s, 7, 3))                   # off_base
                recs['control'].append((p, s, 9, 0))
    return {k: tuple(np.array([r[j] for r in v], np.int64) for j in range(4)) for k, v in recs.items()}


def host_tables(rec, n):
    tabs = [(np.zeros(n, np.int64), np.zeros(n, np.int64)) for _ in range(2)]
    pos, strand, cov, mod = rec
    for s in range(2):
        sel = strand == s
        tabs[s][0][pos[sel]] = cov[sel]
        tabs[s][1][pos[sel]] = mod[sel]
    return tabs


class Tables:
    """The device tables of the sample and of the controls, filled through merge.DeviceMerge as the command fills them."""

    def __init__(self):
        self.dm = {'sample': merge.DeviceMerge(0), 'control': merge.DeviceMerge(0)}

    def fill(self, recs, n):
        out = []
        for role in ('sample', 'control'):
            self.dm[role].open('c', n)
            if len(recs[role][0]):
                self.dm[role].add_records(*recs[role])
            out += [self.dm[role].plus, self.dm[role].minus]
        return out

    def close(self):
        for dm in self.dm.values():
            dm.close()


def both(dev, host, seq, recs, tables, with_control, what):
    n = len(seq)
    d = tables.fill(recs, n)
    h = host_tables(recs['sample'], n) + host_tables(recs['control'], n)
    keep = 4 if with_control else 2
    got, want = dev.count(seq.encode(), *d[:keep]), host.count(seq.encode(), *h[:keep])
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist(), (what, got, want)
    gh, wh = dev.fetch(), host.fetch()
    assert np.array_equal(gh, wh), (what, np.nonzero((gh != wh).any(axis=1))[0][:8])
    return want


@pytest.mark.parametrize('up,down', FLANKS)
def test_sweep_equals_host_engine(hip_lib, up, down):
    rng = np.random.default_rng(1000 * up + down)
    engines = {b: (motifs.DeviceEngine(up, down, b, COV, T_PCT, U_PCT), motifs.HostEngine(up, down, b, COV, T_PCT, U_PCT)) for b in 'ACGT'}
    tables = Tables()
    seen = np.zeros(5, np.int64)
    try:
        for i, n in enumerate(lengths_of(up, down)):
            for variant in range(2):
                base = 'ACGT'[(i + 2 * variant + up) % 4]              # each of the four bases, on every flank
                dev, host = engines[base]
                seq = make_sequence(rng, n, up, down, base, variant)
                recs = records_for(rng, seq, base, i + variant)
                for with_control in (True, False):
                    counters, off_base = both(dev, host, seq, recs, tables, with_control, (up, down, n, variant, base, with_control))
                    seen += counters.sum(axis=0)
        # N and a lower-case letter at each offset of a context, the site itself included, on both strands
        for base in 'AC':
            dev, host = engines[base]
            blocks = []
            for letter, sign in ((base, 1), (COMP[base], -1)):
                for j in range(-up, down + 1):
                    for bad in 'Na':
                        block = list(rng.choice(list('ACGT'), 2 * (up + down) + 3))
                        mid = up + down + 1
                        block[mid] = letter
                        block[mid + sign * j] = bad
                        blocks.append(''.join(block))
            seq = 'ACGT' * 3 + ''.join(blocks) + 'ACGT' * 3
            recs = records_for(rng, seq, base, 1)
            for with_control in (True, False):
                counters, _ = both(dev, host, seq, recs, tables, with_control, (up, down, 'mutants', base, with_control))
                assert up + down == 0 or (counters[:, 4] > 0).all()                                     # edge, on both strands
        assert (seen[:4] > 0).all() and (seen[4] > 0 or up + down == 0)                                 # every counter was exercised on this flank
    finally:
        tables.close()
        for dev, _ in engines.values():
            dev.close()


@pytest.mark.parametrize('up,down', [(3, 3), (4, 4)])
def test_every_key_of_a_strand_in_one_bin(hip_lib, up, down):
    """A contig of one repeated letter, 3 T + 7 long: every tested key of a strand falls into one bin, in LDS (3,3) and in global memory (4,4)."""
    n = 3 * tile() + 7
    tables = Tables()
    try:
        for letter, base, strand in (('A', 'A', 0), ('A', 'T', 1), ('G', 'G', 0)):
            dev, host = motifs.DeviceEngine(up, down, base, COV, T_PCT, U_PCT), motifs.HostEngine(up, down, base, COV, T_PCT, U_PCT)
            pos = np.arange(n, dtype=np.int64)
            strand_of = np.full(n, strand, np.int64)
            mod = np.where(pos % 3 == 0, 30, 0)
            recs = {'sample': (pos, strand_of, np.full(n, 30, np.int64), mod), 'control': (pos, strand_of, np.full(n, 30, np.int64), np.zeros(n, np.int64))}
            counters, _ = both(dev, host, letter * n, recs, tables, True, (up, down, letter, base))
            hist = dev.fetch()
            assert counters[strand, 0] == n - up - down and (hist[:, 0] > 0).sum() == 1 and hist[:, 0].sum() == n - up - down
            assert hist[:, 1].sum() == counters[strand, 1] > 0
            dev.close()
    finally:
        tables.close()


@pytest.mark.parametrize('up,down', [(3, 3), (4, 4)])
def test_sweep_wraps_the_grid(hip_lib, up, down):
    """2,050 tiles (long_cases.motifs_case): mo_count_kernel's workgroup 0 takes tiles 0 and 2,048, workgroup 1 tile 1 and the ragged 2,049 - the LDS
    code buffer restaged per tile, the LDS histogram of (3, 3) kept across a workgroup's tiles and flushed once, the merged runs of (4, 4) - with and
    without controls; one planted context puts tested keys of tile 0 and of tile 2,048 into one bin."""
    t = tile()
    seq, recs, planted = long_cases.motifs_case(t, tuple(RULE_EDGES))
    n = len(seq)
    assert (n + t - 1) // t > 2048                                    # mok::MAX_BLOCKS: the grid wraps
    bins = [long_cases.motif_bin_of(seq, recs, p, up, down, (COV, T_PCT, U_PCT)) for p in planted['shared']]
    assert bins[0] == bins[1] >= 0 and [p // t for p in planted['shared']] == [0, 2048]
    dev, host = motifs.DeviceEngine(up, down, long_cases.MOTIF_BASE, COV, T_PCT, U_PCT), motifs.HostEngine(up, down, long_cases.MOTIF_BASE, COV, T_PCT, U_PCT)
    tables = Tables()
    try:
        for with_control in (True, False):
            counters, off_base = both(dev, host, seq.decode(), recs, tables, with_control, (up, down, 'long', with_control))
            assert (counters[:, [0, 1, 2, 4]] > 0).all() and (off_base > 0).all() and (counters[:, 3] > 0).all() == with_control     # every counter, on both strands
            assert host.fetch()[bins[0], 0] >= 2
    finally:
        tables.close()
        dev.close()


def test_every_key_of_a_strand_in_one_bin_across_the_wrap(hip_lib):
    """The one-letter contig of test_every_key_of_a_strand_in_one_bin on 2,050 tiles, flank (4, 4): every lane of every tile of a workgroup adds to
    one bin of the global histogram, and the run merge meets the wrap."""
    up = down = 4
    n = long_cases.wrap_length(tile())
    assert (n + tile() - 1) // tile() > 2048                          # mok::MAX_BLOCKS
    tables = Tables()
    try:
        for letter, base, strand in (('A', 'A', 0), ('A', 'T', 1)):
            dev, host = motifs.DeviceEngine(up, down, base, COV, T_PCT, U_PCT), motifs.HostEngine(up, down, base, COV, T_PCT, U_PCT)
            pos = np.arange(n, dtype=np.int64)
            strand_of = np.full(n, strand, np.int64)
            mod = np.where(pos % 3 == 0, 30, 0)
            recs = {'sample': (pos, strand_of, np.full(n, 30, np.int64), mod), 'control': (pos, strand_of, np.full(n, 30, np.int64), np.zeros(n, np.int64))}
            counters, _ = both(dev, host, letter * n, recs, tables, True, (up, down, letter, base))
            hist = dev.fetch()
            assert counters[strand, 0] == n - up - down and (hist[:, 0] > 0).sum() == 1 and hist[:, 0].sum() == n - up - down
            assert hist[:, 1].sum() == counters[strand, 1] > 0
            dev.close()
    finally:
        tables.close()


def test_accumulation_and_reset(hip_lib):
    rng = np.random.default_rng(5)
    dev, host = motifs.DeviceEngine(2, 3, 'C', COV, T_PCT, U_PCT), motifs.HostEngine(2, 3, 'C', COV, T_PCT, U_PCT)
    tables = Tables()
    try:
        total = np.zeros((2, 5), np.int64)
        for n in (700, tile() + 300):
            seq = make_sequence(rng, n, 2, 3, 'C', 0)
            total += both(dev, host, seq, records_for(rng, seq, 'C', 0), tables, True, n)[0]
        assert dev.counters.tolist() == total.tolist() == host.counters.tolist() and dev.fetch()[:, 0].sum() == total[:, 0].sum() > 0
        dev.reset(), host.reset()
        assert not dev.fetch().any() and not dev.counters.any() and not dev.off_base.any()
        seq = make_sequence(rng, 300, 2, 3, 'C', 1)
        both(dev, host, seq, records_for(rng, seq, 'C', 2), tables, False, 'after reset')
        assert all(v >= 0 for v in dev.times())
    finally:
        tables.close()
        dev.close()


def test_abi_refusals(hip_lib):
    lib = hip_lib
    for args, words in (((5, 4, b'A', 5, 50, 10), b'flank'), ((9, 0, b'A', 5, 50, 10), b'flank'), ((-1, 0, b'A', 5, 50, 10), b'flank'), ((3, 3, b'N', 5, 50, 10), b'base'),
                        ((3, 3, b'a', 5, 50, 10), b'base'), ((3, 3, b'A', 0, 50, 10), b'coverage'), ((3, 3, b'A', 5, 101, 10), b'percentage'),
                        ((3, 3, b'A', 5, 50, -1), b'control percentage')):
        assert not lib.dm_motifs_create(0, *args) and words in lib.dm_last_error(), args
    assert not lib.dm_motifs_create(99, 3, 3, b'A', 5, 50, 10) and b'no device 99' in lib.dm_last_error()
    h = lib.dm_motifs_create(0, 1, 1, b'A', 5, 50, 10)
    assert h
    seq = np.frombuffer(b'ACGTACGT', np.uint8)
    counters, off = np.zeros(10, np.int64), np.zeros(2, np.int64)
    tabs = [summary.PositionSummary(8) for _ in range(4)]
    short = summary.PositionSummary(7)
    p = [t._h for t in tabs]
    out = (counters.ctypes.data, off.ctypes.data)
    try:
        for call, words in ((lambda: lib.dm_motifs_count(None, seq.ctypes.data, 8, p[0], p[1], None, None, *out), b'null handle'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, None, p[1], None, None, *out), b'null handle'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], None, None, None, *out), b'null handle'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], p[0], None, None, *out), b'one per strand'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], p[1], p[2], None, *out), b'both of their tables or by neither'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], p[1], None, p[3], *out), b'both of their tables or by neither'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], p[1], p[2], p[0], *out), b'of their own'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], short._h, None, None, *out), b'table 1 has 7 positions, the contig 8'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], p[1], p[2], short._h, *out), b'table 3 has 7 positions'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 7, p[0], p[1], None, None, *out), b'positions, the contig 7'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 0, p[0], p[1], None, None, *out), b'1 to 2^31 - 1'),
                            (lambda: lib.dm_motifs_count(h, None, 8, p[0], p[1], None, None, *out), b'null argument'),
                            (lambda: lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], p[1], None, None, None, off.ctypes.data), b'null argument'),
                            (lambda: lib.dm_motifs_fetch(None, counters.ctypes.data), b'null handle'),
                            (lambda: lib.dm_motifs_fetch(h, None), b'null argument'),
                            (lambda: lib.dm_motifs_reset(None), b'null handle'),
                            (lambda: lib.dm_motifs_times(None, None, None), b'null handle')):
            assert call() == _lib.DM_EINVAL and words in lib.dm_last_error(), lib.dm_last_error()
        if lib.dm_device_count() > 1:                                  # a table on another device
            far = summary.PositionSummary(8, device=1)
            assert lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], far._h, None, None, *out) == _lib.DM_EINVAL and b'is on device 1' in lib.dm_last_error()
            far.close()
        # and the handle still works: empty tables, so the A at 4 and the T at 3 are shallow, the A at 0 and the T at 7 have no context
        assert lib.dm_motifs_count(h, seq.ctypes.data, 8, p[0], p[1], None, None, *out) == 0 and counters.tolist() == [0, 0, 1, 0, 1, 0, 0, 1, 0, 1] and not off.any()
        a, b = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
        assert lib.dm_motifs_times(h, ctypes.byref(a), ctypes.byref(b)) == 0 and a.value >= 0 and b.value >= 0
        lib.dm_motifs_destroy(None)
    finally:
        lib.dm_motifs_destroy(h)
        for t in tabs + [short]:
            t.close()


def test_command_on_the_device_equals_the_command_under_host_engine(hip_lib, tmp_path):
    root = str(tmp_path)
    case = motifs_synth.write_case(root)
    for key, with_control in (('with_control', True), ('without_control', False)):
        want = motifs_synth.run_command(case, root, with_control, motifs.HostEngine(3, 3, 'A'), 'host_' + key)
        got = motifs_synth.run_command(case, root, with_control, None, 'dev_' + key)                     # engine None: DeviceEngine on GPU 0
        assert got['txt'] == want['txt'], key
        got['json']['inputs'].pop('FileID'), want['json']['inputs'].pop('FileID')
        assert got['json'] == want['json'], key
        assert any('mod_pos.chr2-.A.bed: line 1 is outside the device grammar: the file is parsed on the host' in n for n in got['json']['notes'])
    assert [m['motif'] for m in got['json']['motifs']] == ['GATC', 'TGCAG']
