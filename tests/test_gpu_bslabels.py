"""GPU (-m gpu): `bslabels` on the device (csrc/bslabels.hip.inc) against its host twins: the classes and counters against bslabels.HostEngine,
exactly, at the wave, block and tile edges and at every edge of the rules; the text of the three lists against bslabels.format_lists_host byte for
byte, in many runs and in one; the truth path it shares with bsperf against dm_bsperf_parse_host; the command against
tests/golden/bslabels_case.json (tests/golden/make_golden_bslabels.py: plain dicts) and against what getfeatures reads from its files; and the
refusals of the C ABI."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import _lib, bslabels, bsperf, getfeatures

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HEADER = 'chrom\tstart\tend\tname\tscore\tstrand\tthickStart\tthickEnd\tcolor\tcoverage\tpercentage\n'
COV, HI, LO = 5, 90, 10
# (coverage, percentage) of replicate 0 and of every other replicate (None: no record) on consecutive sites: every class, coverage exactly c and
# c - 1, 65535 and a saturated 65536, the four percentage edges, a key in one replicate only, replicates that disagree; the last: a site without truth
SCENARIOS = [((30, 95), (30, 100)), ((COV, HI), (65536, HI)), ((COV - 1, 100), (30, 100)), ((30, HI - 1), (30, 100)), ((30, 0), (30, 0)), ((COV, LO), (65535, 0)),
             ((30, LO + 1), (30, 0)), ((COV - 1, 0), (30, 0)), ((30, 100), None), (None, (30, 0)), ((30, 100), (30, 0)), ((30, 50), (30, 50)), (None, None)]


def tile():
    return bslabels.tile_positions()


def make_contig(rng, length, motif, k, R):
    """-> (reference bytes, per replicate (pos, strand, cov, pct)): the motif about every sixth base, cut by both contig ends; SCENARIOS in turn on the
    sites of either strand, a record off the motif now and then, and keys at position 0 and length - 1 of both strands in every replicate."""
    m = len(motif)
    letters = list(motif[m // 2:] if m > 1 else motif)                            # the motif's tail at position 0: cut by the contig's start
    while len(letters) < length:
        letters += list(motif) if rng.random() < 0.35 else [str(rng.choice(list('ACGT')))]
    letters = letters[:length]
    head = motif[:max(m - 1, 1)]
    if length >= 2 * m:
        letters[length - len(head):] = list(head)                                  # and its head at the end
    seq = ''.join(letters).encode()
    code = bslabels.siteperf.site_codes(seq, motif, k)
    recs = [dict() for _ in range(R)]
    for s in range(2):
        sites = 0
        for q in range(length):
            if (code[q] >> s) & 1:
                first, others = SCENARIOS[sites % len(SCENARIOS)]
                sites += 1
                for r in range(R):
                    v = first if r == 0 else others
                    if v is not None:
                        recs[r][(s, q)] = v
            elif rng.random() < 0.08:
                for r in range(R):
                    if rng.random() < 0.7:
                        recs[r][(s, q)] = (int(rng.choice([1, 5, 30])), int(rng.choice([0, 50, 100])))
        for q in {0, length - 1}:
            for r in range(R):
                recs[r].setdefault((s, q), (30, 100))
    out = []
    for r in range(R):
        keys = list(recs[r])
        order = rng.permutation(len(keys))
        out.append(tuple(np.array([f(keys[i], recs[r][keys[i]]) for i in order], np.int64) for f in
                         (lambda key, v: key[1], lambda key, v: key[0], lambda key, v: v[0], lambda key, v: v[1])))
    return seq, out


def classify_both(dev, host, c, seq, motif, k, recs):
    """-> ((device counts, classes), (host counts, classes)) of contig c."""
    got = []
    for e in (dev, host):
        e.open(c, seq, motif, k)
        for r, (pos, strand, cov, pct) in enumerate(recs):
            e.fill(r, pos, bsperf.pack_meta(np.full(len(pos), c, np.int64), strand, cov, pct))
        counts = e.classify()
        got.append((counts, e.fetch_classes()))
    return got


def lengths_under_test():
    t = tile()
    return [1, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 3 * t + 7]


@pytest.mark.parametrize("R", [1, 2, 4])
@pytest.mark.parametrize("motif,k", [('C', 0), ('CG', 0), ('GATC', 1)])
def test_classes_equal_the_host_engine(gpu_device, motif, k, R):
    lengths = lengths_under_test()
    names = ['c%d' % n for n in lengths]
    rng = np.random.default_rng(100 * R + len(motif))
    dev = bslabels.DeviceEngine(names, lengths, R, COV, HI, LO, gpu_device)
    host = bslabels.HostEngine(names, lengths, R, COV, HI, LO)
    seen = np.zeros((2, 5), np.int64)
    try:
        for c, length in enumerate(lengths):
            seq, recs = make_contig(rng, length, motif, k, R)
            (dcounts, dcls), (hcounts, hcls) = classify_both(dev, host, c, seq, motif, k, recs)
            assert np.array_equal(dcounts, hcounts), (length, dcounts, hcounts)
            assert dcls.shape == hcls.shape == (2, length) and np.array_equal(dcls, hcls), (length, np.nonzero(dcls != hcls))
            assert all(dcls[s, q] != 0 for s in range(2) for q in (0, length - 1))           # the keys at both ends have truth
            seen += hcounts
            dev.close_contig()
    finally:
        dev.close()
    assert (seen > 0).all(), seen                                                  # every class and a site without truth, on either strand


def whole_text(dev, which, cap):
    """-> (lines, bytes, largest tile, the runs) of list `which` fetched with buffers of cap bytes (None: the largest tile's)."""
    n_lines, n_bytes, largest = dev.format_begin(which)
    runs, more = [], 1
    while more:
        more, text = dev.format_next(largest if cap is None else cap)
        assert text or not more
        if text:
            runs.append(text)
    return n_lines, n_bytes, largest, runs


def test_text_equals_the_host_formatter_in_many_runs_and_in_one(gpu_device):
    t = tile()
    names, lengths = ['chrT', 'empty'], [3 * t + 7, 300]
    dev = bslabels.DeviceEngine(names, lengths, 2, COV, HI, LO, gpu_device)
    host = bslabels.HostEngine(names, lengths, 2, COV, HI, LO)
    try:
        texts = []
        for attempt in range(2):                                                   # two runs give identical bytes
            seq, recs = make_contig(np.random.default_rng(7), lengths[0], 'CG', 0, 2)
            (dcounts, dcls), (hcounts, hcls) = classify_both(dev, host, 0, seq, 'CG', 0, recs)
            assert np.array_equal(dcls, hcls)
            want = bslabels.format_lists_host('chrT', hcls)
            got = {}
            for name, which in bslabels.LISTS.items():
                n_lines, n_bytes, largest, runs = whole_text(dev, which, None)
                assert b''.join(runs) == want[name], name
                assert (n_lines, n_bytes) == (want[name].count(b'\n'), len(want[name])) and n_lines == int(hcounts[:, which - 1].sum()) > 0
                assert 0 < largest <= n_bytes and all(len(r) <= largest for r in runs)
                assert len(runs) >= (3 if name == 'anymod' else 1)                 # anymod has lines in every tile
                n_lines1, n_bytes1, largest1, one = whole_text(dev, which, n_bytes)
                assert (n_lines1, n_bytes1, largest1) == (n_lines, n_bytes, largest) and one == [want[name]]
                got[name] = b''.join(runs)
                # a buffer one byte below the largest tile: DM_EINVAL, with the size; the handle stays usable
                dev.format_begin(which)
                with pytest.raises(_lib.DeepModHipError, match=r'%d bytes are needed' % largest) as err:
                    more = 1
                    while more:
                        more, _ = dev.format_next(largest - 1)
                assert err.value.code == _lib.DM_EINVAL
                assert b''.join(whole_text(dev, which, 2 * largest)[3]) == want[name]
            texts.append((got, dcls.copy(), dcounts.copy()))
            dev.close_contig()
        assert texts[0][0] == texts[1][0] and np.array_equal(texts[0][1], texts[1][1]) and np.array_equal(texts[0][2], texts[1][2])
        # a contig without truth: three empty lists
        for e in (dev, host):
            e.open(1, b'ACGT' * 75, 'CG', 0)
        counts = dev.classify()
        assert np.array_equal(counts, host.classify()) and counts[:, :4].sum() == 0 and counts[:, 4].tolist() == [75, 75]
        for which in bslabels.LISTS.values():
            assert dev.format_begin(which) == (0, 0, 0) and dev.format_next(16) == (0, b'') and dev.format_next(0) == (0, b'')
    finally:
        dev.close()


def test_text_reaches_seven_digits(gpu_device):
    """One contig of 1,000,001 positions with sites at 999,999 and 1,000,000 (8 to 10 digits: the host test of the same routine)."""
    length = 1000001
    seq = bytearray(b'A' * length)
    for q in (5, 99999, 100000, 999999, 1000000):
        seq[q] = ord('C')
    seq[7] = ord('G')                                                             # a '-' site
    dev = bslabels.DeviceEngine(['chrL'], [length], 1, COV, HI, LO, gpu_device)
    host = bslabels.HostEngine(['chrL'], [length], 1, COV, HI, LO)
    try:
        pos = np.array([5, 99999, 100000, 999999, 1000000, 7, 1000000, 12], np.int64)
        strand = np.array([0, 0, 0, 0, 0, 1, 1, 0], np.int64)
        recs = [(pos, strand, np.full(8, 30, np.int64), np.array([100, 0, 50, 100, 100, 100, 100, 100], np.int64))]
        (dcounts, dcls), (hcounts, hcls) = classify_both(dev, host, 0, bytes(seq), 'C', 0, recs)
        assert np.array_equal(dcounts, hcounts) and np.array_equal(dcls, hcls)
        assert hcounts[0].tolist() == [3, 1, 1, 1, 0] and hcounts[1].tolist() == [1, 0, 0, 1, 0]
        want = bslabels.format_lists_host('chrL', hcls)
        assert want['fulmod'] == b'chrL + 5\nchrL - 7\nchrL + 999999\nchrL + 1000000\n'
        for name, which in bslabels.LISTS.items():
            n_lines, n_bytes, largest, runs = whole_text(dev, which, None)
            assert b''.join(runs) == want[name] and n_bytes == len(want[name]), name
    finally:
        dev.close()


def make_long_contig(rng, length, R):
    """make_contig for motif CG in numpy: random letters, SCENARIOS in turn on the sites of either strand, records off the motif on 8 % of the other
    keys (each in 70 % of the replicates) -> (reference bytes, per replicate (pos, strand, cov, pct))."""
    seq = rng.choice(np.frombuffer(b'ACGT', np.uint8), length).tobytes()
    code = bslabels.siteperf.site_codes(seq, 'CG', 0)
    first = np.array([v[0] if v[0] is not None else (0, 0) for v in SCENARIOS], np.int64)
    others = np.array([v[1] if v[1] is not None else (0, 0) for v in SCENARIOS], np.int64)
    off_motif = [np.nonzero((((code >> s) & 1) == 0) & (rng.random(length) < 0.08))[0] for s in range(2)]
    out = []
    for r in range(R):
        parts = []
        for s in range(2):
            sites = np.nonzero((code >> s) & 1)[0]
            v = (first if r == 0 else others)[np.arange(len(sites)) % len(SCENARIOS)]
            have = v[:, 0] > 0                                                     # (None: no record)
            parts.append((sites[have], np.full(int(have.sum()), s), v[have, 0], v[have, 1]))
            off = off_motif[s][rng.random(len(off_motif[s])) < 0.7]
            parts.append((off, np.full(len(off), s), rng.choice([1, 5, 30], len(off)), rng.choice([0, 50, 100], len(off))))
        rows = [np.concatenate([p[j] for p in parts]).astype(np.int64) for j in range(4)]
        order = rng.permutation(len(rows[0]))
        out.append(tuple(a[order] for a in rows))
    return seq, out


def test_class_sweep_takes_a_second_pass_with_every_class(gpu_device):
    """300,001 positions: bl_class_kernel walks 2 x length = 600,002 keys with a grid of 524,288 threads, so 75,714 threads classify two keys and fold
    both into their counters (test_text_reaches_seven_digits crosses the cap too, with a handful of keys); every class in either pass."""
    grid = 2048 * 256                                                              # blk::MAX_BLOCKS x blk::THREADS
    length, R = 300001, 2
    assert grid < 2 * length < 2 * grid
    seq, recs = make_long_contig(np.random.default_rng(77), length, R)
    dev = bslabels.DeviceEngine(['chrW'], [length], R, COV, HI, LO, gpu_device)
    host = bslabels.HostEngine(['chrW'], [length], R, COV, HI, LO)
    try:
        (dcounts, dcls), (hcounts, hcls) = classify_both(dev, host, 0, seq, 'CG', 0, recs)
        assert np.array_equal(dcounts, hcounts), (dcounts, hcounts)
        assert dcls.shape == hcls.shape == (2, length) and np.array_equal(dcls, hcls), np.nonzero(dcls != hcls)
        flat = hcls.reshape(-1)                                                    # key e = strand x length + position, as the kernel walks them
        for part in (flat[:grid], flat[grid:]):
            assert set(np.unique(part).tolist()) == {0, 1, 2, 3, 4}                 # no truth, and the four classes
        assert (hcounts > 1000).all()
    finally:
        dev.close()


# ---- the truth path shared with bsperf ----
NAMES, LENGTHS =['chr1', 'chr10', 'chrX'], [3000, 2000, 2500]


def _truth_line(rng, i):
    name = ['chr1', 'chr10', 'chrX', 'chr', 'chr11'][int(rng.integers(0, 5))]
    pos = int(rng.integers(0, 2000))
    cov = int(rng.choice([0, 1, 4, 5, 65535, 65536, 2 ** 31 - 1]))
    strand = '+-.'[int(rng.integers(0, 3)) if i % 9 == 0 else int(rng.integers(0, 2))]
    f = [name, str(pos), str(pos + 1), '.', str(min(cov, 1000)), strand, str(pos), str(pos + 1), '0,0,0', str(cov), str(int(rng.integers(0, 101)))]
    kind = i % 5
    return ('\t'.join(f) + '\n' if kind == 0 else ' '.join(f) + ' \n' if kind == 1 else '  '.join(f) + '\n' if kind == 2 else ' \t' + ' \t '.join(f) + '\t\n' if kind == 3
            else 'chr1 1 2 . 1 +\n')


def test_truth_path_is_the_one_of_bsperf(gpu_device):
    """Lines for a little more than three tiles of text, every tile boundary inside a line: the records of add_truth_text are dm_bsperf_parse_host's; a
    chunk with a line outside the grammar adds nothing and reports the line; a key that occurs twice is reported as the smallest (position, strand)."""
    tile_bytes = bsperf.tile_bytes()
    rng = np.random.default_rng(29)
    out, total = [HEADER], len(HEADER)
    while total < 3 * tile_bytes + 600:
        ln = _truth_line(rng, len(out))
        if (total + len(ln)) % tile_bytes == 0:
            ln = ln[:-1] + ' \n'
        out.append(ln)
        total += len(ln)
    starts = np.cumsum([0] + [len(ln) for ln in out])
    assert not (starts[1:] % tile_bytes == 0).any()
    dev = bslabels.DeviceEngine(NAMES, LENGTHS, 2, COV, HI, LO, gpu_device)
    try:
        whole = ''.join(out)
        for first in (True, False):
            text = (whole if first else whole[len(HEADER):]).encode()
            (hpos, hmeta), hlines, hflag, hbad = bsperf.parse_device_grammar(text, NAMES, LENGTHS, first)
            assert (hflag, hbad) == (0, -1) and len(hpos) > 60 and (hlines[1:] > 0).sum() >= 4
            got, n, flag, bad = dev.add_truth_text(1, text, first)
            pos, meta = dev.records()
            assert (flag, bad) == (0, -1) and n == len(hpos) and np.array_equal(pos, hpos) and np.array_equal(meta, hmeta) and np.array_equal(got, hlines)
        k = int(np.searchsorted(starts, tile_bytes)) + 3                           # line k + 1 (1-based) starts in the second tile
        bad_text = (''.join(out[:k]) + 'chr1 5 6 . 7 + 5 6 0,0,0 7 42\r\n' + ''.join(out[k:k + 100])).encode()
        got, n, flag, bad = dev.add_truth_text(0, bad_text, True)
        assert (n, flag, bad) == (0, 1, k + 1) and got.sum() == 0 and len(dev.records()[0]) == 0
        hpos, hmeta, hl = bsperf.host_rows(bad_text, NAMES, LENGTHS, True)         # the host statement takes the chunk
        dev.add_truth_records(0, hpos, hmeta, hl)
        dpos, dmeta = dev.records()
        assert np.array_equal(dpos, hpos) and np.array_equal(dmeta, hmeta)
        # duplicates: in one call, and across two calls; another replicate is another dictionary
        dev.open(0, b'ACGT' * 750, 'C', 0)
        with pytest.raises(bslabels.BsLabelsError, match='replicate 0 holds position 4 of strand - twice'):
            dev.fill(0, [7, 4, 7, 4], bsperf.pack_meta([0] * 4, [1] * 4, [5] * 4, [0] * 4))
        with pytest.raises(_lib.DeepModHipError, match='refused'):
            dev.classify()
        dev.open(0, b'ACGT' * 750, 'C', 0)
        meta = bsperf.pack_meta([0, 0], [0, 1], [5, 5], [90, 90])
        dev.fill(0, [9, 9], meta)
        dev.fill(1, [9], meta[:1])
        with pytest.raises(bslabels.BsLabelsError, match='replicate 1 holds position 9 of strand \\+ twice'):
            dev.fill(1, [2999, 9], meta[[0, 0]])
    finally:
        dev.close()


# ---- the command ----
def golden():
    return json.load(open(os.path.join(GOLDEN, 'bslabels_case.json')))


def _write_case(g, folder, carriage_return=False):
    """genome.fa (chrB in lower case: the command upper-cases) and the two replicates -> (fasta, [replicates])."""
    fasta = folder / 'genome.fa'
    with open(fasta, 'w') as fh:
        for name, seq in g['reference'].items():
            seq = seq.lower() if name == 'chrB' else seq
            fh.write('>%s test\n' % name + ''.join(seq[i:i + 60] + '\n' for i in range(0, len(seq), 60)))
    reps = []
    for r, text in enumerate(g['replicates']):
        if carriage_return and r == 1:                                             # outside the device grammar, and another contig to split() and int()
            cut = text.index('\n', len(text) // 2) + 1
            text = text[:cut] + 'chrC 3 4 . 5 + 3 4 0,0,0 5 50\r\n' + text[cut:]
        path = folder / ('rep%d.bed' % (r + 1))
        path.write_text(text)
        reps.append(str(path))
    return str(fasta), reps


def _options(g, folder, fasta, reps, names=None):
    o = g['options']
    return {'truth': reps, 'Ref': fasta, 'Base': o['Base'], 'outFolder': str(folder / 'out'), 'FileID': 'case', 'chr': names or o['chr'], 'motif': o['motif'],
            'ModinMotif': o['ModinMotif'], 'cov': o['cov'], 'methylated': o['methylated'], 'unmethylated': o['unmethylated']}


def _check_files(g, folder, doc):
    for name, want in g['contigs'].items():
        for which in bslabels.LISTS:
            assert open(bslabels.list_path(str(folder / 'out'), 'case', which, name)).read() == want['texts'][which], (name, which)
        for strand in '+-':
            assert doc['contigs'][name][strand] == want['counts'][strand], (name, strand)


def test_command_equals_the_golden_case_and_feeds_getfeatures(gpu_device, tmp_path, capsys):
    g = golden()
    o = g['options']
    docs = []
    for sub, crlf in (('plain', False), ('crlf', True)):
        folder = tmp_path / sub
        folder.mkdir()
        fasta, reps = _write_case(g, folder, crlf)
        bslabels.bslabels(_options(g, folder, fasta, reps), gpu_device, chunk_bytes=1000)        # a dozen chunks per replicate
        doc = json.load(open(folder / 'out' / 'case_bslabels.json'))
        _check_files(g, folder, doc)
        docs.append(doc)
        for r, path in enumerate(reps):
            want = dict(g['lines'][r])
            if crlf and r == 1:
                want['other_contig'] += 1
                want['seen'] += 1
            assert doc['truth'][path] == dict({k: want[k] for k in bsperf.LINE_KEYS}, lines_seen=want['seen'])
    assert docs[0]['notes'] == [] and len(docs[1]['notes']) == 1 and 'rep2.bed: line ' in docs[1]['notes'][0] and 'parsed on the host' in docs[1]['notes'][0]
    assert set(docs[0]['kernel_ms']) == {'parse', 'fill', 'class', 'format'} and all(v > 0 for v in docs[0]['kernel_ms'].values())
    assert all(open(bslabels.list_path(str(tmp_path / 'plain' / 'out'), 'case', w, 'chrE')).read() == '' for w in bslabels.LISTS)   # in --chr, without truth
    capsys.readouterr()
    # the command line in a process of its own: the same files, and the lines getfeatures prints when it loads them
    folder = tmp_path / 'cli'
    folder.mkdir()
    fasta, reps = _write_case(g, folder)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'DeepMod.py'), 'bslabels', '--truth', ','.join(reps), '--Ref', fasta, '--Base', o['Base'],
                          '--outFolder', str(folder / 'out'), '--FileID', 'case', '--chr', ','.join(o['chr']), '--motif', o['motif'], '--ModinMotif', str(o['ModinMotif']),
                          '--cov', str(o['cov']), '--methylated', str(o['methylated']), '--unmethylated', str(o['unmethylated'])], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    doc = json.load(open(folder / 'out' / 'case_bslabels.json'))
    _check_files(g, folder, doc)
    printed = res.stdout.splitlines()
    fadict = getfeatures.readFA(fasta)
    mo = {'motifORPos': 2}
    mo.update({w: doc['patterns'][w] for w in bslabels.LISTS})
    assert all(os.path.join(str(folder / 'out'), 'case.%s.*.txt' % w) == doc['patterns'][w] and doc['patterns'][w] in printed[-1] for w in bslabels.LISTS)
    said = io.StringIO()
    with contextlib.redirect_stdout(said):
        lists = getfeatures.position_lists(mo, fadict)                            # the golden case goes into getfeatures --motifORPos 2 unchanged
    lists.close()
    theirs = said.getvalue().splitlines()
    ours = [ln for ln in printed if ' fulmod=' in ln]
    assert len(theirs) == 2 and all(ln in ours for ln in theirs)                   # chrA and chrB; getfeatures says nothing of a contig without a position
    assert ours == theirs + ['chrE fulmod=0 anymod=0 nomod=0']
    for which in bslabels.LISTS:
        read = getfeatures.readPosFiles(doc['patterns'][which], fadict)
        for name, entry in g['contigs'].items():
            for strand in '+-':
                want = sorted(p for s, p in entry['keys'][which] if s == strand)
                assert read.get(name, {'+': np.zeros(0), '-': np.zeros(0)})[strand].tolist() == want, (which, name, strand)


def test_command_refuses_a_duplicate_key_with_file_and_position(gpu_device, tmp_path):
    g = golden()
    fasta, reps = _write_case(g, tmp_path)
    text = open(reps[0]).read()
    dup = [ln for ln in text.split('\n')[1:] if ln.startswith('chrB') and len(ln) > 20 and ln.split('\t')[9] != '0' and ln.split('\t')[5] in '+-'][2]
    open(reps[0], 'w').write(text + dup + '\n')
    f = dup.split('\t')
    with pytest.raises(bslabels.BsLabelsError, match=r'rep1\.bed: chrB: replicate 0 holds position %s of strand \%s twice' % (f[1], f[5])):
        bslabels.bslabels(_options(g, tmp_path, fasta, reps), gpu_device)


# ---- the C ABI ----
def test_abi_refusals_launch_nothing_and_leave_the_handle_usable(gpu_device):
    ct = __import__('ctypes')
    lib = _lib.load()
    names = (ct.c_char_p * 2)(b'chr1', b'chr2')
    lens = np.array([8, 12], np.int64)

    def refused(rc, words, code=_lib.DM_EINVAL):
        assert rc == code and words in _lib.last_error(), (rc, _lib.last_error())

    unknown = np.array([8, -1], np.int64)
    for args, words in (((2, names, lens.ctypes.data, 5, 5, 90, 0), 'replicates'), ((2, names, lens.ctypes.data, 2, 0, 90, 0), 'coverage'),
                        ((2, names, lens.ctypes.data, 2, 65536, 90, 0), 'coverage'), ((2, names, lens.ctypes.data, 2, 5, 10, 10), 'unmethylated < methylated'),
                        ((2, names, None, 2, 5, 90, 0), 'every length known'), ((2, names, unknown.ctypes.data, 2, 5, 90, 0), 'every length known'),
                        ((0, names, lens.ctypes.data, 2, 5, 90, 0), 'contig names')):
        assert not lib.dm_bslabels_create(gpu_device, *args) and words in _lib.last_error(), (args, _lib.last_error())
    h = lib.dm_bslabels_create(gpu_device, 2, names, lens.ctypes.data, 2, 5, 90, 0)
    assert h
    try:
        seq = np.frombuffer(b'ACGCGTAC', np.uint8)
        counts = np.zeros((2, 5), np.int64)
        cls = np.zeros((2, 8), np.uint8)
        a, b, c = ct.c_int64(), ct.c_int64(), ct.c_int64()
        refused(lib.dm_bslabels_classify(h, counts.ctypes.data), 'no contig is open')
        refused(lib.dm_bslabels_open(h, 2, seq.ctypes.data, 8, b'CG', 2, 0), 'contig 2 of 2')
        refused(lib.dm_bslabels_open(h, -1, seq.ctypes.data, 8, b'CG', 2, 0), 'contig -1 of 2')
        refused(lib.dm_bslabels_open(h, 0, seq.ctypes.data, 7, b'CG', 2, 0), '7 reference bytes for a contig of 8')
        refused(lib.dm_bslabels_open(h, 1, seq.ctypes.data, 8, b'CG', 2, 0), '8 reference bytes for a contig of 12')
        refused(lib.dm_bslabels_open(h, 0, seq.ctypes.data, 8, b'CNG', 3, 0), 'none of A, C, G, T')
        refused(lib.dm_bslabels_open(h, 0, seq.ctypes.data, 8, b'CG', 2, 2), 'modified offset 2')
        refused(lib.dm_bslabels_open(h, 0, seq.ctypes.data, 8, b'CGCGCGCGC', 9, 0), 'motif of 9 bases')
        assert lib.dm_bslabels_fill(h, 0, 0, None, None, None, None) == _lib.DM_ESTATE           # nothing is open after a refused open
        assert lib.dm_bslabels_open(h, 0, seq.ctypes.data, 8, b'CG', 2, 0) == 0
        pos, meta = np.array([1, 3], np.int32), bsperf.pack_meta([0, 0], [0, 0], [30, 30], [100, 100])
        refused(lib.dm_bslabels_fill(h, 2, 2, pos.ctypes.data, meta.ctypes.data, None, None), 'replicate 2 of 2')
        beyond, other = np.array([8], np.int32), bsperf.pack_meta([1], [0], [30], [100])
        refused(lib.dm_bslabels_fill(h, 0, 1, beyond.ctypes.data, meta.ctypes.data, None, None), 'position 8 of 8')
        refused(lib.dm_bslabels_fill(h, 0, 1, pos.ctypes.data, other.ctypes.data, None, None), 'the open one is 0')
        refused(lib.dm_bslabels_add_truth_text(h, 2, b'x\n', 2, 0, None, None, None, None), 'replicate 2 of 2')
        assert lib.dm_bslabels_format_begin(h, 1, ct.byref(a), ct.byref(b), ct.byref(c)) == _lib.DM_ESTATE     # before classify
        assert lib.dm_bslabels_fetch_classes(h, cls.ctypes.data) == _lib.DM_ESTATE
        for r in range(2):
            assert lib.dm_bslabels_fill(h, r, 2, pos.ctypes.data, meta.ctypes.data, None, None) == 0
        assert lib.dm_bslabels_classify(h, counts.ctypes.data) == 0
        assert counts.tolist() == [[2, 0, 0, 0, 0], [0, 0, 0, 0, 2]]
        refused(lib.dm_bslabels_classify(h, counts.ctypes.data), 'has been classified')
        for which in (0, 4, -1):
            refused(lib.dm_bslabels_format_begin(h, which, ct.byref(a), ct.byref(b), ct.byref(c)), 'list %d' % which)
        assert lib.dm_bslabels_format_begin(h, 1, ct.byref(a), ct.byref(b), ct.byref(c)) == 0 and (a.value, b.value, c.value) == (2, 18, 18)
        buf = ct.create_string_buffer(32)
        refused(lib.dm_bslabels_format_next(h, buf, 17, ct.byref(a)), '18 bytes are needed')
        assert lib.dm_bslabels_format_next(h, buf, 18, ct.byref(a)) == 0 and buf.raw[:a.value] == b'chr1 + 1\nchr1 + 3\n'
        assert lib.dm_bslabels_fetch_classes(h, cls.ctypes.data) == 0 and cls.tolist() == [[0, 1, 0, 1, 0, 0, 0, 0], [0] * 8]
        assert lib.dm_bslabels_close_contig(h) == 0
    finally:
        lib.dm_bslabels_destroy(h)
