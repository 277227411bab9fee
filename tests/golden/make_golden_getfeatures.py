"""Golden vectors for `getfeatures`, produced by running the REFERENCE's own handle_record / get_Feature / readFA / readMotifMod
(bin/DeepMod_scripts/myGetFeatureBasedPos.py) in the build container with the stub `tensorflow` / `h5py` modules of make_golden_host.import_reference:
`myDetect.getRefSeq` (samtools) is replaced by an in-memory genome, f5data is synthetic as in make_golden_record.py.

Output: tests/golden/getfeatures/<scenario>.json.gz - the FASTA text, the options, the position lists (as the reference holds them), per read the SAM
fields and the event table, and the reference's results: the decompressed text of every <k>.xy.gz, the lines of every <k>.xy.ind, the error channel.

Scenarios (reads of 500-700 events; the two reads around a kept share of 0.9 need 1,299 / 1,300 / 1,310 aligned events - with 200 padding rows of
which at most 50 are kept, no shorter read can pass 0.9):
  cg_neg      motif CG / 0, posneg 0: both strands, a motif at both contig ends, lower case and N in the FASTA, a read of 499 aligned events, a read on
              a contig without sites, a read with no labelled row
  cg_pos      motif CG / 0, posneg 1: indels inside and next to sites, both C-G swap shapes (:298-319), the motif in the read but not in the reference
              (:379-382), an insertion that shares its refbasei with a labelled base, a gappy read (:409-444), kept shares just below / at / above 0.9
  cg_pos_share  the reads at and above a kept share of 0.9
  gatc_pos    motif GATC / 1, posneg 1: no swap; the base of interest is not the first
  gatc_neg    the same motif, posneg 0
  ccagg_pos   motif CCAGG / 1, posneg 1: a motif that is not its own reverse complement
  lists_neg / lists_pos   --motifORPos 2 with all three lists
  three_files the cg_neg reads with a size_per_batch of 56,000 bytes: three files

Run only where the reference is (needs /root/reference):  python tests/golden/make_golden_getfeatures.py
"""
from __future__ import annotations

import copy
import glob
import gzip
import json
import os
import sys
import tempfile
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_host import EVENT_DTYPE, import_reference  # noqa: E402

OUT = os.path.join(HERE, 'getfeatures')
COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A', 'N': 'N'}


def revcomp(s):
    return ''.join(COMP[c] for c in reversed(s))


def make_read(rng, genome, name, rname, strand, ops, start, lead=0, tail=0):
    """ops in reference orientation: ('M', n) copies the reference, ('m', n) mismatches, ('s', 'ACG') substitutes exactly these bases (CIGAR M),
    ('I', n) random insertions, ('i', 'CG') inserts exactly these bases, ('D', n) deletions.  -> SAM fields + the basecall."""
    pos, seq, cig = start, [], []

    def push(op, n):
        if cig and cig[-1][0] == op:
            cig[-1][1] += n
        else:
            cig.append([op, n])
    for op, arg in ops:
        if op == 'M':
            seq.append(genome[pos:pos + arg].replace('N', 'A')); pos += arg; push('M', arg)
        elif op == 'm':
            for _ in range(arg):
                seq.append(str(rng.choice([b for b in 'ACGT' if b != genome[pos]]))); pos += 1
            push('M', arg)
        elif op == 's':
            seq.append(arg); pos += len(arg); push('M', len(arg))
        elif op == 'I':
            seq.append(''.join(rng.choice(list('ACGT'), arg))); push('I', arg)
        elif op == 'i':
            seq.append(arg); push('I', len(arg))
        elif op == 'D':
            pos += arg; push('D', arg)
    samseq = ''.join(rng.choice(list('ACGT'), lead)) + ''.join(seq) + ''.join(rng.choice(list('ACGT'), tail))
    cigar = ('%dS' % lead if lead else '') + ''.join('%d%s' % (n, op) for op, n in cig) + ('%dS' % tail if tail else '')
    return {'name': name, 'rname': rname, 'flag': 0 if strand == '+' else 16, 'pos': start + 1, 'cigar': cigar, 'seq': samseq,
            'basecall': samseq if strand == '+' else revcomp(samseq)}


def random_ops(rng, span, p_mis=0.05, p_ins=0.03, p_del=0.03, edge=4):
    ops, used = [('M', edge)], edge
    while used < span - edge:
        u = rng.random()
        if u < p_ins:
            ops.append(('I', int(rng.integers(1, 4))))
        elif u < p_ins + p_del:
            n = min(int(rng.integers(1, 4)), span - edge - used); ops.append(('D', n)); used += n
        elif u < p_ins + p_del + p_mis:
            ops.append(('m', 1)); used += 1
        else:
            n = min(int(rng.integers(1, 12)), span - edge - used); ops.append(('M', n)); used += n
    ops.append(('M', span - used))
    return ops


def events_for(rng, rd):
    n = len(rd['basecall'])
    ev = np.zeros(n, dtype=EVENT_DTYPE)
    ev['mean'] = np.round(np.clip(rng.normal(0, 1.2, n), -5, 5), 3)
    ev['stdv'] = np.round(np.abs(rng.normal(0.25, 0.15, n)), 3)
    ev['length'] = rng.geometric(0.12, n)
    ev['start'] = np.cumsum(np.r_[0, ev['length'][:-1]])
    ev['model_state'] = ['NN' + b + 'NN' for b in rd['basecall']]
    rd['ev_mean'] = [float(v) for v in ev['mean']]
    rd['ev_stdv'] = [float(v) for v in ev['stdv']]
    rd['ev_length'] = [int(v) for v in ev['length']]
    return ev


def genomes(rng):
    """chrS: random, CG at both ends, a CG-free stretch, planted C-G swap material and motif-in-read material; chrQ: no C at all (no site of any motif
    used here); the FASTA carries lower-case lines and an N run."""
    g = list(''.join(rng.choice(list('ACGT'), 9000)))
    g[0:2] = 'CG'
    g[-2:] = 'CG'
    s = ''.join(g)
    free = ''.join(rng.choice(list('AT'), 800))                                            # neither C nor G: no site of any motif used here, on either strand
    s = s[:4000] + free + s[4800:]
    s = s[:1500] + 'ACGGGTTACCGTA' + s[1513:]                                               # reference "CGG" and "CCG" (:298-319)
    s = s[:1700] + 'TTCATTGATTTT' + s[1712:]                                                # "CA" / "GAT": the read will say "CG" / "GATC"
    s = s[:6000] + 'N' * 12 + s[6012:]
    q = ''.join(rng.choice(list('AT'), 1500))
    fasta = '>chrS synthetic\n'
    for i in range(0, len(s), 60):
        line = s[i:i + 60]
        fasta += (line.lower() if (i // 60) % 5 == 2 else line) + '\n'
    fasta += '\n>chrQ no sites\n' + '\n'.join(q[i:i + 70] for i in range(0, len(q), 70)) + '\n'
    return {'chrS': s, 'chrQ': q}, fasta


def run_reference(gf, genome, fasta_path, mo, reads, f5data, f5align, pos_lists=None):
    """-> (files {k: {'xy': text, 'ind': text}}, errors, the lists as sorted [strand, pos] pairs per contig)"""
    mo = copy.deepcopy(mo)
    fadict = gf.readFA(fasta_path, mo['region'][0])
    assert {k: v for k, v in fadict.items()} == genome
    if mo['motifORPos'] == 1:
        mo['fulmodlist'], _ = gf.readMotifMod(fadict, mo['motif'][0], mo['motif'][1], mo['region'][0], mo['region'][1], mo['region'][2])
        mo['anymodlist'] = None
        mo['nomodlist'] = None
    else:
        for mthi, key in enumerate(('fulmodlist', 'anymodlist', 'nomodlist')):
            mo[key] = defaultdict(lambda: defaultdict())
            for tchr, tstrand, tpos in pos_lists[key]:
                mo[key][tchr][(tstrand, int(tpos))] = [1 - mthi, fadict[tchr][int(tpos)]]
    gf.myDetect.getRefSeq = lambda mopt, sp, rname: sp['ref_info'].__setitem__(rname, genome[rname])
    tmp = tempfile.mkdtemp()
    sp_options = defaultdict()
    sp_options.update({'ctfolder': tmp, 'Error': defaultdict(list)})
    sp_param = defaultdict()
    sp_param.update({'f5data': f5data, 'ref_info': defaultdict(), 'f5status': '', 'line': ''})
    gf.handle_record(mo, sp_options, sp_param, f5align, f5data)
    files = {}
    for fn in sorted(glob.glob(os.path.join(tmp, '*.xy.gz')), key=lambda p: int(os.path.basename(p).split('.')[0])):
        k = os.path.basename(fn).split('.')[0]
        files[k] = {'xy': gzip.open(fn, 'rt').read(), 'ind': open(fn[:-3] + '.ind').read()}
    lists = {}
    for key in ('fulmodlist', 'anymodlist', 'nomodlist'):
        lists[key] = None if mo[key] is None else {c: sorted([s, int(p)] for (s, p) in d.keys()) for c, d in mo[key].items()}
    return files, {k: list(v) for k, v in sp_options['Error'].items()}, lists


def main():
    import_reference()
    from DeepMod_scripts import myGetFeatureBasedPos as gf
    rng = np.random.default_rng(2024)
    genome, fasta = genomes(rng)
    os.makedirs(OUT, exist_ok=True)
    fasta_path = os.path.join(tempfile.mkdtemp(), 'genome.fa')
    open(fasta_path, 'w').write(fasta)
    S = genome['chrS']

    def rd(name, strand, ops, start, rname='chrS', lead=0, tail=0):
        return make_read(rng, genome[rname], name, rname, strand, ops, start, lead, tail)
    swap = [('M', 60), ('M', 2), ('D', 1), ('M', 1), ('D', 2), ('M', 4), ('M', 1), ('D', 1)]     # at 1440: the two C-G shapes of make_golden_record.py
    plain = [
        rd('fwd_from_contig_start', '+', random_ops(rng, 620), 0, lead=6, tail=3),
        rd('rev_to_contig_end', '-', random_ops(rng, 640), len(S) - 640, lead=4, tail=8),
        rd('fwd_over_N_and_lower', '+', random_ops(rng, 560, p_ins=0.02, p_del=0.02), 5700),
        rd('short_499', '+', [('M', 499)], 2500, lead=3, tail=2),
        rd('aligned_500', '-', [('M', 500)], 3000, lead=2),
        rd('no_site_contig', '+', random_ops(rng, 560), 300, rname='chrQ'),
        rd('no_labelled_row', '+', [('M', 620)], 4090),
        rd('rev_plain', '-', random_ops(rng, 530), 7200, lead=5, tail=5),
    ]
    indel = [
        rd('swap_fwd', '+', swap + [('M', 520)], 1440),
        rd('swap_rev', '-', swap + [('M', 520)], 1440),
        # reference TTCATTGATTTT at 1700: the read says CG where the reference has CA, and GATC where it has GATT
        rd('motif_in_read_fwd', '+', [('M', 102), ('s', 'G'), ('M', 5), ('s', 'C'), ('M', 500)], 1600),
        rd('motif_in_read_rev', '-', [('M', 102), ('s', 'G'), ('M', 5), ('s', 'C'), ('M', 500)], 1600),
        rd('indels_fwd', '+', random_ops(rng, 600, p_ins=0.06, p_del=0.06), 2100, lead=3),
        rd('indels_rev', '-', random_ops(rng, 600, p_ins=0.06, p_del=0.06), 2800, tail=4),
        rd('gappy_fwd', '+', random_ops(rng, 560, p_mis=0.08, p_ins=0.16, p_del=0.16), 5000),
        rd('gappy_rev', '-', random_ops(rng, 560, p_mis=0.08, p_ins=0.16, p_del=0.16), 6400),
    ]
    # an insertion in front of / behind every kind of site neighbourhood: "CG" gets an inserted base before the C, between C and G, and a deleted G
    variants = [[('i', 'A')], [('M', 1), ('i', 'T')], [('M', 1), ('D', 1)], [('D', 1)], [('i', 'CG')], [('M', 2), ('i', 'G')], [('D', 2)], [('m', 1)], [('M', 1), ('m', 1)]]
    ops, at = [('M', 4)], 7290
    for p in [i for i in range(7300, 7900) if S[i:i + 2] == 'CG']:
        if p < at + 3 or not variants:
            continue
        var = variants.pop(0)
        ops += [('M', p - at)] + var
        at = p + sum(a for o, a in var if o in 'MmD')                 # the reference bases the variant consumes
    assert not variants
    ops.append(('M', 7286 + 640 - at))
    indel.append(rd('site_indels_fwd', '+', ops, 7286))
    indel.append(rd('site_indels_rev', '-', ops, 7286))
    share = [rd('share_below_1299', '+', [('M', 1299)], 100), rd('share_equal_1300', '-', [('M', 1300)], 1000), rd('share_above_1310', '+', [('M', 1310)], 2300)]

    def pack(reads):
        recs, f5data, f5align = [], {}, {}
        for r in reads:
            r = dict(r)
            ev = events_for(rng, r)
            f5data[r['name']] = (r['basecall'], ev, None, '/wrk/' + r['name'] + '.fast5', (0, 0))
            f5align[r['name']] = (60, r['flag'], r['rname'], r['pos'], r['cigar'], r['seq'])
            recs.append(r)
        return recs, f5data, f5align

    def scenario(name, mo, reads, pos_lists=None):
        recs, f5data, f5align = pack(reads)
        base = {'region': [None, None, None], 'outLevel': 2, 'fnum': 7, 'windowsize': 21, 'size_per_batch': 1 * 10 ** 7}
        base.update(mo)
        files, errors, lists = run_reference(gf, genome, fasta_path, base, recs, f5data, f5align, pos_lists)
        out = {'fasta': fasta, 'options': {k: base[k] for k in ('motifORPos', 'posneg', 'size_per_batch') if k in base}, 'motif': base.get('motif'),
               'lists': lists, 'reads': recs, 'files': files, 'errors': errors}
        with gzip.GzipFile(os.path.join(OUT, name + '.json.gz'), 'wb', mtime=0) as fh:
            fh.write(json.dumps(out).encode())
        print(name, 'files', {k: (v['xy'].count('\n'), v['ind'].count('\n')) for k, v in files.items()}, 'errors', errors,
              os.path.getsize(os.path.join(OUT, name + '.json.gz')), 'bytes')

    cg = {'motifORPos': 1, 'motif': ['CG', 0]}
    scenario('cg_neg', dict(cg, posneg=0), plain)
    scenario('three_files', dict(cg, posneg=0, size_per_batch=56000), plain)
    scenario('cg_pos', dict(cg, posneg=1), indel + share[:1])
    scenario('cg_pos_share', dict(cg, posneg=1), share[1:] + plain[:1])
    scenario('gatc_pos', {'motifORPos': 1, 'motif': ['GATC', 1], 'posneg': 1}, indel[:8] + plain[:2])
    scenario('gatc_neg', {'motifORPos': 1, 'motif': ['GATC', 1], 'posneg': 0}, indel[:4] + plain[:2])
    scenario('ccagg_pos', {'motifORPos': 1, 'motif': ['CCAGG', 1], 'posneg': 1}, indel[4:8] + plain[:2])
    # position lists: C positions on both strands, drawn from the bases the reads cover; some positions sit in two lists
    cpos = [('+', i) for i in range(0, 9000) if S[i] == 'C'] + [('-', i) for i in range(0, 9000) if S[i] == 'G']
    pick = lambda frac: [['chrS', s, p] for (s, p) in cpos if rng.random() < frac]
    lists = {'fulmodlist': pick(0.08), 'anymodlist': pick(0.05), 'nomodlist': pick(0.30)}
    scenario('lists_neg', {'motifORPos': 2, 'posneg': 0}, plain[:3] + indel[:2] + indel[4:6], lists)
    scenario('lists_pos', {'motifORPos': 2, 'posneg': 1}, plain[:3] + indel[:2] + indel[4:10], lists)


if __name__ == '__main__':
    main()
