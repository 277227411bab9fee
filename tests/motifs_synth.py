"""TEST INFRASTRUCTURE - not part of the product.  The synthetic case of the `motifs` command that tests/test_motifs_host.py (under HostEngine) and
tests/test_gpu_motifs.py (on the device) both run: a reference of two contigs, a sample of two runs and one control run, as mod_pos BED files.

chr1 is 12,800 random bases with 40 GATC and 25 TGCAG planted; chr2 is 500 with 8 and 3.  In the sample every A of a GATC (index 1) and of a TGCAG
(index 3) is modified, planted or not, and no other A; in the control only the A of TGCAG is.  So with the control the only motif is GATC, and
without it TGCAG comes second.  The sizes follow from the selection rule: a pattern with f fixed letters matches about R = (N / 2) / 4^f keys of a
random contig of N bases, a quarter of the matches of a sub-pattern one letter short of a motif are that motif by chance, and a planted palindrome
is a key on either strand.  So a two-letter sub-pattern of GATC holds about 100 + 80 modified among 400 + 80 keys (below --minFrac 50) and GATC
itself only modified ones; a three-letter sub-pattern of TGCAG about 25 + 25 among 100 + 25, TGCAG itself about 50, all modified."""
import os

import numpy as np

COMP = {'A': 'T', 'C': 'G', 'G': 'C', 'T': 'A'}
BASE = 'A'


def _contig(rng, length, planted):
    letters = list(rng.choice(list('ACGT'), length))
    slots = rng.permutation((length - 40) // 10)[:sum(n for _, n in planted)]      # one motif per slot of 10 bases, none within 20 of an end
    words = [w for w, n in planted for _ in range(n)]
    for slot, word in zip(slots, words):
        at = 20 + 10 * int(slot)
        letters[at:at + len(word)] = list(word)
    return ''.join(letters)


def _oriented(seq, strand, p, lo, hi):
    """The oriented letters at offsets lo..hi of position p ('' where the contig ends)."""
    out = []
    for j in range(lo, hi + 1):
        q = p + j if strand == '+' else p - j
        out.append('' if q < 0 or q >= len(seq) else (seq[q] if strand == '+' else COMP[seq[q]]))
    return ''.join(out)


def _in_motif(seq, strand, p):
    """(the key is the A of a GATC, the key is the A of a TGCAG)"""
    return _oriented(seq, strand, p, -1, 2) == 'GATC', _oriented(seq, strand, p, -3, 1) == 'TGCAG'


def _line(chrom, p, strand, cov, mod):
    return ' '.join([chrom, str(p), str(p + 1), BASE, str(min(cov, 1000)), strand, str(p), str(p + 1), '0,0,0', str(cov), str(100 * mod // max(cov, 1)), str(mod), '\n'])


def write_case(root: str) -> dict:
    """Writes genome.fa, sample/run1, sample/run2 and control/run1 below root -> {'Ref', 'predFolder', 'control', 'reference': {contig: bases}}."""
    rng = np.random.default_rng(7)
    ref = {'chr1': _contig(rng, 12800, (('GATC', 40), ('TGCAG', 25))), 'chr2': _contig(rng, 500, (('GATC', 8), ('TGCAG', 3)))}
    with open(os.path.join(root, 'genome.fa'), 'w') as fh:
        for name, seq in ref.items():
            fh.write('>%s synthetic\n' % name)
            for i in range(0, len(seq), 60):
                fh.write((seq[i:i + 60].lower() if i % 600 == 0 else seq[i:i + 60]) + '\n')       # some lines in lower case: the command folds case
    texts = {}
    for name, seq in ref.items():
        for strand in '+-':
            rows = {('sample', 'run1'): [], ('sample', 'run2'): [], ('control', 'run1'): []}
            for p in range(len(seq)):
                letter = seq[p] if strand == '+' else COMP[seq[p]]
                if letter != BASE:
                    if p % 997 == 5:                                                  # a line on a letter that is not the base: off_base
                        rows[('sample', 'run1')].append(_line(name, p, strand, 3, 0))
                    continue
                gatc, tgcag = _in_motif(seq, strand, p)
                shallow = rng.random() < 0.08
                for run in ('run1', 'run2'):
                    cov = 2 if shallow else 6
                    mod = cov if (gatc or tgcag) else int(rng.random() < 0.3)
                    rows[('sample', run)].append(_line(name, p, strand, cov, mod))
                if rng.random() < 0.9:                                                # the rest: no control record, no_control
                    rows[('control', 'run1')].append(_line(name, p, strand, 10, 9 if tgcag else int(rng.random() < 0.5)))
            for (role, run), lines in rows.items():
                texts[(role, run, name, strand)] = ''.join(lines)
    texts[('sample', 'run2', 'chr2', '-')] = texts[('sample', 'run2', 'chr2', '-')].replace('\n', '\r\n')      # outside the device grammar: parsed on the host
    for (role, run, name, strand), text in texts.items():
        folder = os.path.join(root, role, run)
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, 'mod_pos.%s%s.%s.bed' % (name, strand, BASE)), 'w', newline='') as fh:
            fh.write(text)
    return {'Ref': os.path.join(root, 'genome.fa'), 'predFolder': os.path.join(root, 'sample'), 'control': os.path.join(root, 'control'), 'reference': ref}


def run_command(case: dict, root: str, with_control: bool, engine, fileid: str) -> dict:
    """The command on the case under `engine` -> {'txt': the report, 'json': the document as written, root replaced by <root> and `times` dropped}."""
    import json
    from deepmod_amd import motifs
    out = os.path.join(root, 'out')
    mo = {'predFolder': case['predFolder'], 'control': [case['control']] if with_control else [], 'Ref': case['Ref'], 'Base': BASE, 'outFolder': out, 'FileID': fileid,
          'flank': '3,3', 'threads': 2}
    motifs.motifs(mo, engine=engine)
    with open(os.path.join(out, fileid + '_motifs.txt')) as fh:
        txt = fh.read()
    with open(os.path.join(out, fileid + '_motifs.json')) as fh:
        doc = json.loads(fh.read().replace(root, '<root>'))
    doc.pop('times')
    return {'txt': txt, 'json': doc}


def main():
    """python tests/motifs_synth.py: regenerates tests/golden/motifs_command.json, the command's two outputs under HostEngine with and without the control."""
    import json
    import sys
    import tempfile
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    from deepmod_amd import motifs
    with tempfile.TemporaryDirectory() as root:
        case = write_case(root)
        doc = {key: run_command(case, root, ctrl, motifs.HostEngine(3, 3, BASE), key) for key, ctrl in (('with_control', True), ('without_control', False))}
    with open(os.path.join(here, 'golden', 'motifs_command.json'), 'w') as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
