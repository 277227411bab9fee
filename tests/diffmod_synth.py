"""TEST INFRASTRUCTURE - not part of the product.  The cases of `diffmod` that tests/test_diffmod_host.py (HostEngine and the compiled host twin),
tests/test_gpu_diffmod.py (the device) and tests/golden/make_golden_diffmod.py share.

Condition on the inputs.  A table whose probability ratio to the observed one lies in (1, 1 + 1e-5] without being an exact tie sits on the edge of the
inclusion rule (1 + 1e-7): rounding of the 36 ulp the error bound allows could decide it either way.  on_edge() finds such keys with the oracle's
integers, and every generator here drops them (random_keys reports how many: 1 % at most is allowed).

The error bound (derived, not measured): relative 1e-9 for N = cA + cB <= 4096, 1e-6 above; for an exact p below 1e-290 only that the
result is <= 1e-289 (check_p).

The synthetic command case (write_case): two contigs, chrA of 2,600 positions with files for both strands and chrB of 700; a sample of two runs
and two control folders of one run each, as mod_pos BED files.  Sample and control of a site are drawn from the same per-site rate, except 40
planted sites at 80 % in the sample and 10 % in the controls (the other way round where the position is a multiple of 4); a few sites are shallow in the sample or in the controls, one control file has \\r\\n
line ends (outside the device grammar: parsed on the host), and the site DELTA_SITE sits exactly on --minDelta 10."""
import os

import numpy as np

BASE = 'C'
COV = 5
FDR = 0.05
DELTA_SITE = ('chrA', 2500, '+', (2000, 600), (2000, 400))   # 30 % against 20 %: exactly 10 points, p about 1e-12: listed at --minDelta 10, not at 11
SUPPORTS = (1, 2, 16, 17, 64, 65)


def on_edge(cA, mA, cB, mB) -> bool:
    from deepmod_amd import diffmod
    lo, ws = diffmod.exact_weights(cA, mA, cB, mB)
    wo = ws[mA - lo]
    return any(wo < w and w * 10 ** 5 <= wo * (10 ** 5 + 1) for w in ws)


def check_p(got: float, exact: float, total: int, what=None):
    """The bound of the issue: relative 1e-9 for N <= 4096, 1e-6 above; below 1e-290 only an upper bound."""
    if exact < 1e-290:
        assert 0.0 <= got <= 1e-289, (what, got, exact)
    else:
        bound = 1e-9 if total <= 4096 else 1e-6
        assert abs(got - exact) <= bound * exact, (what, got, exact, abs(got - exact) / exact)


def random_keys(seed: int, n: int, max_cov: int = 300):
    """n random keys (cA, mA, cB, mB) with coverages 1..max_cov, the ones on the edge dropped -> (keys, dropped)."""
    rng = np.random.default_rng(seed)
    keys, dropped = [], 0
    while len(keys) < n:
        cA, cB = int(rng.integers(1, max_cov + 1)), int(rng.integers(1, max_cov + 1))
        rate = rng.random()
        mA, mB = int(rng.binomial(cA, rate)), int(rng.binomial(cB, rate if rng.random() < 0.7 else rng.random()))
        if on_edge(cA, mA, cB, mB):
            dropped += 1
            continue
        keys.append((cA, mA, cB, mB))
    return keys, dropped


def key_with_support(S: int, share: float = 0.6):
    """A key whose support has exactly S tables: M = S - 1, both coverages M + 5."""
    M = S - 1
    mA = int(round(share * M))
    return (M + 5, mA, M + 5, M - mA)


def sweep_keys(small_support: int, max_total: int):
    """The keys of the GPU sweep test, each fate and each path of the test kernel: (cA, mA, cB, mB) in the order they are laid out."""
    keys = [key_with_support(S) for S in SUPPORTS + (small_support, small_support + 1)]
    keys += [key_with_support(S, 0.5) for S in (2, 17, small_support + 1)]
    keys += [(5000, 2600, 5000, 2400), (5000, 5000, 5000, 0), (700, 10, 900, 600)]        # S = 5001 twice (the second underflows), a lopsided one
    keys += [(max_total // 2, 30, max_total // 2, 10), (max_total - 6, 3, 6, 2)]            # exactly at MAX_TOTAL: tested
    keys += [(max_total // 2 + 1, 30, max_total // 2, 10), (max_total, 0, COV, 0)]          # one above, and far above: too_deep
    keys += [(COV - 1, 1, 30, 3), (0, 0, 30, 3), (30, 3, COV - 1, 0), (30, 3, 0, 0), (COV, COV, COV, 0), (COV, 0, COV, 0), (9, 9, 9, 9)]
    assert not any(cA >= COV and cB >= COV and cA + cB <= max_total and on_edge(cA, mA, cB, mB) for cA, mA, cB, mB in keys)
    return keys


def layout(keys, length: int, tile: int, phase: int):
    """The keys on a contig of `length` positions: on the last and the first position of every tile, at both ends, and spread over the rest; on
    both strands (alternating, starting with strand phase & 1) -> {'sample': (pos, strand, cov, mod), 'control': ..} with zero-coverage records left out."""
    spots = [0, length - 1] + [e + d for e in range(tile, length, tile) for d in (-1, 0)]
    spots += [int(x) for x in np.linspace(1, max(length - 2, 1), 3 * len(keys))]
    spots = sorted({p for p in spots if 0 <= p < length})
    recs = {'sample': [], 'control': []}
    for i, p in enumerate(spots):
        for s in range(2):
            cA, mA, cB, mB = keys[(2 * i + s + phase) % len(keys)]
            if (i + s + phase) % 7 == 3:
                continue                                              # a position of one strand only
            if cA:
                recs['sample'].append((p, s, cA, mA))
            if cB:
                recs['control'].append((p, s, cB, mB))
    return {k: tuple(np.array([r[j] for r in v], np.int64) for j in range(4)) for k, v in recs.items()}


def host_tables(rec, n: int):
    tabs = [(np.zeros(n, np.int64), np.zeros(n, np.int64)) for _ in range(2)]
    pos, strand, cov, mod = rec
    for s in range(2):
        sel = strand == s
        tabs[s][0][pos[sel]] = cov[sel]
        tabs[s][1][pos[sel]] = mod[sel]
    return tabs


# ---- the command case -------------------------------------------------------------------------------------------------------------------------

def _line(chrom, p, strand, cov, mod):
    return ' '.join([chrom, str(p), str(p + 1), BASE, str(min(cov, 1000)), strand, str(p), str(p + 1), '0,0,0', str(cov), str(100 * mod // max(cov, 1)), str(mod), '\n'])


def case_sites():
    """{(contig, pos, strand): ((cov, mod) of sample run1, of sample run2, of control c1, of control c2), planted} from seed 11."""
    rng = np.random.default_rng(11)
    sites = {}
    for name, length, n_sites, n_planted in (('chrA', 2600, 420, 32), ('chrB', 700, 110, 8)):
        pos = np.sort(rng.choice(np.arange(1, length - 150), n_sites, replace=False))
        planted = set(rng.choice(pos, n_planted, replace=False).tolist())
        for p in pos.tolist():
            strand = '+-'[int(rng.integers(0, 2))]
            is_planted = p in planted
            rate = rng.choice([0.0, 0.05, 0.3, 0.7, 0.95])
            covs = [int(rng.integers(25, 40) if is_planted else rng.integers(8, 40)) for _ in range(4)]
            kind = rng.random()
            if kind < 0.05:
                covs[0], covs[1] = 1, 2                               # shallow in the sample
            elif kind < 0.10:
                covs[2], covs[3] = 2, 0                               # shallow in the controls
            runs = []
            for j, c in enumerate(covs):
                r = (0.8 if (j < 2) != (p % 4 == 0) else 0.1) if is_planted else rate       # (a planted site at a multiple of 4: the other way round)
                runs.append((c, int(rng.binomial(c, r))))
            sites[(name, p, strand)] = (tuple(runs), is_planted)
    name, p, strand, a, b = DELTA_SITE
    sites[(name, p, strand)] = ((a, (0, 0), b, (0, 0)), False)
    return sites


def pooled(runs):
    return (runs[0][0] + runs[1][0], runs[0][1] + runs[1][1], runs[2][0] + runs[3][0], runs[2][1] + runs[3][1])


def write_case(root: str) -> dict:
    """Writes sample/run1, sample/run2, c1/run1 and c2/run1 below root -> {'predFolder', 'control': [..], 'sites': case_sites()}."""
    sites = case_sites()
    texts = {}
    for (name, p, strand), (runs, _) in sorted(sites.items()):
        for j, (folder, run) in enumerate((('sample', 'run1'), ('sample', 'run2'), ('c1', 'run1'), ('c2', 'run1'))):
            cov, mod = runs[j]
            if cov:
                texts.setdefault((folder, run, name, strand), []).append(_line(name, p, strand, cov, mod))
    for (folder, run, name, strand), lines in texts.items():
        text = ''.join(lines)
        if (folder, name, strand) == ('c2', 'chrB', '-'):
            text = text.replace('\n', '\r\n')                          # outside the device grammar: parsed on the host
        path = os.path.join(root, folder, run)
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, 'mod_pos.%s%s.%s.bed' % (name, strand, BASE)), 'w', newline='') as fh:
            fh.write(text)
    return {'predFolder': os.path.join(root, 'sample'), 'control': [os.path.join(root, 'c1'), os.path.join(root, 'c2')], 'sites': sites}


def run_command(case: dict, root: str, engine, fileid: str, **options) -> dict:
    """The command on the case under `engine` -> {'txt': the report, 'json': the document as written, root replaced by <root> and `times` dropped}."""
    import json
    from deepmod_amd import diffmod
    out = os.path.join(root, 'out')
    mo = dict({'predFolder': case['predFolder'], 'control': case['control'], 'Base': BASE, 'outFolder': out, 'FileID': fileid, 'cov': COV, 'fdr': FDR, 'threads': 2}, **options)
    diffmod.diffmod(mo, engine=engine)
    with open(os.path.join(out, fileid + '_diffmod.txt')) as fh:
        txt = fh.read()
    with open(os.path.join(out, fileid + '_diffmod.json')) as fh:
        doc = json.loads(fh.read().replace(root, '<root>'))
    doc.pop('times')
    return {'txt': txt, 'json': doc}


def parse_report(txt: str):
    """-> [(chr, pos, strand, covA, modA, pctA, covB, modB, pctB, delta text, p, q)]"""
    rows = []
    for ln in txt.splitlines()[1:]:
        f = ln.split('\t')
        rows.append((f[0], int(f[1]), f[2]) + tuple(int(v) for v in f[3:9]) + (f[9], float(f[10]), float(f[11])))
    return rows
