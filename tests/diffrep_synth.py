"""TEST INFRASTRUCTURE - not part of the product.  The cases of `diffmod --replicates 1` that tests/test_diffrep_host.py (RepHostEngine and the
compiled host twin), tests/test_gpu_diffrep.py (the device) and tests/golden/make_golden_diffrep.py share.

A key here is (c, m): the coverages and the modified counts of its KA + KB replicates as the tables hold them, sample replicates first.

The criterion (derived, not measured on any engine under test).  D* and phi* are the oracle's (diffmod.rep_exact, 50 digits), P(D) is
the oracle's p as a function of D at phi*, E = KAPPA 2^-53 C with C the summed coverage of the used replicates:
    P(D* + E) (1 - RHO) <= p <= P(max(0, D* - E)) (1 + RHO),        |phi - phi*| <= RHO phi*,        p == 1.0 and phi == 1.0 under the integer rule.
KAPPA = 18: the first-order bound of the three-h formula with a logarithm of 1 ulp (above the 16 a half-ulp logarithm would give: the device's log is
documented at 1 ulp, and the bound charges it on each of six terms of size up to C ln 2).  RHO = 2.5e-11: the series of at most 90 terms and the
front factor, 440 roundings, magnified by (1 - p) / p <= 456 where p = 1 - q is formed above x = 1/2.  No key is dropped.

planted_keys(KA, KB, a, b) plants, for least replicate counts (a, b): equal proportions by the integer rule (with replicates that differ); p_A = 0
against p_B = 1; one group at 0 or at 1 only; X2 / nu below 1 and far above 1; a replicate at cov - 1 and a replicate absent (dropped: nu changes, or
the key is shallow when a, b leave no room); nA = a - 1; nB = b - 1; C exactly 2^20 and 2^20 + 1; counts stored with m > c and with m < 0; no
replicate at all.

The synthetic command case (write_case): two contigs, chrA of 2,600 positions with files for both strands and chrB of 700; three sample replicates
s1..s3 and two control replicates c1, c2 of one run each (s2 of two runs on chrA: a replicate may be several runs), as mod_pos BED files.  Per site all
replicates are drawn from one rate, except 40 planted sites of 150 to 250 reads per replicate (80 % in every sample replicate, 10 % in every
control; the other way round at a multiple of 4: at nu = 3 a call takes depth) and 30 disagreeing sites, where one sample replicate sits at 90 %
and everything else at 10 %: the pooled Fisher test calls them, the replicates do not bear it out.  A few sites are shallow in one replicate, one
control file has \\r\\n line ends (parsed on the host), and DELTA_SITE sits exactly on --minDelta 10."""
import functools
import os
from decimal import Decimal

import numpy as np

BASE = 'C'
COV = 5
FDR = 0.05
KAPPA = 18
RHO = 2.5e-11
MAX_TOTAL = 1 << 20
SHAPES = ((1, 2), (2, 1), (2, 2), (3, 5), (8, 8))
DELTA_SITE = ('chrA', 2500, '+', ((10000, 3000), (5000, 1500), (5000, 1500)), ((10000, 2000), (10000, 2000)))      # 30 % against 20 %: exactly 10 points


def low_min_reps(KA: int, KB: int):
    """Least replicate counts one below the default where the rule a + b >= 3 leaves room."""
    a, b = max(KA - 1, 1), max(KB - 1, 1)
    while a + b < 3:
        if b < KB:
            b += 1
        else:
            a += 1
    return a, b


def _spread(total: int, parts: int):
    """total in `parts` near-equal positive parts."""
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


def planted_keys(KA: int, KB: int, a: int, b: int):
    K = KA + KB
    A, B = range(KA), range(KA, K)

    def key(c, m):
        return tuple(int(v) for v in c), tuple(int(v) for v in m)

    def both(ca, ma, cb, mb):
        return key([ca] * KA + [cb] * KB, [ma] * KA + [mb] * KB)

    keys = [both(10, 3, 20, 6)]                                                            # equal by the integer rule, every replicate alike
    c = [12 + 2 * i for i in range(K)]
    keys.append(key(c, [v // 2 for v in c]))                                               # equal, every replicate at one half of another coverage
    if KA > 1:
        c, m = [20] * K, [5] * K
        m[0], m[1] = 2, 8                                                                  # equal group proportions from replicates that differ
        keys.append(key(c, m))
    keys.append(both(300, 0, 250, 250))                                                    # p_A = 0 against p_B = 1 (deep: below 0.05 at nu = 1 too)
    keys.append(both(250, 250, 300, 0))
    keys.append(key([30] * K, [0] * KA + [3 + 2 * j for j in range(KB)]))                  # one group at 0 only
    keys.append(key([30] * K, [30] * KA + [20 - j for j in range(KB)]))                    # one group at 1 only
    keys.append(key([30] * K, [4 + j for j in range(KA)] + [30] * KB))
    keys.append(key([100] * K, [30 + (i % 2) for i in A] + [60 + (i % 2) for i in B]))     # X2 / nu below 1
    keys.append(key([100] * K, [5 if i % 2 else 95 for i in range(K)]))                    # and far above 1
    keys.append(key([400] * K, [40 + 90 * (i % 3) for i in A] + [300 - 100 * (i % 2) for i in B]))
    for drop in (0, K - 1):                                                                # a replicate at cov - 1, a replicate absent
        for left in (COV - 1, 0):
            c, m = [40] * K, [10] * KA + [25] * KB
            c[drop], m[drop] = left, min(left, 2)
            keys.append(key(c, m))
    c, m = [40] * K, [10] * KA + [25] * KB                                                 # nA = a - 1
    for i in range(KA - a + 1):
        c[i], m[i] = COV - 1, 1
    keys.append(key(c, m))
    c, m = [40] * K, [10] * KA + [25] * KB                                                 # nB = b - 1
    for j in range(KB - b + 1):
        c[KA + j], m[KA + j] = (COV - 1, 1) if j % 2 else (0, 0)
    keys.append(key(c, m))
    for total in (MAX_TOTAL, MAX_TOTAL + 1):                                               # C exactly 2^20, and one above: too_deep
        c = _spread(total // 2, KA) + _spread(total - total // 2, KB)
        keys.append(key(c, [v // 3 for v in c[:KA]] + [v // 3 + 40 for v in c[KA:]]))
    c = _spread(MAX_TOTAL - 60, KA) + _spread(60, KB)                                      # deep and lopsided, D small
    keys.append(key(c, [v // 10 for v in c[:KA]] + [v // 10 + 1 for v in c[KA:]]))
    keys.append(key([2 ** 31 - 1] * K, [7] * K))                                           # far above: the sum is formed in 64 bits
    keys.append(key([20] * K, [35] * KA + [-4] * KB))                                      # stored with m > c and m < 0: held to 20 and 0
    keys.append(key([20] * K, [25 if i % 2 else 6 for i in range(K)]))
    keys.append(key([0] * K, [0] * K))                                                     # no replicate at all: ignored
    keys.append(key([0] * (K - 1) + [2], [0] * K))                                         # one shallow replicate alone
    return keys


def random_keys(KA: int, KB: int, seed: int, n: int, max_cov: int = 300):
    rng = np.random.default_rng(seed)
    keys = []
    for _ in range(n):
        c = rng.integers(1, max_cov + 1, KA + KB)
        rate = rng.random()
        other = rate if rng.random() < 0.5 else rng.random()
        spread = rng.choice([0.0, 0.05, 0.3])
        r = np.clip(np.array([rate] * KA + [other] * KB) + spread * rng.standard_normal(KA + KB), 0.0, 1.0)
        keys.append((tuple(int(v) for v in c), tuple(int(v) for v in rng.binomial(c, r))))
    return keys


def sweep_keys(KA: int, KB: int, a: int, b: int):
    return planted_keys(KA, KB, a, b) + random_keys(KA, KB, 100 * KA + KB, 10)


def held(key):
    """The key as a table filled from files can hold it: 0 <= m <= c."""
    c, m = key
    return tuple(max(v, 0) for v in c), tuple(min(max(w, 0), max(v, 0)) for v, w in zip(c, m))


def layout(keys, K: int, length: int, tile: int, phase: int):
    """The keys on a contig of `length` positions: on the last and the first position of every tile, at both ends, and spread over the rest; on
    both strands -> per replicate (pos, strand, cov, mod) as int64 arrays, the entries without coverage and without modified count left out."""
    edges = {p for p in [0, length - 1] + [e + d for e in range(tile, length, tile) for d in (-1, 0)] if 0 <= p < length}
    spots = sorted(edges | {int(x) for x in np.linspace(1, max(length - 2, 1), 2 * len(keys))})
    recs = [[] for _ in range(K)]
    inner = 0
    for i, p in enumerate(spots):
        inner += p not in edges
        for s in range(2):
            if p in edges:
                c, m = keys[(i + s) % 4]                              # (the first four planted keys are tested whatever the least counts)
            elif inner > len(keys) and (inner + s + phase) % 3 == 0:
                continue                                              # a position of one strand only
            else:
                c, m = keys[(inner + 5 * s + phase) % len(keys)]      # the first len(keys) inner spots: every key on either strand
            for j in range(K):
                if c[j] or m[j]:
                    recs[j].append((p, s, c[j], m[j]))
    return [tuple(np.array([r[f] for r in v], np.int64) for f in range(4)) for v in recs]


def host_tables(rec, n: int):
    """-> (plus, minus), each (coverage, modified), as plain arrays: any count can be stored."""
    tabs = [(np.zeros(n, np.int64), np.zeros(n, np.int64)) for _ in range(2)]
    pos, strand, cov, mod = rec
    for s in range(2):
        sel = strand == s
        tabs[s][0][pos[sel]] = cov[sel]
        tabs[s][1][pos[sel]] = mod[sel]
    return tuple(tabs)


def keys_on_a_line(keys, KA: int):
    """Every key on its own position of the '+' strand -> (sample, control) for the engines."""
    K = len(keys[0][0])
    z = (np.zeros(len(keys), np.int64), np.zeros(len(keys), np.int64))
    reps = [((np.array([k[0][j] for k in keys], np.int64), np.array([k[1][j] for k in keys], np.int64)), z) for j in range(K)]
    return reps[:KA], reps[KA:]


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bounds(used_a: tuple, used_b: tuple):
    """-> (lowest p, highest p, lowest phi, highest phi) a tested key's engine may give, as floats rounded outwards by one part in 10^16."""
    from deepmod_amd import diffmod
    e = diffmod.rep_exact(used_a, used_b)
    if e['equal']:
        return 1.0, 1.0, 1.0, 1.0
    ctx = diffmod._rep_context()
    E = ctx.multiply(Decimal(KAPPA * (e['cA'] + e['cB'])), Decimal(2) ** -53)
    rho, eps = Decimal(RHO), Decimal(10) ** -16
    lo = diffmod.rep_tail(e['nu'], ctx.divide(ctx.add(e['D'], E), e['phi'])) * (1 - rho)
    hi = diffmod.rep_tail(e['nu'], ctx.divide(max(ctx.subtract(e['D'], E), Decimal(0)), e['phi'])) * (1 + rho)
    return float(lo * (1 - eps)), float(hi * (1 + eps)), float(e['phi'] * (1 - rho)), float(e['phi'] * (1 + rho))


def check_key(p: float, phi: float, used_a, used_b, what=None):
    lo, hi, phi_lo, phi_hi = bounds(tuple(map(tuple, used_a)), tuple(map(tuple, used_b)))
    assert lo <= p <= hi, (what, p, lo, hi)
    assert phi_lo <= phi <= phi_hi, (what, phi, phi_lo, phi_hi)


def used_of(key, KA: int, cov: int, a: int, b: int):
    """-> (fate, used sample replicates, used control replicates) of a key."""
    from deepmod_amd import diffmod
    c, m = key
    return diffmod.rep_fate(cov, a, b, c[:KA], m[:KA], c[KA:], m[KA:])


def check_records(rec, tables, KA: int, cov: int, a: int, b: int, what=None):
    """Every record of an engine against the oracle's reading of the tables it was given (tables: per replicate (plus, minus) host tables): the integer
    columns exact, phi and p within the criterion."""
    for i in range(len(rec['p'])):
        q, s = int(rec['pos'][i]), int(rec['strand'][i])
        key = (tuple(int(t[s][0][q]) if q < len(t[s][0]) else 0 for t in tables), tuple(int(t[s][1][q]) if q < len(t[s][1]) else 0 for t in tables))
        f, ua, ub = used_of(key, KA, cov, a, b)
        assert f == 0, (what, q, s, key)
        want = (sum(c for c, _ in ua), sum(m for _, m in ua), sum(c for c, _ in ub), sum(m for _, m in ub), len(ua), len(ub))
        assert tuple(int(rec[k][i]) for k in ('cA', 'mA', 'cB', 'mB', 'nA', 'nB')) == want, (what, q, s, key)
        check_key(float(rec['p'][i]), float(rec['phi'][i]), ua, ub, (what, q, s, key))


# ---- the command case -------------------------------------------------------------------------------------------------------------------------

FOLDERS = ('s1', 's2', 's3', 'c1', 'c2')


def _line(chrom, p, strand, cov, mod):
    return ' '.join([chrom, str(p), str(p + 1), BASE, str(min(cov, 1000)), strand, str(p), str(p + 1), '0,0,0', str(cov), str(100 * mod // max(cov, 1)), str(mod), '\n'])


def case_sites():
    """{(contig, pos, strand): (((cov, mod) of s1, s2, s3), ((cov, mod) of c1, c2), kind)}, kind one of 'null', 'planted', 'disagree', 'delta', from
    seed 12."""
    rng = np.random.default_rng(12)
    sites = {}
    for name, length, n_sites, n_planted, n_disagree in (('chrA', 2600, 420, 32, 24), ('chrB', 700, 110, 8, 6)):
        pos = np.sort(rng.choice(np.arange(1, length - 150), n_sites, replace=False))
        special = rng.choice(pos, n_planted + n_disagree, replace=False).tolist()
        planted, disagree = set(special[:n_planted]), set(special[n_planted:])
        for p in pos.tolist():
            strand = '+-'[int(rng.integers(0, 2))]
            kind = 'planted' if p in planted else 'disagree' if p in disagree else 'null'
            rate = rng.choice([0.0, 0.05, 0.3, 0.7, 0.95])
            covs = [int(rng.integers(150, 250) if kind == 'planted' else rng.integers(25, 40) if kind == 'disagree' else rng.integers(8, 40)) for _ in range(5)]
            shallow = rng.random()
            if kind == 'null' and shallow < 0.05:
                covs[int(rng.integers(0, 3))] = int(rng.integers(0, COV))                  # one sample replicate shallow or absent
            elif kind == 'null' and shallow < 0.10:
                covs[3 + int(rng.integers(0, 2))] = int(rng.integers(0, COV))              # one control replicate
            runs = []
            for j, c in enumerate(covs):
                if kind == 'planted':
                    r = 0.8 if (j < 3) != (p % 4 == 0) else 0.1                            # (at a multiple of 4: the other way round)
                elif kind == 'disagree':
                    r = 0.9 if j == p % 3 else 0.1                                         # one sample replicate against everything else
                else:
                    r = rate
                runs.append((c, int(rng.binomial(c, r))))
            sites[(name, p, strand)] = (tuple(runs[:3]), tuple(runs[3:]), kind)
    name, p, strand, a, b = DELTA_SITE
    sites[(name, p, strand)] = (a, b, 'delta')
    return sites


def pooled(site):
    sample, control = site[0], site[1]
    return (sum(c for c, _ in sample), sum(m for _, m in sample), sum(c for c, _ in control), sum(m for _, m in control))


def write_case(root: str) -> dict:
    """Writes s1/run1, s2/run1 (s2/run2 holds every second site of chrA instead), s3/run1, c1/run1 and c2/run1 below root -> {'predFolder': [..],
    'control': [..], 'sites': case_sites()}."""
    sites = case_sites()
    texts = {}
    for n, ((name, p, strand), (sample, control, _)) in enumerate(sorted(sites.items())):
        for j, folder in enumerate(FOLDERS):
            cov, mod = (sample + control)[j]
            run = 'run2' if folder == 's2' and name == 'chrA' and n % 2 else 'run1'
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
    return {'predFolder': [os.path.join(root, f) for f in FOLDERS[:3]], 'control': [os.path.join(root, f) for f in FOLDERS[3:]], 'sites': sites}


def run_command(case: dict, root: str, engine, fileid: str, **options) -> dict:
    """The command on the case under `engine` -> {'txt': the report, 'json': the document as written, root replaced by <root> and `times` dropped}."""
    import json
    from deepmod_amd import diffmod
    out = os.path.join(root, 'out')
    mo = dict({'predFolder': case['predFolder'], 'control': case['control'], 'Base': BASE, 'outFolder': out, 'FileID': fileid, 'cov': COV, 'fdr': FDR, 'threads': 2,
               'replicates': 1}, **options)
    diffmod.diffmod(mo, engine=engine)
    with open(os.path.join(out, fileid + '_diffmod.txt')) as fh:
        txt = fh.read()
    with open(os.path.join(out, fileid + '_diffmod.json')) as fh:
        doc = json.loads(fh.read().replace(root, '<root>'))
    doc.pop('times')
    return {'txt': txt, 'json': doc}


def parse_report(txt: str):
    """-> [(chr, pos, strand, covA, modA, pctA, covB, modB, pctB, delta text, repA, repB, phi, p, q)]"""
    rows = []
    for ln in txt.splitlines()[1:]:
        f = ln.split('\t')
        rows.append((f[0], int(f[1]), f[2]) + tuple(int(v) for v in f[3:9]) + (f[9], int(f[10]), int(f[11]), float(f[12]), float(f[13]), float(f[14])))
    return rows
