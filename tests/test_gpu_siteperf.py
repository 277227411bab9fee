"""GPU: the kernels of `siteperf` (csrc/siteperf.hip.inc) against the numpy statement of the semantics (deepmod_amd/siteperf.py, HostEngine) - integers,
compared with == - and the command against the lines the reference's own tool printed (tests/golden/siteperf_cases.json)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import long_cases
from conftest import ROOT
from deepmod_amd import siteperf as sp
from test_siteperf_host import CASES, golden_lines, write_case

pytestmark = pytest.mark.gpu

FIELDS = ("hist", "counts", "lines_seen", "lines_skipped", "base_mismatch")


def random_seq(rng, n, motif=None, every=20):
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    if motif is not None:
        pat = np.frombuffer(motif.upper().encode(), np.uint8)
        p = int(rng.integers(0, every))
        while p + len(pat) <= n:
            seq[p:p + len(pat)] = pat
            p += len(pat) + int(rng.integers(1, every))
    return seq.astype(np.uint8)


def same(a, b):
    for key in FIELDS:
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("motif,k", [("CG", 0), ("GATC", 1), ("GAATTC", 2), ("TCGA", 3), ("A", 0)])
def test_site_codes_equal_the_twin(gpu_device, motif, k):
    rng = np.random.default_rng(len(motif) * 10 + k)
    dev = sp.DeviceEngine((1, 5), gpu_device)
    try:
        for n in (1, 5, 1023, 1024, 1025, 4097):
            seq = random_seq(rng, n, motif)
            pat = np.frombuffer(motif.encode(), np.uint8)
            if n > 2 * len(pat):                                     # the motif cut by both ends: its tail first, its head last
                seq[:len(pat) - 1] = pat[1:]
                seq[n - (len(pat) - 1):] = pat[:-1]
            site = np.nonzero(sp.site_codes(seq, motif, k))[0]
            mid = int(site[len(site) // 2]) if len(site) else n // 2
            for start, end in ((None, None), (mid, mid), (0, n // 2), (n // 3, n - 1), (0, n - 1), (mid + 1, mid + 3)):
                dev.set_contig(seq, motif, k, start, end)
                got = dev.codes()
                assert got.shape == (n,) and np.array_equal(got, sp.site_codes(seq, motif, k, start, end)), (n, start, end)
    finally:
        dev.close()


def make_line(rng, name, n_pos, sep=b"\t", wide=False):
    cov = int(rng.integers(0, 40))
    mod = int(rng.integers(0, cov + 1))
    pct = int(mod * 100 / cov) if cov else 0
    pos = int(rng.integers(0, n_pos))
    num = (lambda v: b"%010d" % v) if wide else (lambda v: b"%d" % v)
    f = [name, num(pos), b"%d" % (pos + 1), bytes([int(rng.choice(np.frombuffer(b"ACGTN", np.uint8)))]), b"%d" % min(cov, 1000), b"+" if rng.random() < 0.5 else b"-",
         b"%d" % pos, b"%d" % (pos + 1), b"0,0,0", num(cov), num(pct), num(mod)]
    return sep.join(f)


def make_text(rng, name, n_pos, size, newline_at_end=True, wide=False):
    """Exactly `size` bytes of lines: the last line takes a thirteenth field of the length that is missing."""
    lines, used = [], 0
    while True:
        ln = make_line(rng, name, n_pos, b"\t" if len(lines) % 2 else b" ", wide)
        if used + len(ln) + 1 + 140 > size:
            break
        lines.append(ln)
        used += len(ln) + 1
    ln = make_line(rng, name, n_pos)
    fill = size - used - len(ln) - (1 if newline_at_end else 0) - 1
    assert fill >= 1
    lines.append(ln + b"\t" + b"x" * fill)
    text = b"\n".join(lines) + (b"\n" if newline_at_end else b"")
    assert len(text) == size
    return text


def test_parser_equals_the_host_parser(gpu_device):
    tile = sp.tile_bytes()
    assert tile >= 1024
    rng = np.random.default_rng(7)
    n = 4097
    seq = random_seq(rng, n, "CG")
    texts = [make_text(rng, b"ctgA", n, size) for size in (tile - 1, tile, tile + 1, 3 * tile + 27)]
    texts.append(make_text(rng, b"ctgA", n, 2 * tile + 5, newline_at_end=False))
    texts.append(make_text(rng, b"ctgA", n, tile + 300, wide=True))
    wide = b"ctgA 0000000007 8 C 1000 + 7 8 0,0,0 2147483647 0100 2147483647\n"
    texts.append(wide * 3)
    # every tile boundary is straddled by a line: no newline directly before a boundary
    for t in texts:
        assert all(t[b - 1:b] != b"\n" for b in range(tile, len(t), tile))
    dev, host = sp.DeviceEngine((1, 5, 10), gpu_device), sp.HostEngine((1, 5, 10))
    try:
        dev.set_contig(seq, "Cg", 0)
        host.set_contig(seq, "Cg", 0)
        for t in texts:
            want = sp.parse_bed_host(t, "t")["ctgA"]
            rows, flag, bad = dev.add_text(t, sp.RUN, "ctgA")
            assert (rows, flag, bad) == (len(want[0]), 0, -1)
            got = dev.records()
            twin, tflag, _ = sp.parse_device_grammar(t, "ctgA", n)
            assert tflag == 0
            for g, w, tw in zip(got, want, twin):
                assert np.array_equal(g, w) and np.array_equal(tw, w)
            host.add_records(sp.RUN, *want[:6])
        dev.finish_contig()
        host.finish_contig()
        same(dev.fetch(), host.fetch())
        parse_ms, count_ms = dev.times()
        assert parse_ms > 0.0 and count_ms > 0.0
    finally:
        dev.close()


GOOD = b"c1\t5\t6\tC\t7\t+\t5\t6\t0,0,0\t7\t42\t3\n"
VIOLATIONS = {
    "carriage return": GOOD.replace(b"\n", b"\r\n"),
    "empty line": b"\n",
    "two separators": GOOD.replace(b"\tC\t", b"\t\tC\t"),
    "another contig": GOOD.replace(b"c1", b"c2"),
    "a sign": GOOD.replace(b"\t42\t", b"\t+42\t"),
    "percentage above 100": GOOD.replace(b"\t42\t", b"\t101\t"),
    "position off the contig": GOOD.replace(b"\t5\t6\tC", b"\t5000\t5001\tC"),
    "strand": GOOD.replace(b"\t+\t", b"\t.\t"),
    "a base of two bytes": GOOD.replace(b"\tC\t", b"\tCC\t"),
    "eleven fields": b"\t".join(GOOD.split(b"\t")[:11]) + b"\n",
    "eleven digits": GOOD.replace(b"\t7\t42", b"\t12345678901\t42"),
    "above 2^31 - 1": GOOD.replace(b"\t7\t42", b"\t2147483648\t42"),
}


@pytest.mark.parametrize("what", sorted(VIOLATIONS))
def test_grammar_violation_is_flagged_with_its_line(gpu_device, what):
    tile = sp.tile_bytes()
    before = tile // len(GOOD) + 40                                   # the bad line lies in the second tile
    text = GOOD * before + VIOLATIONS[what] + GOOD * 30
    dev = sp.DeviceEngine((1, 5), gpu_device)
    try:
        dev.set_contig(random_seq(np.random.default_rng(1), 4097, "CG"), "Cg", 0)
        for role in (sp.RUN, sp.CONTROL):
            rows, flag, bad = dev.add_text(text, role, "c1")
            assert (flag, bad) == (1, before + 1)
            assert sp.parse_device_grammar(text, "c1", 4097)[1:] == (1, before + 1)
        dev.finish_contig()
        got = dev.fetch()
        assert got["hist"].sum() == 0 and got["counts"].sum() == 0 and got["lines_seen"] == 0      # a flagged text is not counted
    finally:
        dev.close()


def test_command_takes_the_host_path_for_a_text_outside_the_grammar(gpu_device, tmp_path):
    case = CASES["empty_class"]
    other = dict(case, run={rel: t.replace(" ", "  ") for rel, t in case["run"].items()},
                 controls=[{rel: t.replace("\n", " \r\n") for rel, t in files.items()} for files in case["controls"]])
    mo = write_case(other, str(tmp_path))
    doc = sp.siteperf(mo)
    assert doc["lines"] == golden_lines(case, mo["outFolder"])
    assert len(doc["notes"]) == 2 and all("line 1 is outside the device grammar" in n for n in doc["notes"])
    twin = sp.siteperf(write_case(case, str(tmp_path / "twin")), engine=sp.HostEngine((1, 5)))
    assert doc["histogram"]["counts"] == twin["histogram"]["counts"] and doc["read_level"] == twin["read_level"]


def random_records(rng, n, n_pos, bases=b"CCCCCCGA", max_cov=30):
    cov = rng.integers(0, max_cov + 1, n)
    mod = (cov * rng.random(n)).astype(np.int64)
    pct = np.where(cov > 0, (100 * mod) // np.maximum(cov, 1), 0)
    return (rng.integers(0, n_pos, n), rng.integers(0, 2, n), rng.choice(np.frombuffer(bases, np.uint8), n), cov, pct, mod)


def run_both(gpu_device, thresholds, seq, motif, k, region, batches):
    dev, host = sp.DeviceEngine(thresholds, gpu_device), sp.HostEngine(thresholds)
    try:
        for e in (dev, host):
            e.set_contig(seq, motif, k, *region)
            for role, rec in batches:
                e.add_records(role, *rec)
            e.finish_contig()
        got, want = dev.fetch(), host.fetch()
        same(got, want)
        return got
    finally:
        dev.close()


@pytest.fixture(scope="module")
def mixed_input():
    rng = np.random.default_rng(42)
    seq = random_seq(rng, 4097, "CG", 12)
    batches = [(sp.RUN, random_records(rng, 30000, 4097)), (sp.CONTROL, random_records(rng, 10000, 4097)), (sp.CONTROL, random_records(rng, 10000, 4097))]
    return seq, batches


def test_histograms_of_random_records(gpu_device, mixed_input):
    seq, batches = mixed_input
    got = run_both(gpu_device, (1, 5, 10), seq, "Cg", 0, (None, None), batches)
    assert got["lines_seen"] == 50000 and got["hist"].sum() > 30000 and (got["hist"].sum(axis=(1, 2, 3)) > 0).all()
    got = run_both(gpu_device, (1, 5, 10), seq, "Cg", 0, (1000, 3000), batches)
    assert got["lines_skipped"] > 20000


def test_every_capped_grid_takes_a_second_pass(gpu_device):
    """150,001 bases, a RUN and a CONTROL batch of 300,000 records each and a second CONTROL batch (long_cases.siteperf_case): sp_count_kernel and
    sp_scatter_kernel loop over more records than their grid has threads, sp_walk_kernel over the 2 x len elements of the control table."""
    grid = 1024 * 256                                                 # spk::MAX_BLOCKS x spk::THREADS
    seq, batches = long_cases.siteperf_case()
    assert 2 * len(seq) > grid and len(batches[0][1][0]) > grid and len(batches[1][1][0]) > grid and [role for role, _ in batches] == [sp.RUN, sp.CONTROL, sp.CONTROL]
    for role, rec in batches[:2]:                                     # records and control sites on both sides of element `grid` of 2 x len
        e = 2 * rec[0] + rec[1]
        assert (e < grid).sum() > 1000 and (e >= grid).sum() > 1000
    got = run_both(gpu_device, (1, 5, 10), seq, "Cg", 0, (None, None), batches)
    assert got["lines_seen"] == sum(len(rec[0]) for _, rec in batches) == 620000 and (got["hist"].sum(axis=(1, 2, 3)) > 0).all()
    assert got["hist"].sum() > 400000                                 # the run's entries and the controls' sites


def test_contention_on_one_bin(gpu_device):
    seq = random_seq(np.random.default_rng(3), 4097, "CG", 12)
    site = int(np.nonzero(sp.site_codes(seq, "Cg", 0) & 1)[0][5])
    n = 200000
    rec = (np.full(n, site), np.zeros(n), np.full(n, ord("C")), np.full(n, 7), np.full(n, 57), np.full(n, 4))
    got = run_both(gpu_device, (1, 5), seq, "Cg", 0, (None, None), [(sp.RUN, rec)])
    assert got["hist"][0, 1, 1, 57] == n and got["hist"].sum() == n
    assert list(got["counts"]) == [4 * n, 0, 0, 3 * n]


def test_every_percentage_and_every_threshold_edge(gpu_device):
    seq = random_seq(np.random.default_rng(4), 1025, "CG", 12)
    pct = np.arange(101)
    sites = np.nonzero(sp.site_codes(seq, "Cg", 0) & 1)[0]
    pos = sites[pct % len(sites)]
    every = (pos, np.zeros(101), np.full(101, ord("C")), np.full(101, 100), pct, pct)
    got = run_both(gpu_device, (1, 5), seq, "Cg", 0, (None, None), [(sp.RUN, every), (sp.CONTROL, (np.arange(101) + 200, np.ones(101), np.full(101, ord("C")), np.full(101, 100), pct, pct))])
    assert (got["hist"][0, 1].sum(axis=0) == 1).all()                  # every percentage once among the run's site entries
    assert (got["hist"][:, 0].sum(axis=(0, 1)) == 1).all()             # and once among the control's
    thresholds = (2, 3, 5, 8, 13, 21, 34, 55)
    cov = np.array(sorted({max(t + d, 0) for t in thresholds for d in (-1, 0, 1)} | {0}))
    n = len(cov)
    rec = (np.arange(n) + 10, np.arange(n) % 2, np.full(n, ord("C")), cov, np.zeros(n), np.zeros(n))
    got = run_both(gpu_device, thresholds, seq, "Cg", 0, (None, None), [(sp.RUN, rec), (sp.CONTROL, rec)])
    per_bucket = got["hist"].sum(axis=(0, 1, 3))
    want = [int(((cov >= t) & (cov < (thresholds[j + 1] if j + 1 < len(thresholds) else 10 ** 9))).sum()) * 2 for j, t in enumerate(thresholds)]
    assert per_bucket.tolist() == want


def test_one_control_site_in_three_files(gpu_device):
    seq = np.frombuffer(b"AACGAAAAAAAAAAAAAAAA", np.uint8)
    one = lambda base, cov, mod: ([4], [0], [ord(base)], [cov], [int(mod * 100 / cov)], [mod])      # next to the '+' site at 2, seen at offset -2
    got = run_both(gpu_device, (1, 5), seq, "Cg", 0, (None, None), [(sp.CONTROL, one("A", 2, 1)), (sp.CONTROL, one("C", 1, 1)), (sp.CONTROL, one("C", 2, 1))])
    assert got["hist"].sum() == 1 and got["hist"][5, 0, 1, 60] == 1    # the first file's base (not B): M_nb; coverage 5, int(3 * 100 / 5)
    got = run_both(gpu_device, (1, 5), seq, "Cg", 0, (None, None), [(sp.CONTROL, one("C", 2, 1)), (sp.CONTROL, one("A", 1, 1)), (sp.CONTROL, one("A", 2, 1))])
    assert got["hist"].sum() == 1 and got["hist"][2, 0, 1, 60] == 1    # M_n2B
    # within one file the first line decides
    two = ([4, 4, 4], [0, 0, 0], [ord("A"), ord("C"), ord("C")], [1, 1, 1], [0, 0, 0], [0, 0, 0])
    got = run_both(gpu_device, (1, 5), seq, "Cg", 0, (None, None), [(sp.CONTROL, two)])
    assert got["hist"][5, 0, 0, 0] == 1


def test_two_runs_give_the_same_bytes(gpu_device, mixed_input):
    seq, batches = mixed_input
    out = []
    for _ in range(2):
        dev = sp.DeviceEngine((1, 5, 10), gpu_device)
        try:
            dev.set_contig(seq, "Cg", 0)
            for role, rec in batches:
                dev.add_records(role, *rec)
            dev.finish_contig()
            got = dev.fetch()
            out.append(b"".join(np.asarray(got[key]).tobytes() for key in FIELDS))
        finally:
            dev.close()
    assert out[0] == out[1]


def test_records_outside_the_contig_are_refused_before_a_launch(gpu_device):
    from deepmod_amd import _lib
    dev = sp.DeviceEngine((1, 5), gpu_device)
    try:
        dev.set_contig(b"ACGTACGT", "Cg", 0)
        for rec in (([8], [0], [67], [1], [0], [0]), ([-1], [0], [67], [1], [0], [0]), ([1], [2], [67], [1], [0], [0]), ([1], [0], [67], [1], [101], [0]), ([1], [0], [67], [1], [0], [2])):
            with pytest.raises(_lib.DeepModHipError, match="record 0"):
                dev.add_records(sp.RUN, *rec)
        assert dev.fetch()["hist"].sum() == 0
    finally:
        dev.close()


def deepmod_cli():
    spec = importlib.util.spec_from_file_location("_deepmod_cli", os.path.join(ROOT, "bin", "DeepMod.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", ["cg", "gatc", "region", "empty_class"])
def test_command_writes_the_reference_lines(gpu_device, name, tmp_path):
    case = CASES[name]
    mo = write_case(case, str(tmp_path))
    argv = ["siteperf", "--predFolder", mo["predFolder"], "--control", ",".join(mo["control"]), "--Ref", mo["Ref"], "--motif", case["motif"], "--ModinMotif", str(case["k"]),
            "--outFolder", mo["outFolder"], "--FileID", "g", "--threads", "2"]
    if case["chr"]:
        argv += ["--chr", case["chr"], "--start", str(case["start"]), "--end", str(case["end"])]
    cli = deepmod_cli()
    args = cli.build_parser().parse_args(argv)
    args.func(args)
    with open(os.path.join(mo["outFolder"], "g_siteperf.txt"), newline="") as fh:
        assert fh.read() == "".join(ln + "\n" for ln in golden_lines(case, mo["outFolder"]))
    with open(os.path.join(mo["outFolder"], "g_siteperf.json")) as fh:
        doc = json.load(fh)
    twin = sp.siteperf(write_case(case, str(tmp_path / "twin")), engine=sp.HostEngine((1, 5)))
    assert doc["histogram"]["counts"] == twin["histogram"]["counts"] and doc["read_level"] == twin["read_level"]
    assert doc["base_mismatch_lines"] == twin["base_mismatch_lines"] and doc["lines_outside_region"] == twin["lines_outside_region"]
    assert doc["notes"] == []                                         # every file went through the device parser


def test_shim_gives_the_same_file(gpu_device, tmp_path):
    case = CASES["region"]
    mo = write_case(case, str(tmp_path))
    fig = str(tmp_path / "figs")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "DeepMod_tools", "cal_EcoliDetPerf.py"), mo["predFolder"], mo["Ref"], case["motif"], str(case["k"]), case["chr"],
                          str(case["start"]), str(case["end"]), fig, ",".join(mo["control"])], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    want = golden_lines(case, fig)
    with open(os.path.join(fig, "cal_EcoliDetPerf_siteperf.txt")) as fh:
        assert fh.read().splitlines() == want
    assert out.stdout.splitlines()[-len(want):] == want
