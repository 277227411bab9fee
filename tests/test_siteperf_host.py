"""CPU: the numpy statement of `siteperf` (deepmod_amd/siteperf.py, HostEngine) against the lines the reference's own cal_EcoliDetPerf.py printed
(tests/golden/siteperf_cases.json, made by tests/golden/make_golden_siteperf.py), the category rule at its edges, the command's refusals, the
shim's argument mapping, and the line routine under the address sanitizer (tests/siteperf_asan_driver.cpp)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import siteperf as sp

GOLDEN = os.path.join(ROOT, "tests", "golden", "siteperf_cases.json")


def load_cases():
    with open(GOLDEN) as fh:
        return {c["name"]: c for c in json.load(fh)["cases"]}


CASES = load_cases()


def write_case(case, root):
    """The case's files under root -> the options of siteperf.siteperf()."""
    def tree(folder, files):
        for rel, content in files.items():
            path = os.path.join(folder, rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(content)
    tree(os.path.join(root, "run"), case["run"])
    controls = []
    for i, files in enumerate(case["controls"]):
        controls.append(os.path.join(root, "control%d" % i))
        tree(controls[-1], files)
    with open(os.path.join(root, "ref.fa"), "w") as fh:
        fh.write(case["fasta"])
    return {"predFolder": os.path.join(root, "run"), "control": controls, "Ref": os.path.join(root, "ref.fa"), "motif": case["motif"], "ModinMotif": case["k"],
            "chr": case["chr"] or None, "start": case["start"], "end": case["end"], "cov": (1, 5), "outFolder": os.path.join(root, "out"), "FileID": "t", "threads": 2}


def golden_lines(case, out_folder):
    return [ln.replace("{FIG}", out_folder) for ln in case["lines"]]


@pytest.mark.parametrize("name", ["cg", "gatc", "region", "empty_class"])
def test_twin_prints_the_reference_lines(name, tmp_path):
    case = CASES[name]
    mo = write_case(case, str(tmp_path))
    doc = sp.siteperf(mo, engine=sp.HostEngine((1, 5)))
    assert doc["lines"] == golden_lines(case, mo["outFolder"])
    with open(os.path.join(mo["outFolder"], "t_siteperf.txt")) as fh:
        assert fh.read().splitlines() == golden_lines(case, mo["outFolder"])
    with open(os.path.join(mo["outFolder"], "t_siteperf.json")) as fh:
        stored = json.load(fh)
    assert stored["histogram"]["counts"] == doc["histogram"]["counts"]
    assert sum(v["label0"] + v["label1"] for v in stored["categories"].values()) == int(np.sum(doc["histogram"]["counts"]))


def test_empty_class_case_has_no_auc_line_at_5():
    lines = CASES["empty_class"]["lines"]
    assert sum(" 5 0." in ln or " 5 1." in ln for ln in lines if "roc_plot" in ln) == 0
    assert sum("ap_plot" in ln and " 5 ap=" in ln for ln in lines) == 2


def drop_lines_the_reference_loses(text, start, end):
    """The rule of DESIGN.md 16: readmodf_dict reads one more line after every out-of-region line it examines and never looks at it, so the line
    directly after an examined out-of-region line is lost, whatever it holds."""
    kept, skip = [], False
    for line in text.splitlines():
        if skip:
            skip = False
            continue
        kept.append(line)
        pos = int(line.split()[1])
        if not start <= pos <= end:
            skip = True
    return "".join(ln + "\n" for ln in kept)


def test_departure_case(tmp_path):
    case = CASES["departure"]
    mo = write_case(case, str(tmp_path / "as_is"))
    doc = sp.siteperf(mo, engine=sp.HostEngine((1, 5)))
    assert doc["lines"] != golden_lines(case, mo["outFolder"])                     # this build reads every in-region control line
    lossy = dict(case, controls=[{rel: drop_lines_the_reference_loses(t, case["start"], case["end"]) for rel, t in files.items()} for files in case["controls"]])
    assert lossy["controls"] != case["controls"]
    mo = write_case(lossy, str(tmp_path / "lossy"))
    doc = sp.siteperf(mo, engine=sp.HostEngine((1, 5)))
    assert doc["lines"] == golden_lines(case, mo["outFolder"])


def test_site_codes_follow_the_reference_rule():
    seq = b"ACGCGTTGATCAGAATTCCG"
    for motif, k in (("Cg", 0), ("gAtc", 1), ("gaAttc", 2), ("TCGA", 3), ("A", 0)):
        pat = motif.upper()
        rc = sp.revcomp(pat)
        m = len(pat)
        want = np.zeros(len(seq), np.uint8)
        for i in range(len(seq)):
            if i - k >= 0 and seq[i - k:i - k + m] == pat.encode():
                want[i] |= 1
            j = i - (m - 1 - k)
            if j >= 0 and seq[j:j + m] == rc.encode():
                want[i] |= 2
        assert np.array_equal(sp.site_codes(seq, motif, k), want), motif
        cut = want.copy()
        cut[:3] = 0
        cut[11:] = 0
        assert np.array_equal(sp.site_codes(seq, motif, k, 3, 10), cut), motif


def test_category_first_offset_wins():
    # '+' CpG sites at 2 and 6: position 5 sees -3 (site at 2) before +1 (site at 6) -> n3
    seq = b"AACGAACGAAAAAAAA"
    code = sp.site_codes(seq, "Cg", 0)
    assert list(np.nonzero(code & 1)[0]) == [2, 6]
    is_b = np.array([True])
    assert sp.categories(code, [5], [0], is_b)[0] == 3
    assert sp.categories(code, [5], [0], ~is_b)[0] == 5
    assert sp.categories(code, [4], [0], is_b)[0] == 2                              # -2 before +2
    assert sp.categories(code, [3], [0], is_b)[0] == 1                              # -1 before +3
    assert sp.categories(code, [2], [0], ~is_b)[0] == 0                             # a site is M whatever the line's base
    assert sp.categories(code, [10], [0], is_b)[0] == 4
    assert sp.categories(code, [10], [0], ~is_b)[0] == 6
    assert sp.categories(code, [5], [1], is_b)[0] == 2                              # '-' sites at 3 and 7: -2 before +2


def test_category_at_the_contig_edges():
    seq = b"CGAAAAAAAAACG"                                                          # '+' sites at 0 and 11, '-' sites at 1 and 12
    code = sp.site_codes(seq, "Cg", 0)
    n = len(seq)
    pos = [0, 1, 2, n - 3, n - 2, n - 1]
    t = np.ones(len(pos), bool)
    assert list(sp.categories(code, pos, [0] * 6, t)) == [0, 1, 2, 1, 0, 1]
    assert list(sp.categories(code, pos, [1] * 6, t)) == [1, 0, 1, 2, 1, 0]
    # a neighbour outside start..end is no site
    code = sp.site_codes(seq, "Cg", 0, 1, n - 3)
    assert list(sp.categories(code, pos, [0] * 6, t)) == [4, 4, 4, 4, 4, 4]
    assert list(sp.categories(code, pos, [1] * 6, t)) == [1, 0, 1, 4, 4, 4]


def test_fasta_is_compared_case_sensitively(tmp_path):
    assert not sp.site_codes(b"AAcgAACg", "Cg", 0).any()
    assert list(np.nonzero(sp.site_codes(b"AAcgAACG", "cg", 0))[0]) == [6, 7]
    fa = tmp_path / "x.fa"
    fa.write_text(">a  b c\nACgt\nAC\n>b\nGG\n")
    assert sp.read_fasta(str(fa)) == {"a": b"ACgtAC", "b": b"GG"}
    assert sp.read_fasta(str(fa), "b") == {"b": b"GG"}


def test_control_sums_cross_a_threshold_only_together():
    seq = b"AACGAAAA"
    e = sp.HostEngine((1, 5))
    e.set_contig(seq, "Cg", 0)
    for cov, mod in ((2, 1), (3, 3)):
        e.add_records(sp.CONTROL, [2], [0], [ord("C")], [cov], [int(mod * 100 / cov)], [mod])
    e.finish_contig()
    got = e.fetch()
    assert got["hist"].sum() == 1
    assert got["hist"][0, 0, 1, 80] == 1                                            # one label-0 entry on M: coverage 5, int(4 * 100 / 5)
    assert list(got["counts"]) == [0, 4, 1, 0]
    # the same lines of a run are two entries, neither reaches 5
    e = sp.HostEngine((1, 5))
    e.set_contig(seq, "Cg", 0)
    e.add_records(sp.RUN, [2, 2], [0, 0], [ord("C")] * 2, [2, 3], [50, 100], [1, 3])
    e.finish_contig()
    got = e.fetch()
    assert got["hist"][0, 1, 0, 50] == 1 and got["hist"][0, 1, 0, 100] == 1 and got["hist"].sum() == 2
    assert list(got["counts"]) == [4, 0, 0, 1]


def test_device_grammar_on_the_host(hip_lib):
    good = b"c1\t5\t6\tC\t7\t+\t5\t6\t0,0,0\t7\t42\t3\n"
    rec, flag, bad = sp.parse_device_grammar(good + good.replace(b"\t", b" ").replace(b"+", b"-"), "c1", 10)
    assert (flag, bad) == (0, -1)
    assert [a.tolist() for a in rec] == [[5, 5], [0, 1], [67, 67], [7, 7], [42, 42], [3, 3]]
    host = sp.parse_bed_host(good, "f")["c1"]
    assert [a.tolist() for a in host[:6]] == [[5], [0], [67], [7], [42], [3]]
    bad_lines = [good.replace(b"\n", b"\r\n"), b"\n", good.replace(b"\tC\t", b"\t\tC\t"), good.replace(b"c1", b"c2"), good.replace(b"\t42\t", b"\t+42\t"),
                 good.replace(b"\t42\t", b"\t101\t"), good.replace(b"\t5\t6\tC", b"\t10\t11\tC"), good.replace(b"\t7\t42\t3", b"\t2\t42\t3"),
                 good.replace(b"\t+\t", b"\t*\t"), good.replace(b"\tC\t", b"\tCC\t"), b"\t".join(good.split(b"\t")[:11]) + b"\n",
                 good.replace(b"\t7\t42", b"\t12345678901\t42"), good.replace(b"\t7\t42", b"\t2147483648\t42"), good.replace(b"3\n", b"3\t\n")]
    for k, line in enumerate(bad_lines):
        _, flag, bad = sp.parse_device_grammar(good + line + good, "c1", 10)
        assert (flag, bad) == (1, 2), (k, line)
    rec, flag, bad = sp.parse_device_grammar(good.replace(b"\t7\t42\t3", b"\t2147483647\t42\t2147483647")[:-1] + b"\textra field", "c1", 10)
    assert (flag, bad) == (0, -1) and rec[3].tolist() == [2 ** 31 - 1] and rec[5].tolist() == [2 ** 31 - 1]


def test_host_parser_refuses_with_file_and_line():
    good = "c1 5 6 C 7 +  5 6 0,0,0 7 42 3 \n"                                      # two spaces and a trailing one: white-space split
    assert sp.parse_bed_host((good + "\n" + good).encode(), "f")["c1"][6].tolist() == [1, 3]
    for line in ("c1 5 6 C 7 + 5 6 0,0,0 7 42\n", "c1 x 6 C 7 + 5 6 0,0,0 7 42 3\n", "c1 5 6 C 7 ? 5 6 0,0,0 7 42 3\n", "c1 5 6 C 7 + 5 6 0,0,0 7 142 3\n"):
        with pytest.raises(sp.SitePerfError, match=r"^f:2: "):
            sp.parse_bed_host((good + line).encode(), "f")


def test_command_refusals(tmp_path):
    case = CASES["empty_class"]
    mo = write_case(case, str(tmp_path))
    eng = lambda: sp.HostEngine((1, 5))
    empty = tmp_path / "empty"
    empty.mkdir()
    for change, words in (({"predFolder": str(empty)}, "no mod_pos"), ({"control": [str(empty)]}, "no mod_pos"), ({"control": [str(tmp_path / "none")]}, "no prediction folder"),
                          ({"Ref": str(tmp_path / "none.fa")}, "reference file does not exist"), ({"start": 5}, "need --chr"),
                          ({"cov": tuple(range(1, 10))}, "1 to 8 coverage thresholds"), ({"motif": "cG", "ModinMotif": 0}, "lower case"),
                          ({"ModinMotif": 2}, "no position in the motif"), ({"chr": "absent"}, "holds no contig")):
        with pytest.raises(sp.SitePerfError, match=words):
            sp.siteperf(dict(mo, **change), engine=eng())
    # a position that is not on the contig: refused with file and line
    over = dict(case, run={"mod_pos.x.C.bed": "ctg\t800\t801\tC\t3\t+\t800\t801\t0,0,0\t3\t0\t0\n"})
    mo2 = write_case(over, str(tmp_path / "over"))
    with pytest.raises(sp.SitePerfError, match=r"mod_pos\.x\.C\.bed:1: position 800 is not on ctg"):
        sp.siteperf(mo2, engine=eng())
    # lines of a contig that is not evaluated are passed over and counted
    other = dict(case, run=dict(case["run"], **{"mod_pos.y.C.bed": "elsewhere\t1\t2\tC\t3\t+\t1\t2\t0,0,0\t3\t0\t0\n" * 3}))
    mo3 = write_case(other, str(tmp_path / "other"))
    doc = sp.siteperf(mo3, engine=eng())
    assert doc["lines_other_contig"] == 3 and doc["lines"] == golden_lines(case, mo3["outFolder"])


def run_cli(args, cwd):
    return subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True)


def test_command_line_refuses_in_one_line(tmp_path):
    cli = os.path.join(ROOT, "bin", "DeepMod.py")
    mo = write_case(CASES["empty_class"], str(tmp_path))
    base = ["siteperf", "--predFolder", mo["predFolder"], "--control", ",".join(mo["control"]), "--Ref", mo["Ref"], "--motif", "Cg", "--ModinMotif", "0",
            "--outFolder", mo["outFolder"], "--FileID", "t"]
    for extra, words in ((["--start", "5"], "need --chr"), (["--cov", "1,2,3,4,5,6,7,8,9"], "1 to 8 coverage thresholds"), (["--Ref", str(tmp_path / "no.fa")], "does not exist")):
        out = run_cli([cli] + base + extra, str(tmp_path))
        assert out.returncode != 0
        assert words in out.stderr and len(out.stderr.strip().splitlines()) == 1, out.stderr


def test_shim_argument_mapping():
    mo = sp.shim_options(["run", "g.fa", "Cg", "0", "", "-1", "-1", "figs", "c1,c2"])
    assert mo == {"predFolder": "run", "Ref": "g.fa", "motif": "Cg", "ModinMotif": 0, "chr": None, "start": None, "end": None, "outFolder": "figs", "figure_folder": "figs",
                  "FileID": "cal_EcoliDetPerf", "control": ["c1", "c2"], "cov": (1, 5), "threads": 1}
    mo = sp.shim_options(["run", "g.fa", "gaAttc", "2", "eco", "10", "99", "figs", "c1"])
    assert (mo["chr"], mo["start"], mo["end"], mo["ModinMotif"], mo["control"]) == ("eco", 10, 99, 2, ["c1"])
    with pytest.raises(sp.SitePerfError, match="usage"):
        sp.shim_options(["run"])
    with open(os.path.join(ROOT, "DeepMod_tools", "cal_EcoliDetPerf.py")) as fh:
        assert "shim_options(sys.argv[1:])" in fh.read()


def test_measures_without_entries_and_without_a_class():
    h = np.zeros((sp.NCAT, 2, 2, sp.NPCT), np.int64)
    m = sp.measures(h, (1, 5))
    assert np.isnan(m["all_mp"][1]["auc"]) and np.isnan(m["all_mp"][1]["ap"])
    h[0, 0, 0, 10] = 3                                                              # negatives only: sklearn's recall-is-one rule gives ap 0.0
    m = sp.measures(h, (1, 5))
    assert np.isnan(m["motif_mp"][1]["auc"]) and m["motif_mp"][1]["ap"] == 0.0 and np.isnan(m["motif_mp"][5]["ap"])
    h[0, 1, 1, 90] = 2                                                              # perfectly separated
    m = sp.measures(h, (1, 5))
    assert m["motif_mp"][1]["auc"] == 1.0 and m["motif_mp"][1]["ap"] == 1.0
    assert m["motif_mp"][5]["positives"] == 2 and m["motif_mp"][5]["negatives"] == 0 and m["motif_mp"][5]["ap"] == 1.0


def test_line_routine_under_address_sanitizer(tmp_path):
    """tests/siteperf_asan_driver.cpp: csrc/siteperf.inc (on csrc/bedline.inc) built as a PROGRAM with -fsanitize=address,undefined and the sanitizer
    runtime linked in statically - every text and record array in a heap block of exactly its size; the good and bad lines above, texts cut at every
    byte, random byte mutations; every accepted record inside the contig, percentage <= 100, modified <= coverage."""
    gxx = shutil.which('g++')
    runtime = subprocess.run([gxx, '-print-file-name=libasan.a'], capture_output=True, text=True).stdout.strip() if gxx else ''
    if not gxx or not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip('g++ / static libasan not available')
    exe = str(tmp_path / 'siteperf_asan_driver')
    build = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'siteperf_asan_driver.cpp')],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:verify_asan_link_order=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'SITEPERF-ASAN-OK' in res.stdout, res.stdout[-1500:] + res.stderr[-4000:]
