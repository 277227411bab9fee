"""Dev tool (GPU box): end-to-end rate of `bin/DeepMod.py detect` from RAW containers (signal + events + alignments: the
reference's FAST5 shape) - signal statistics on the GPU, dm_map_read, get_Feature, classifier, on-device summary, BED.
    python tools/e2e_detect_raw.py [n_reads] [threads,threads,...] [options of this tool] [more arguments of detect]

--move      the measurement of `detect --move` (profiles/move/README.md): a run of reads with MOVE TABLES and its twin event-table run are
            generated; per thread count three variants are timed, --runs times each, interleaved:
              move         detect --move                              (move tables posted to the signal stage, segmented on the device)
              move_host    detect --move, DEEPMOD_MOVE_ON_DEVICE=0   (event tables built by dm_move_events, posted as for an event-table run)
              twin         detect on the twin run                    (the event-table path)
            and the BED files of the three are compared.
--tree DIR  with --move: also time the twin run with bin/DeepMod.py of another checkout of this repository (built there), e.g. the parent commit
--repeat K  the work folder holds the generated containers K times by symbolic links (as bench.py's e2e_raw leg: 4,000 reads x 20)
--runs N    runs per variant (default 1; 3 with --move)
--only V    with --move: one variant only (move | move_host | twin; twin keeps the --tree run beside it), e.g. under a profiler
"""
import argparse, glob, multiprocessing, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deepmod_amd import synth, synth_reads

GENOME = 500000


def _gen(args):
    out, part, n, move, twin = args
    kw = dict(move=True, twin_dir=twin) if move else {}
    return synth_reads.write_synthetic_raw_run(out, n_reads=n, reads_per_file=10, genome_len=GENOME, seed=3, chrom="chrS", part=part,
                                               min_len=2000, max_len=8000, **kw)[0]


def _link(src, dst, repeat):
    """dst: the containers (and side-car SAM files) of src `repeat` times by symbolic links, one genome"""
    os.makedirs(dst)
    os.symlink(os.path.join(src, "genome.fa"), os.path.join(dst, "genome.fa"))
    for k in range(repeat):
        for f in sorted(glob.glob(os.path.join(src, "*.dmraw.npz"))):
            stem = f[:-len(".dmraw.npz")]
            os.symlink(f, os.path.join(dst, "c%02d_%s" % (k, os.path.basename(f))))
            os.symlink(stem + ".sam", os.path.join(dst, "c%02d_%s.sam" % (k, os.path.basename(stem))))
    return dst


def _run(tree, wrk, prefix, out, threads, extra, env=None):
    cmd = [sys.executable, os.path.join(tree, "bin", "DeepMod.py"), "detect", "--wrkBase", wrk, "--Ref", wrk + "/genome.fa", "--modfile", prefix,
           "--outFolder", out, "--Base", "C", "--gpus", "1", "--threads", str(threads), "--FileID", "raw", "--alignStr", "minimap2"] + extra
    t0 = time.time()
    res = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    wall = time.time() - t0
    if res.returncode:
        print(res.stdout[-2000:], res.stderr[-3000:])
        sys.exit(1)
    return wall, res.stdout


def _times(wall, so):
    """-> (whole command s, detect step s, steady state s = device drained - first batch from a feeder, base-positions)"""
    m1 = re.search(r"Streaming detect: (\d+) reads, (\d+) base-positions .* in ([0-9.]+) s", so)
    m3 = re.search(r"first batch from a feeder ([0-9.]+), last batch ([0-9.]+), device drained ([0-9.]+)", so)
    return wall, float(m1.group(3)) if m1 else float("nan"), (float(m3.group(3)) - float(m3.group(1))) if m3 else float("nan"), int(m1.group(2)) if m1 else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("n_reads", nargs="?", type=int, default=3000)
    ap.add_argument("threads", nargs="?", default=None)
    ap.add_argument("--move", action="store_true")
    ap.add_argument("--tree", default=None)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--runs", type=int, default=None)
    ap.add_argument("--only", choices=["move", "move_host", "twin"], default=None)
    args, detect_args = ap.parse_known_args()
    n_reads = args.n_reads
    ncpu = min(32, len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS") or 32))
    thread_list = [int(v) for v in args.threads.split(",")] if args.threads else [ncpu]
    runs = args.runs or (3 if args.move else 1)
    tmp = tempfile.mkdtemp()
    src, twin_src = tmp + "/src", (tmp + "/src_twin" if args.move else None)
    per = -(-n_reads // ncpu)
    t0 = time.time()
    with multiprocessing.get_context("spawn").Pool(ncpu) as pool:
        files = sum(pool.map(_gen, [(src, p, per, args.move, twin_src) for p in range(ncpu)]), [])
    size = sum(os.path.getsize(f) for f in files)
    print("generated %d raw containers (%d reads, %.2f GB%s) in %.1f s; the work folder holds them %d x" %
          (len(files), per * ncpu, size / 1e9, "; move tables, and the twin event-table run" if args.move else "", time.time() - t0, args.repeat), flush=True)
    wrk = _link(src, tmp + "/in", args.repeat)
    twin = _link(twin_src, tmp + "/in_twin", args.repeat) if args.move else None
    prefix = tmp + "/model/m"
    os.makedirs(tmp + "/model")
    synth.write_synthetic_checkpoint(prefix, seed=26, scale=4.0)
    for threads in thread_list:
        if not args.move:
            for k in range(runs):
                wall, so = _run(ROOT, wrk, prefix, "%s/out%d_%d" % (tmp, threads, k), threads, detect_args)
                for ln in so.splitlines():
                    if "Streaming detect" in ln or "host stages" in ln or "timeline" in ln:
                        print(ln.strip())
                print("raw containers -> BED: %d feeder threads, whole command %.1f s" % (threads, wall))
            continue
        variants = [("move", ROOT, wrk, ["--move"], {}), ("move_host", ROOT, wrk, ["--move"], {"DEEPMOD_MOVE_ON_DEVICE": "0"}), ("twin", ROOT, twin, [], {})]
        if args.tree:
            variants.append(("twin@" + os.path.basename(os.path.normpath(args.tree)), os.path.abspath(args.tree), twin, [], {}))
        if args.only:
            variants = [v for v in variants if v[0].split("@")[0] == args.only]
        got, beds = {v[0]: [] for v in variants}, {}
        for k in range(runs):
            for name, tree, folder, extra, env in variants:        # interleaved: a drift of the box meets every variant alike
                out = "%s/out_%s_%d_%d" % (tmp, name.replace("@", "_"), threads, k)
                wall, so = _run(tree, folder, prefix, out, threads, extra + detect_args, env)
                got[name].append(_times(wall, so))
                beds.setdefault(name, {os.path.basename(f): open(f, "rb").read() for f in glob.glob(out + "/raw/*.bed")})
                print("%-12s run %d: whole command %.2f s, detect step %.2f s, steady state %.2f s (%d base-positions)" % ((name, k) + got[name][-1]), flush=True)
                if k == 0:
                    for ln in so.splitlines():
                        if "host stages" in ln or "signal stage" in ln:
                            print("    " + ln.strip())
        print("BED files of all variants identical: %s" % (all(b == beds[variants[0][0]] and len(b) == 2 for b in beds.values()),))
        for name, rows in got.items():
            cols = list(zip(*[r[:3] for r in rows]))
            print("%-12s %d feeder threads, %d runs: " % (name, threads, len(rows)) +
                  ", ".join("%s median %.2f s (min %.2f, max %.2f)" % (what, sorted(c)[len(c) // 2], min(c), max(c)) for what, c in zip(("whole command", "detect step", "steady state"), cols)))
