"""Writes tests/golden/edges_parent_bits.npz: the probability bits (uint32 views) and classes of the calls of tests/edges_cases.py, for both
split-f16 modes and both weight sets.  Run ONCE, on a GPU, with the library of the commit before the classifier's edge work (profiles/edges):

    python tests/golden/make_golden_edges.py [path/to/that/libdeepmod_hip.so] [output.npz]

tests/test_gpu_edges.py holds every later library to these bits exactly.  Re-running it on a later library would only record that library
against itself: do that when a change is MEANT to move bits, and say so."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    from deepmod_amd import _lib
    if len(argv) > 1:
        _lib.LIB_PATH = os.path.abspath(argv[1])
    out_path = argv[2] if len(argv) > 2 else None
    import edges_cases as ec
    from deepmod_amd import model
    lib = _lib.load()
    out = {"library": np.array(lib.dm_version().decode() + " | " + lib.dm_build_flags().decode())}
    for wname in ec.WEIGHTS:
        w = ec.weights(wname)
        for precision in ec.PRECISIONS:
            m = model.BiLSTMModel(w, device=0, precision=precision)
            for case in ec.CASES:
                prob, cls, geo = ec.run(m, case)
                out[ec.key(wname, precision, case, "prob")] = ec.bits(prob)
                out[ec.key(wname, precision, case, "cls")] = np.ascontiguousarray(cls, np.uint8)
                print("%-9s %-5s %-12s n = %6d  grid %3d of %3d  class 1: %d" % (wname, precision, case, len(cls), geo[1], geo[0], int(cls.sum())), flush=True)
            m.close()
    out_path = out_path or ec.FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez_compressed(out_path, **out)
    print("wrote %s: %d bytes" % (out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    main(sys.argv)
