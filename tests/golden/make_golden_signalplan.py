"""What dm_signal_plan_batch answers, recorded from the library of the checkout this file lies in: the host-only planner of a signal batch is the one
piece of the stage's host arithmetic the C ABI exposes, so its answers at one commit hold a later rewrite of that arithmetic to the same results
(tests/test_signal.py::test_plan_of_a_batch_answers_as_recorded).

Output (plain data): signalplan.json - per case of cases() below the recorded return code, first_empty (accepted batches) and message (refused
ones).  The test takes the inputs from cases() and asks through answer(), as this file did.

Run in a checkout whose library is built, at the commit to record:  python tests/golden/make_golden_signalplan.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
U64 = 2 ** 64


def cases():
    """name -> (raw_off, ev_off, start, length)"""
    three = ([0, 60, 200, 230], [0, 3, 7, 9])
    out = {
        'one_read': ([0, 100], [0, 3], [5, 20, 40], [15, 20, 30]),
        'single_event': ([0, 50], [0, 1], [7], [9]),
        'single_event_off_the_end': ([0, 50], [0, 1], [49], [900]),
        'three_reads_empty_at_0_middle_nowhere': three + ([10, 10, 30, 0, 40, 80, 100, 2, 12], [0, 20, 25, 40, U64 - 11, 20, 30, 10, 500]),
        'three_reads_nothing_empty': three + ([10, 10, 30, 0, 40, 80, 100, 2, 12], [5, 20, 25, 40, 10, 20, 30, 10, 500]),
        'start_2_63_inside': ([0, 1000], [0, 4], [0, 2 ** 63 + 7, 20, 30], [10, 10, 10, 10]),
        'start_2_64_minus_5_last': ([0, 1000], [0, 4], [0, 10, 20, U64 - 5], [10, 10, 10, 3]),
        'start_2_63_first': ([0, 1000], [0, 4], [2 ** 63, 10, 20, 30], [10, 10, 10, 10]),
        'end_wraps_before_start': ([0, 1000], [0, 4], [8, 10, 20, 30], [2, 10, 10, U64 - 25]),
        'end_wraps_inside': ([0, 1000], [0, 4], [0, 10, 20, 30], [10, U64 - 5, 10, 10]),
        'end_wraps_in_second_read': ([0, 10, 30], [0, 1, 3], [0, 12, 3], [5, 4, U64 - 1]),
        'all_events_empty_but_the_slice': ([0, 40], [0, 3], [5, 9, 9], [0, 0, 20]),
        'read_without_events': ([0, 10, 20], [0, 2, 2], [1, 2], [2, 2]),
        'read_without_samples': ([0, 20, 20], [0, 2, 4], [1, 2, 3, 4], [2, 2, 2, 2]),
        'raw_offsets_decrease': ([0, 20, 10], [0, 2, 4], [1, 2, 3, 4], [2, 2, 2, 2]),
        'raw_off_starts_at_1': ([1, 10, 20], [0, 2, 4], [1, 2, 3, 4], [2, 2, 2, 2]),
        'ev_off_starts_at_2': ([0, 10, 20], [2, 2, 4], [1, 2, 3, 4], [2, 2, 2, 2]),
        'no_samples_at_all': ([0, 10, 0], [0, 2, 4], [1, 2, 3, 4], [2, 2, 2, 2]),
        'no_events_at_all': ([0, 10, 20], [0, 2, 0], [1, 2, 3, 4], [2, 2, 2, 2]),
        'reads_4096': (list(range(4097)), list(range(4097)), [0] * 4096, [1] * 4096),
        'reads_4097': (list(range(4098)), list(range(4098)), [0] * 4097, [1] * 4097),
    }
    return out


def answer(lib, last_error, raw_off, ev_off, start, length):
    ro, eo = np.asarray(raw_off, np.int64), np.asarray(ev_off, np.int64)
    st, ln = np.asarray(start, np.uint64), np.asarray(length, np.uint64)
    n = len(ro) - 1
    fe = np.full(n, -7, np.int64)
    rc = int(lib.dm_signal_plan_batch(n, ro.ctypes.data, eo.ctypes.data, st.ctypes.data, ln.ctypes.data, fe.ctypes.data))
    return {'rc': rc, 'first_empty': fe.tolist() if rc == 0 else None, 'message': None if rc == 0 else last_error()}


def main():
    sys.path.insert(0, ROOT)
    from deepmod_amd import _lib
    lib = _lib.load()
    out = {}
    for name, (raw_off, ev_off, start, length) in cases().items():
        got = answer(lib, _lib.last_error, raw_off, ev_off, start, length)
        out[name] = got
        print('%-40s rc %2d %s' % (name, got['rc'], got['first_empty'] if got['rc'] == 0 and len(raw_off) < 10 else got['message'] or ''))
    path = os.path.join(HERE, 'signalplan.json')
    with open(path, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
        f.write('\n')
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
