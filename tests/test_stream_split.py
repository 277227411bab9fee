"""CPU: the streaming path as four modules (deepmod_amd/batch.py, handover.py, sigserver.py, stream.py): the one byte layout of a handed-over batch
holds the offsets it always had, a feeder process loads nothing of the device side, and deepmod_amd.stream still carries every name that tests and
tools reach through it."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from deepmod_amd import batch, handover, sigserver, stream

# (n_rows, n_pos, n_sel) -> (o_pos, o_flags, end, o_sel), cls: the values of the hand-written _shm_layout and of HipBackend.submit's own arithmetic
CLASSIC = {(0, 0, 0): ((0, 0, 1, 256), 256),
           (5, 9, 0): ((256, 512, 521, 768), 768),
           (5, 9, 4): ((256, 512, 784, 768), 1024),
           (1000, 1003, 0): ((28160, 36352, 37355, 37376), 37376),
           (1000, 260, 250): ((28160, 30464, 31976, 30976), 32000)}
# (n_rows, n_pos, n_sel, n_ev, n_reads) -> (ev3, code, rdesc, pos, flags, sel, end), rows, cls: of _shm_layout_dev and the same arithmetic
DEVICE = {(0, 0, 0, 0, 0): ((0, 256, 512, 768, 1024, 1280, 1284), 1536, 1536),
          (5, 9, 4, 37, 3): ((0, 512, 768, 1024, 1280, 1536, 1552), 1792, 2048),
          (5, 9, 4, 0, 3): ((0, 256, 512, 768, 1024, 1280, 1296), 1536, 1792),           # the resident form: no event crosses
          (1000, 260, 250, 700, 12): ((0, 8448, 9472, 9984, 12288, 12800, 13800), 13824, 41984)}


def _offsets(buf, views):
    base = np.frombuffer(buf, np.uint8).ctypes.data
    return [(v.ctypes.data - base, v.shape, v.dtype) for v in views]


def test_batch_layout_is_the_bytes_it_always_was():
    """handover.BatchLayout, as literals: the feeder's slot, the GPU process' view of it and the staging set of HipBackend.submit are laid out by this one
    object, so a slip in it is self-consistent and no round trip sees it - quirks included (without sel the classic form ends behind its flags)."""
    for (R, T, S), ((o_pos, o_flags, end, o_sel), cls) in CLASSIC.items():
        lay = handover.BatchLayout(R, T, S)
        assert (lay.o['rows'], lay.o['pos'], lay.o['flags'], lay.o['sel'], lay.o['end']) == (0, o_pos, o_flags, o_sel, end), (R, T, S)
        assert (lay.end, lay.rows, lay.cls) == (end, 0, cls), (R, T, S)
        buf = bytearray(lay.end)
        want = [(0, (R, 7), np.float32), (o_pos, (T,), np.int64), (o_flags, (T,), np.uint8)] + ([(o_sel, (S,), np.int32)] if S else [])
        assert _offsets(buf, lay.views(buf)) == want, (R, T, S)
    for (R, T, S, E, N), (offs, rows, cls) in DEVICE.items():
        lay = handover.BatchLayout(R, T, S, dev=(E, N))
        names = ('ev3', 'code', 'rdesc', 'pos', 'flags', 'sel', 'end')
        assert lay.o == dict(zip(names, offs)) and handover._shm_layout_dev(R, T, S, E, N) == lay.o, (R, T, S, E, N)
        assert (lay.end, lay.rows, lay.cls) == (offs[-1], rows, cls), (R, T, S, E, N)
        buf = bytearray(lay.end)
        want = [(offs[0], (max(E, 1), 3), np.float32), (offs[1], (R,), np.uint8), (offs[2], (N, 4), np.int64), (offs[3], (T,), np.int64),
                (offs[4], (T,), np.uint8), (offs[5], (S,), np.int32)]
        assert _offsets(buf, lay.views(buf)) == want, (R, T, S, E, N)


@pytest.mark.parametrize('module', ['deepmod_amd.handover', 'deepmod_amd.sigserver'])
def test_feeder_side_modules_load_nothing_of_the_device_side(module):
    """A spawned feeder process imports the module of feeder_process_main: that must not bring torch, the model, the counters or the engine with it."""
    code = ("import sys, %s\n"
            "bad = [m for m in ('torch', 'deepmod_amd.model', 'deepmod_amd.summary', 'deepmod_amd.stream') if m in sys.modules]\n"
            "assert not bad, bad\n"
            "ours = sorted(m for m in sys.modules if m.startswith('deepmod_amd.'))\n"
            "allowed = ['deepmod_amd.' + m for m in ('_lib', 'predstore', 'rawreads', 'signal', 'batch', 'handover')] + [%r]\n"
            "assert set(ours) <= set(allowed), ours\n" % (module, module))
    res = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]


def test_stream_still_carries_the_names_tests_and_tools_reach_through_it():
    homes = {batch: ('Prepared', 'assemble_rows', 'rows_from_reads', 'prepare_batch', '_prepare_batch_c', '_prepare_batch_py'),
             handover: ('feeder_process_main', 'prepared_from_shm', 'shm_dir_for', 'WorkList', '_shm_layout_dev'),
             sigserver: ('RemoteSignalNormalizer', 'SignalResults', 'DeviceBlockPool', 'signal_server', '_sig_layout', '_sig_layout_res', '_sig_layout_move')}
    for home, names in homes.items():
        for name in names:
            assert getattr(stream, name) is getattr(home, name), name
