"""GPU (-m gpu): one handle, texts of several sizes in a row - what a buffer set shared by every text parser (csrc/host.h DevBufs, csrc/textlines.hip.inc)
could newly break: a block kept from a larger text, a block grown for the next, the appended newline behind a shorter text.  For each of XYLoader,
siteperf.DeviceEngine, merge.DeviceMerge and bsperf.DeviceEngine one handle takes 3 T + 5 bytes, one line, exactly 2 T bytes ending in a newline,
T + 1 bytes without a final newline and a text with one bad line (T = dm_xyload_tile_bytes()), and after each the records on the device and the
first bad line equal the host parser's on the same bytes.  Reference: the line routines compiled for the host (parse_host / parse_device_grammar),
which the host tests hold to np.loadtxt and to the reference tools."""
import numpy as np
import pytest

from deepmod_amd import _lib, bsperf, merge, siteperf, xyload

pytestmark = pytest.mark.gpu

BS_NAMES, BS_LENGTHS = ['chr1', 'chr10', 'chrX'], [3000, 2000, None]


def xy_line(i, longer):
    return '%d.000 0.000 1.000 0.%03d 1.000 0.000 0.000 -1.250 0.125 %d.000\n' % (10 + i % 90, i % 1000, 33 if longer else 3)


def sp_line(i, longer):
    return 'c1\t%d\t6\tC\t%d\t%s\t5\t6\t0,0,0\t%d\t%d\t%d\n' % (i % 10, 77 if longer else 7, '+-'[i % 2], 200 + i % 800, 10 + i % 90, 100 + i % 100)


def bm_line(i, longer):
    return 'chr1 %d 6 C %d %s  5 6 0,0,0 %d 42 %d\n' % (1000 + i % 1000, 77 if longer else 7, '+-'[i % 2], 200 + i % 800, 100 + i % 100)


def bs_line(i, longer):
    return 'chr1\t%d\t6\t.\t%d\t%s\t5\t6\t0,0,0\t%d\t%d\n' % (1000 + i % 1000, 77 if longer else 7, '+-'[i % 2], 100 + i % 900, 10 + i % 90)


def exact(line, size, final_newline=True):
    """A text of exactly `size` bytes of lines line(i, False) (L bytes) and line(i, True) (L + 1 bytes), the last one with or without its newline."""
    total = size if final_newline else size + 1
    L = len(line(0, False))
    assert len(line(0, True)) == L + 1 and total >= L * L
    n, longer = total // L, total % L                                 # n lines, `longer` of them one byte longer: n L + longer = total
    text = ''.join(line(i, i < longer) for i in range(n))
    assert len(text) == total
    return (text if final_newline else text[:-1]).encode()


def texts(line, bad_line):
    T = _lib.load().dm_xyload_tile_bytes()
    assert T == 4096
    out = [exact(line, 3 * T + 5), line(7, False).encode(), exact(line, 2 * T), exact(line, T + 1, final_newline=False),
           (line(1, False) + bad_line + '\n' + line(2, True)).encode()]
    assert [len(t) for t in out[:4]] == [3 * T + 5, len(line(7, False)), 2 * T, T + 1] and out[2].endswith(b'\n') and not out[3].endswith(b'\n')
    return out


def same(got, want):
    return len(got) == len(want) and all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, want))


def test_xyloader_across_sizes(gpu_device):
    ld = xyload.XYLoader(gpu_device)
    flags = []
    for text in texts(xy_line, xy_line(3, False)[:-1] + '\r'):
        table, flag, bad = xyload.parse_host(text)
        assert ld.parse(text) == (len(table), flag, bad)
        feats, head = ld.fetch_table()
        assert np.array_equal(np.hstack([head, feats]).view(np.uint32), table.view(np.uint32))
        flags.append((flag, bad))
    assert flags == [(0, -1)] * 4 + [(1, 2)]
    ld.close()


def test_siteperf_engine_across_sizes(gpu_device):
    e = siteperf.DeviceEngine((1, 5), gpu_device)
    e.set_contig(b'ACGCGTTGAT', 'Cg', 0)
    flags = []
    for text in texts(sp_line, sp_line(3, False)[:-1] + '\t'):
        want, flag, bad = siteperf.parse_device_grammar(text, 'c1', 10)
        assert e.add_text(text, siteperf.RUN, 'c1') == (len(want[0]), flag, bad)
        assert same(e.records(), [a[:0] for a in want] if flag else want)            # a flagged text leaves no records
        flags.append((flag, bad))
    assert flags == [(0, -1)] * 4 + [(1, 2)]
    e.close()


def test_device_merge_across_sizes(gpu_device):
    d = merge.DeviceMerge(gpu_device)
    d.open('chr1', 2000)
    flags = []
    for text in texts(bm_line, 'chr1 5 6 C 7 + 5 6 0,0,0 7 42 8'):
        want, flag, bad = merge.parse_device_grammar(text, 'chr1', 2000)
        assert d.add_text(text) == (len(want[0]), flag, bad)
        assert same(d.records(), [a[:0] for a in want] if flag else want)
        flags.append((flag, bad))
    assert flags == [(0, -1)] * 4 + [(1, 2)]
    d.close()


def test_bsperf_engine_across_sizes(gpu_device):
    e = bsperf.DeviceEngine(BS_NAMES, lengths=BS_LENGTHS, device=gpu_device)
    flags = []
    for k, text in enumerate(texts(bs_line, 'chr1 5 6 . 7 + 5 6 0,0,0 7 101')):
        want, lines, flag, bad = bsperf.parse_device_grammar(text, BS_NAMES, BS_LENGTHS, first_chunk=k == 0)
        got_lines, n, got_flag, got_bad = e.add_truth_text(0, text, first_chunk=k == 0)
        assert (got_flag, got_bad) == (flag, bad)
        if flag:                                                                     # a flagged chunk adds nothing
            assert n == 0 and not got_lines.any()
        else:
            assert n == len(want[0]) and np.array_equal(got_lines, lines) and same(e.records(), want)
        flags.append((flag, bad))
    assert flags == [(0, -1)] * 4 + [(1, 2)]
    e.close()
