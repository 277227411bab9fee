"""The hand-over of a batch from a feeder process to the GPU process of the streaming detect (deepmod_amd/stream.py has the overview of the path):
the byte layout of a handed-over batch (`BatchLayout`), the body of a feeder process, the GPU process' view of what it prepared, the work list the
feeders take their batches from.  A spawned feeder imports this module and the batch builder, never the device side (model, summary, stream)."""
from __future__ import annotations

import os
import queue
from typing import Optional

import numpy as np

from .batch import Prepared, prepare_batch


# ---------------------------------------------------------------------------------------------
# feeder processes: the host side of a batch is numpy / zipfile / small C calls per read - Python threads serialise on the
# interpreter lock (32 feeder threads prepared 1.5x what one does), so the CLI prepares batches in worker PROCESSES and
# hands the three arrays over through a file in /dev/shm that the GPU process maps (and unlinks at once).
# ---------------------------------------------------------------------------------------------
_ALIGN = 256


def _layout(fields, align: int = 64):
    """[(name, nbytes)] -> {name: byte offset, ..., 'end': size}: the fields back to back, each on a multiple of `align`.  A field of 0 bytes takes no
    room: ('in_end', 0) marks the place where the inputs of a request end."""
    o, pos = {}, 0
    for name, nbytes in fields:
        o[name] = pos
        pos = -(-(pos + nbytes) // align) * align
    o['end'] = pos
    return o


class BatchLayout:
    """Byte layout of a handed-over batch, the one statement of it: the feeder sizes and fills its slot by it, the GPU process reads the slot and
    lays out its staging set by it.  Two forms, each array on a multiple of 256 bytes:
      classic / compact (dev None)   [rows f32[n_rows][7] | pos i64[n_pos] | flags u8[n_pos] | sel i32[n_sel]]
      device form (dev = (n_ev, n_reads); the resident form has n_ev 0)
                                     [ev3 f32[n_ev][3] | code u8[n_rows] | rdesc i64[n_reads][4] | pos i64[n_pos] | flags u8[n_pos] | sel i32[n_sel]]
    `o`: name -> offset, with 'end' = `end`, the bytes that cross processes and PCIe (the last array is not padded; without sel the classic form
    ends behind its flags and leaves o['sel'] unused).  Behind `end`, on the device only: `rows`, where the feature rows lie there (the device
    form assembles them, the classic form uploads them at 0), and `cls`, the classes."""
    __slots__ = ('n_rows', 'n_pos', 'n_sel', 'dev', 'o', 'end', 'rows', 'cls')

    def __init__(self, n_rows: int, n_pos: int, n_sel: int = 0, dev=None):
        self.n_rows, self.n_pos, self.n_sel, self.dev = n_rows, n_pos, n_sel, dev
        up = lambda nbytes: -(-nbytes // _ALIGN) * _ALIGN
        if dev is None:
            o = _layout((('rows', 28 * n_rows), ('pos', 8 * n_pos), ('flags', max(n_pos, 1)), ('sel', 4 * n_sel)), _ALIGN)
            o['end'] = o['sel'] + 4 * n_sel if n_sel else o['flags'] + max(n_pos, 1)
            self.rows, self.cls = 0, up(o['end'])
        else:
            o = _layout((('ev3', 12 * max(dev[0], 1)), ('code', max(n_rows, 1)), ('rdesc', 32 * max(dev[1], 1)), ('pos', 8 * max(n_pos, 1)),
                         ('flags', max(n_pos, 1)), ('sel', 4 * max(n_sel, 1))), _ALIGN)
            o['end'] = o['sel'] + 4 * max(n_sel, 1)
            self.rows = up(o['end'])                 # nothing is uploaded behind `end`
            self.cls = self.rows + up(28 * n_rows)
        self.o, self.end = o, o['end']

    def views(self, buf):
        """The arrays of a buffer of at least `end` bytes: (rows, pos, flags[, sel]), sel only when n_sel > 0; device form (ev3, code, rdesc, pos, flags, sel)"""
        view = lambda dtype, count, name: np.frombuffer(buf, dtype, count, self.o[name])
        pos_flags = (view(np.int64, self.n_pos, 'pos'), view(np.uint8, self.n_pos, 'flags'))
        if self.dev is None:
            return (view(np.float32, self.n_rows * 7, 'rows').reshape(self.n_rows, 7),) + pos_flags + ((view(np.int32, self.n_sel, 'sel'),) if self.n_sel else ())
        n_ev, n_reads = max(self.dev[0], 1), self.dev[1]
        return (view(np.float32, 3 * n_ev, 'ev3').reshape(-1, 3), view(np.uint8, self.n_rows, 'code'),
                view(np.int64, 4 * n_reads, 'rdesc').reshape(n_reads, 4)) + pos_flags + (view(np.int32, self.n_sel, 'sel'),)


def _shm_layout_dev(n_rows: int, n_pos: int, n_sel: int, n_ev: int, n_reads: int):
    """offsets of the device form by name, `end` included (BatchLayout)"""
    return BatchLayout(n_rows, n_pos, n_sel, (n_ev, n_reads)).o


def map_file(path: str, size: int, flags: int = 0):
    """Open a path, map `size` bytes of it read-write, close the descriptor -> the mapping.  flags = os.O_CREAT (| os.O_TRUNC): the file is created
    if need be and sized to `size` first."""
    import mmap
    fd = os.open(path, os.O_RDWR | flags, 0o600)
    try:
        if flags & os.O_CREAT:
            os.ftruncate(fd, size)
        return mmap.mmap(fd, size)
    finally:
        os.close(fd)


def usable_cpus() -> int:
    """CPUs this process may really use: affinity mask capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            n = min(n, max(1, int(float(quota) / float(period))))
    except Exception:
        pass
    return n


def shm_dir_for(moptions) -> str:
    """Directory of the hand-over files of this GPU process: /dev/shm when it has room (a container's default 64 MB tmpfs does
    not hold one batch), else the output folder (the files then go through the page cache of that file system)."""
    root = moptions['outFolder']
    try:
        st = os.statvfs('/dev/shm')
        if os.access('/dev/shm', os.W_OK) and st.f_bavail * st.f_frsize >= (2 << 30):
            root = '/dev/shm'
    except OSError:
        pass
    return os.path.join(root, 'deepmod_amd_%d' % os.getpid())


def feeder_process_main(moptions, work, ready, device: int, shm_dir: str, wid: int, free_slots=None, slot_bytes: int = 0,
                        sig_requests=None, sig_answers=None):
    """Body of one feeder process: file lists from `work` (a multiprocessing queue of (files, ...) items, filled before the
    run starts; empty = done) -> prepare_batch -> arrays into shared memory -> a small description on `ready`.
    Shared memory = one of the GPU process' page-locked slot files (`free_slots`: queue of slot numbers; the batch must fit
    `slot_bytes`), else a file of its own that the GPU process maps and unlinks."""
    import traceback
    norm = []

    def normalizer():                      # created on first use: only batches with raw containers need the signal stage
        if not norm:
            if sig_requests is not None:   # the GPU process' signal server: this process owns no HIP context
                from . import sigserver
                norm.append(sigserver.RemoteSignalNormalizer(wid, shm_dir, sig_requests, sig_answers))
            else:
                from . import signal as dmsignal
                norm.append(dmsignal.SignalNormalizer(device))
        return norm[0]

    slot_maps = {}

    def slot_map(i):
        if i not in slot_maps:
            slot_maps[i] = map_file(os.path.join(shm_dir, 'slot_%d' % i), slot_bytes)
        return slot_maps[i]

    seq = 0
    try:
        while True:
            try:
                item = work.get(block=False)
            except Exception:              # queue.Empty (also through a manager proxy): nothing left
                break
            files = item[0] if isinstance(item, tuple) else item
            path = os.path.join(shm_dir, 'b%d_%d' % (wid, seq))
            seq += 1
            holder = {}

            def alloc(n_rows, n_pos, n_sel=0, dev=None):
                holder['dev'] = dev
                lay = BatchLayout(n_rows, n_pos, n_sel, dev)
                if free_slots is not None and lay.end <= slot_bytes:
                    holder['slot'] = free_slots.get()                    # blocks while the device queue holds every slot
                    return lay.views(slot_map(holder['slot']))
                holder['mm'] = map_file(path, lay.end, os.O_CREAT | os.O_TRUNC)
                return lay.views(holder['mm'])

            pb = prepare_batch(moptions, files, normalizer, alloc)
            meta = {'path': path if 'mm' in holder else None, 'slot': holder.get('slot'), 'n_rows': pb.n_rows, 'n_pos': len(pb.pos),
                    'groups': pb.groups, 'n_windows': pb.n_windows, 'n_reads': pb.n_reads, 'errors': {k: list(v) for k, v in pb.errors.items()},
                    'contig_len': dict(pb.contig_len), 'timing': dict(pb.timing), 'files': list(pb.files), 'f32': pb.f32,
                    'n_sel': None if pb.sel is None else len(pb.sel), 'dev': holder.get('dev') if (pb.ev3 is not None or pb.code is not None) else None,
                    'sig': pb.sig}
            pb.rows = pb.pos = pb.flags = pb.sel = pb.ev3 = pb.code = pb.rdesc = None          # drop the views before a mapping goes away
            if 'mm' in holder:
                holder['mm'].close()
            ready.put(meta)
    except BaseException:
        ready.put({'failed': traceback.format_exc()})
    finally:
        ready.put(None)


def prepared_from_shm(meta, slot_buffer=None) -> Prepared:
    """The GPU process' view of a batch a feeder process prepared: in one of its page-locked slots (slot_buffer(i) -> the
    slot's mapping), or in a file of its own (unlinked as soon as it is mapped)."""
    import mmap
    pb = Prepared()
    pb.n_rows, pb.groups, pb.n_windows, pb.n_reads = meta['n_rows'], [tuple(g) for g in meta['groups']], meta['n_windows'], meta['n_reads']
    for k, v in meta['errors'].items():
        pb.errors[k].extend(v)
    pb.contig_len = dict(meta['contig_len'])
    for k, v in meta['timing'].items():
        pb.timing[k] += v
    pb.files = meta['files']
    pb.f32 = bool(meta.get('f32', False))
    n_sel = meta.get('n_sel')
    dev = meta.get('dev')
    mk = BatchLayout(meta['n_rows'], meta['n_pos'], n_sel or 0, dev).views
    views = None
    if meta.get('slot') is not None:
        views = mk(slot_buffer(meta['slot']))
    elif meta['path'] is not None:
        fd = os.open(meta['path'], os.O_RDONLY)
        try:
            mm = mmap.mmap(fd, 0, prot=mmap.PROT_READ)
        finally:
            os.close(fd)
            os.unlink(meta['path'])
        views = mk(mm)
    pb.sig = tuple(meta['sig']) if meta.get('sig') is not None else None
    if views is not None and dev is not None:
        pb.ev3, pb.code, pb.rdesc, pb.pos, pb.flags = views[:5]
        if pb.sig is not None:             # resident form: the statistics are a device block of the signal stage, nothing per event in the slot
            pb.ev3 = None
        pb.rows = None
        pb.sel = views[5] if n_sel else np.zeros(0, np.int32)
        return pb
    if views is not None:
        pb.rows, pb.pos, pb.flags = views[:3]
    if n_sel is not None:
        pb.sel = views[3] if (views is not None and n_sel) else np.zeros(0, np.int32)
    return pb


class WorkList:
    """The work items of one run, known before its processes start, handed out through one shared counter: what the feeders
    and ranks of a streaming run take their batches from.  Same calls as the reference's h5files_Q (`get(block=False)`, queue.Empty
    when nothing is left), without a manager process in between (0.2 s of start-up and shut-down on a 2 s run) and without the
    window in which a multiprocessing.Queue that was filled a moment ago still reads as empty.
    The items travel to the processes through a file, not through their start-up pipe: a spawned process receives its arguments
    through a pipe of 64 KB, and a parent that writes more blocks until the child's interpreter is up and reading - four feeders
    with the 2,000 paths of a run in their arguments started one after the other (0.07 s each) instead of side by side."""

    def __init__(self, items, ctx, directory: Optional[str] = None):
        import pickle
        import tempfile
        self._items = list(items)
        self.n = len(self._items)
        self.head = ctx.Value('q', 0)
        if directory is None and os.path.isdir('/dev/shm') and os.access('/dev/shm', os.W_OK):
            directory = '/dev/shm'
        try:
            fd, self.path = tempfile.mkstemp(prefix='deepmod_work_', suffix='.pkl', dir=directory)
        except OSError:                      # (a full or read-only /dev/shm: the default temporary directory)
            fd, self.path = tempfile.mkstemp(prefix='deepmod_work_', suffix='.pkl')
        with os.fdopen(fd, 'wb') as fh:
            pickle.dump(self._items, fh, protocol=4)

    def __getstate__(self):
        return {'_items': None, 'n': self.n, 'head': self.head, 'path': self.path}

    def get(self, block: bool = False):
        with self.head.get_lock():
            i = self.head.value
            if i >= self.n:
                raise queue.Empty
            self.head.value = i + 1
        if self._items is None:
            import pickle
            with open(self.path, 'rb') as fh:
                self._items = pickle.load(fh)
        return self._items[i]

    def empty(self) -> bool:
        return self.head.value >= self.n

    def close(self):
        """By the process that made the list, once every process that takes from it has ended."""
        try:
            os.remove(self.path)
        except OSError:
            pass

