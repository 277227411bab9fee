"""Streaming, read-sharded detect: one process per GPU keeps the per-position counters on the device for the
whole run and the only cross-process exchange is one integer RCCL reduce per contig x strand at the end.

The reference moves every read's predictions through the file system: detect workers write per-read tables
(myDetect.py:716-760) and per-chromosome index files (:762-782, :1194-1221), summary workers read them back and
accumulate a dict keyed by (chr, strand, pos) (:1028-1120); several runs are merged by adding BED files
(DeepMod_tools/sum_chr_mod.py:47-52).  Here the same arithmetic is

    worker batch -> feature rows + per-row (position, flags)           host, feeder threads   (`prepare_*`)
                 -> dm_predict_read (windows assembled on the device)   one in-order device queue per GPU
                 -> dm_summary_add_classified / dm_summary_add          (class -> base scatter of :824-833 fused with :1089-1100)
    end of run   -> dm_summary_reduce over a persistent communicator    deepmod_amd/comm.py
                 -> rank 0: dm_summary_fetch -> BED bytes               deepmod_amd/summary.py:bed_lines

and the BED files are byte-identical to the stored path's (tests/test_gpu_stream.py) for any number of ranks:
integer sums do not depend on the order or the sharding of the reads.

`StreamEngine` is the rank-local logic; it talks to the device through a small backend object (`HipBackend`: the C ABI).
tests/test_stream_gloo.py drives the same engine on CPU ranks with a stand-in backend (oracle classifier and counters,
gloo transport) - only the transport and the device calls are replaced, the sharding / grouping / merge logic is this file.

The path lives in four modules, one per place its code runs:
    batch.py      the batch builder: file list -> `Prepared` (`prepare_batch`).  Feeder threads and feeder processes, host only.
    handover.py   a batch from a feeder process to the GPU process: its byte layout (`BatchLayout`), `feeder_process_main`,
                  `prepared_from_shm`, the `WorkList` the feeders draw from.  A feeder process imports this and batch.py, no more.
    sigserver.py  the signal stage across processes: request layouts, the feeder's `RemoteSignalNormalizer`, the GPU process'
                  `signal_server` threads and what they hand to the batch loop (`SignalResults`, `DeviceBlockPool`).
    stream.py     this file: `HipBackend`, `StreamEngine`, `stream_rank_main` - the GPU process, which alone talks to the device.
"""
from __future__ import annotations

import os
import queue
import threading
import time
from collections import defaultdict
from typing import Dict, Iterable, List, NamedTuple, Tuple

import numpy as np

from .batch import HALF
from .handover import BatchLayout, map_file
# re-exported: every name that tests, tests/cpu_backend.py and tools/ reach as stream.<name> (this file uses some of them itself)
from .batch import Prepared, assemble_rows, rows_from_reads, prepare_batch, _prepare_batch_c, _prepare_batch_py      # noqa: F401
from .handover import feeder_process_main, prepared_from_shm, shm_dir_for, WorkList, _shm_layout_dev              # noqa: F401
from .sigserver import (RemoteSignalNormalizer, SignalResults, DeviceBlockPool, signal_server,                   # noqa: F401
                        _sig_layout, _sig_layout_res, _sig_layout_move)


# ---------------------------------------------------------------------------------------------
# device backend (C ABI) and the rank-local engine
# ---------------------------------------------------------------------------------------------
class HipBackend:
    """The device side of the engine through libdeepmod_hip.so: one model, one in-order stream, NSET staging sets (page-locked
    host memory + device buffers, grow-only), one PositionSummary per contig x strand.  Batch k is copied into set k % NSET
    while the device works on the batches before it; a stream marker per set says when the set may be refilled."""
    NSET = 3

    def __init__(self, moptions, device: int):
        from . import _lib, model as dm
        self._lib = _lib.load()
        self.device = device
        _, init_l, _, _, _, X, Y, _, _, _, _, mfpred = dm.mCreateSession(moptions['fnum'], moptions['hidden'], moptions['windowsize'], moptions)
        self.sess = dm.new_session(device)
        dm.import_meta_graph(moptions['modfile'][0] + '.meta').restore(
            self.sess, dm.latest_checkpoint(moptions['modfile'][1]) or moptions['modfile'][0])
        self.model = self.sess.model
        self.model.set_option(_lib.DM_OPT_ASYNC, 1)
        self._precision = self.model.get_info(_lib.DM_INFO_PRECISION)
        # CUs left to the signal server's kernels (DM_OPT_RESERVED_CUS).  Measured: behind a classifier launch that holds every CU
        # the histogram kernel of a 40-read request takes 1.9 ms instead of 0.15 ms, but with 32 CUs reserved the classifier is
        # 4.5 % slower and the end-to-end rate no better (profiles/r02/README.md): default 0
        self.model.set_option(_lib.DM_OPT_RESERVED_CUS, int(moptions.get('reserved_cus', os.environ.get('DEEPMOD_RESERVED_CUS', 0))))
        self._sets = [{'host': None, 'dev': None, 'sig_block': None} for _ in range(self.NSET)]
        # resident form: set by the engine when signal server threads run in this process (sigserver.SignalResults / DeviceBlockPool)
        self.signal_results = None
        self.signal_blocks = None
        self._k = 0
        self._h2d = self._lib.dm_model_h2d_ahead if int(os.environ.get('DEEPMOD_COPY_AHEAD', 1)) else self._lib.dm_model_h2d_async
        self.timing = defaultdict(float)   # where submit() spends the GPU process' time

    def _staging(self, st, nbytes):
        """(pinned host block, device block) of one set, both at least nbytes (the set's marker has passed: nothing reads them)."""
        if st['host'] is None or st['host'].nbytes < nbytes:
            from . import model as dm
            cap = int(nbytes * 1.25) + 4096
            for blk in (st['host'], st['dev']):
                if blk is not None:
                    blk.free()
            st['host'] = dm.PinnedArray(cap, self.device)
            st['dev'] = dm.DeviceArray((cap,), np.uint8, self.device)
        return st['host'], st['dev']

    def new_summary(self, length: int):
        from . import summary
        s = summary.PositionSummary(length, self.device)
        s.follow(self.model)
        return s

    def submit(self, pb: Prepared, summaries) -> None:
        """Queue one batch: stage, upload, classify every row (windows assembled on the device), accumulate per group.
        Returns after enqueue; the batch's own arrays are free again on return (pb.on_done is called)."""
        from . import _lib
        resident = pb.sig is not None              # the statistics of the batch's events are a device block of the signal stage
        sig_block = self._take_signal(pb) if resident else None
        if pb.n_rows == 0:
            if sig_block is not None:
                self.signal_blocks.give(sig_block)
            self._arrays_free(pb)
            return
        S = 0 if pb.sel is None else len(pb.sel)
        dev_form = pb.ev3 is not None or resident  # raw reads in the device form: the feature rows are built on the device (dm_rows_assemble)
        lay = BatchLayout(pb.n_rows, len(pb.pos), S, ((0 if resident else len(pb.ev3)), len(pb.rdesc)) if dev_form else None)
        n_cls = pb.n_rows if pb.sel is None else max(S, 1)
        t0 = time.perf_counter()
        i = self._k % self.NSET
        self._k += 1
        self.model.wait_mark(i)                    # the launches that read this set (batch k - NSET) are done
        if self._sets[i]['sig_block'] is not None: # ... and with them the statistics block that batch read
            self.signal_blocks.give(self._sets[i]['sig_block'])
        self._sets[i]['sig_block'] = sig_block
        t1 = time.perf_counter()
        host, dev = self._staging(self._sets[i], lay.cls + n_cls)
        self._stage(pb, lay, host)
        t2 = time.perf_counter()
        # on the copy stream: the upload of this batch runs while the device classifies the batches before it (nothing queued reads
        # this set: its marker has passed), and the launches below wait for it
        _lib.check(self._h2d(self.model._h, dev.ptr, host.ptr, lay.end))
        self._classify(pb, lay, dev.ptr, sig_block)
        self._accumulate(pb, lay, dev.ptr, summaries)
        self.model.mark(i)
        t3 = time.perf_counter()
        self.timing['wait_device'] += t1 - t0
        self.timing['stage'] += t2 - t1
        self.timing['launch'] += t3 - t2

    def _take_signal(self, pb: Prepared):
        """The device block of a resident batch's statistics, once its signal request has been served (pb.f32 follows the request's range flag)"""
        from . import _lib
        if self.signal_results is None:
            raise RuntimeError('a batch in the resident form reached a backend without a signal stage')
        t0 = time.perf_counter()
        sig_block, sig_flags, sig_err = self.signal_results.take(pb.sig)
        self.timing['wait_signal'] += time.perf_counter() - t0
        if sig_err is not None:
            raise _lib.DeepModHipError(sig_err)
        if sig_flags & 1:
            pb.f32 = True
        if pb.n_rows and len(pb.rdesc) and (int(pb.rdesc[:, 2].min()) < 0 or 12 * int(pb.rdesc[:, 3].max()) > sig_block.nbytes):
            # (the descriptors and the request come from the same feeder call; a mismatch would be a read outside the block on the device)
            self.signal_blocks.give(sig_block)
            raise RuntimeError('a batch whose read descriptors point outside the statistics of its signal request %r' % (pb.sig,))
        return sig_block

    @staticmethod
    def _arrays_free(pb: Prepared) -> None:
        if pb.on_done is not None:                 # e.g. the feeder's shared-memory slot goes back to its queue
            pb.on_done()
            pb.on_done = None

    def _stage(self, pb: Prepared, lay: BatchLayout, host) -> None:
        """The batch's arrays into the page-locked block of its set, where `lay` puts them; the batch's own arrays are free after that"""
        if lay.dev is None:
            arrays = (pb.rows, pb.pos, pb.flags, pb.sel)       # (a batch without sel has no view for it either)
        else:                                      # the resident form has its statistics on the device already
            arrays = (pb.ev3 if pb.sig is None else None, pb.code, pb.rdesc, pb.pos, pb.flags, pb.sel)
        for dst, src in zip(lay.views(host.view(np.uint8, lay.end)), arrays):
            if src is not None:
                np.copyto(dst, src, casting='same_kind')
        self._arrays_free(pb)

    def _classify(self, pb: Prepared, lay: BatchLayout, d0: int, sig_block) -> None:
        """Assemble the feature rows (device form) and classify them, with the fp32 kernel if the batch asks for it.  d0: the set's device block"""
        from . import _lib
        o, R, S = lay.o, lay.n_rows, lay.n_sel
        d_rows, d_cls = d0 + lay.rows, d0 + lay.cls
        if lay.dev is not None:
            self.model.assemble_rows_device(d_rows, d0 + o['code'], sig_block.ptr if pb.sig is not None else d0 + o['ev3'], d0 + o['rdesc'], lay.dev[1], R)
            self.timing['rows_on_device'] += R
            if pb.sig is not None:
                self.timing['stats_on_device'] += R
        if pb.sel is None:
            # classic form: window centred on row r -> cls[r]; rows 0..9 and R-10..R-1 are padding of the first / last read
            classify = lambda: self.model.predict_rows_device(d_rows, R, HALF, R - 2 * HALF, d_cls + HALF)
        else:
            # compact form: only the windows centred on a base of interest, cls[i] belongs to window sel[i]
            classify = lambda: (self.model.predict_rows_at_device(d_rows, R, d0 + o['sel'], S, d_cls) if S else None)
        if pb.f32 and self._precision != _lib.DM_PREC_F32:      # launches are queued in order: the switch covers this batch only
            self.model.set_option(_lib.DM_OPT_PRECISION, _lib.DM_PREC_F32)
            classify()
            self.model.set_option(_lib.DM_OPT_PRECISION, self._precision)
            self.timing['f32_batches'] += 1
        else:
            classify()
        self.timing['classified'] += (R - 2 * HALF) if pb.sel is None else S

    def _accumulate(self, pb: Prepared, lay: BatchLayout, d0: int, summaries) -> None:
        """Classes and extra rows of every (contig, strand) group of the batch into that group's counters"""
        d_pos, d_flags, d_cls = d0 + lay.o['pos'], d0 + lay.o['flags'], d0 + lay.cls
        xbase = lay.n_rows if pb.sel is None else lay.n_sel
        for g in pb.groups:
            c, s, lo, hi, xlo, xhi = g[:6]
            summ = summaries(c, s, pb.contig_len.get(c, 0))
            if pb.sel is None:
                summ.add_classified_device(d_pos + 8 * lo, d_flags + lo, d_cls + lo, hi - lo)
            elif g[7] > g[6]:
                summ.add_classified_device(d_pos + 8 * g[6], d_flags + g[6], d_cls + g[6], g[7] - g[6])
            if xhi > xlo:
                summ.add_device(d_pos + 8 * (xbase + xlo), d_flags + xbase + xlo, xhi - xlo)

    def sync(self):
        self.model.sync()

    def close(self):
        self.sync()
        for st in self._sets:
            for blk in (st['host'], st['dev']):
                if blk is not None:
                    blk.free()
            if st['sig_block'] is not None and self.signal_blocks is not None:
                self.signal_blocks.give(st['sig_block'])
            st['host'] = st['dev'] = st['sig_block'] = None
        if self.signal_blocks is not None:
            if self.signal_results is not None:         # statistics whose batch never arrived (a feeder that failed after posting its request)
                for key in self.signal_results.pending():
                    self.signal_blocks.give(self.signal_results.take(key, timeout=1.0)[0])
            self.signal_blocks.close()
        self.sess.close()


def finalize_threads(n_tables: int, longest: int, budget_positions: int = 250_000_000) -> int:
    """Tables fetched and formatted side by side by a single rank's finalize: bounded by the positions in flight."""
    return max(1, min(8, n_tables, budget_positions // max(int(longest), 1)))


class _ClusterStage:
    """detect --clusterCpG: the CpG-cluster stage of a contig from its two counter tables while they are still on the device
    (ClusterModel.sites: dm_cluster_sites) - what sum_chr_mod.py, generate_motif_pos.py and hm_cluster_predict.py compute from the BED
    files of the run - written as `<outFolder>_clusterCpG.<chr>.<Base>.bed` (outFolder = `<command-line folder>/<FileID>`, the tools' prefix).
    A contig without a site gets no file, as with the tools."""

    class Table(NamedTuple):
        """One strand's counters of the contig in work, kept open until its pair has been through the stage."""
        summary: object
        first: int                           # the positions this rank holds of it: [first, first + count)
        count: int
        edges: list                          # cluster.slice_edges of a slice (its first and last 26 cov | mod values); None for a whole table

    def __init__(self, engine, gather, scattered: bool):
        from . import cluster
        self.eng, self.gather, self.cluster, self.scattered = engine, gather, cluster, scattered
        self.mo = engine.mo
        self._model = None
        self.parts = {}                      # contig -> [bytes of this rank's '+' part, of its '-' part]
        self.contig, self.tables = None, {}  # the contig in work and its Table per strand

    @property
    def model(self):
        """Loaded by the first contig this rank computes: a rank that only hands its counters to rank 0 never loads it."""
        if self._model is None:
            self._model = self.cluster.ClusterModel.from_checkpoint(self.mo['clusterCpG'], getattr(self.eng.backend, 'device', 0))
        return self._model

    def path(self, chrom: str) -> str:
        return '%s_clusterCpG.%s.%s.bed' % (self.mo['outFolder'].rstrip('/'), chrom, self.mo['Base'])

    def _seq(self, chrom: str) -> str:
        from . import readmap
        seqs = readmap.read_fasta(self.mo['Ref'])          # (parsed once per process: the rank read it for the contig lengths, and this is that dict)
        if chrom not in seqs:
            raise RuntimeError('--clusterCpG: contig %r of the run is not in --Ref %s' % (chrom, self.mo['Ref']))
        return seqs[chrom]

    def keep(self, chrom: str, strand: str, summary, first: int = 0, count=None, cov=None, mod=None) -> None:
        """Takes a table over instead of closing it.  Tables arrive contig by contig ('+' before '-'); the first table of the next contig sends the
        pair before it through the stage.  cov, mod: the host copy of a slice, for its edges."""
        if self.contig is not None and self.contig != chrom:
            self.flush()
        self.contig = chrom
        edges = self.cluster.slice_edges(cov, mod, None, None)[0] if cov is not None else None
        self.tables[strand] = self.Table(summary, int(first), int(summary.length if count is None else count), edges)

    def flush(self) -> None:
        """The pair in work through the stage, then its tables are closed.  A strand without a table counts as zeros."""
        if self.contig is None:
            return
        chrom, plus, minus = self.contig, self.tables.get('+'), self.tables.get('-')
        self.contig, self.tables = None, {}
        some = plus or minus
        if self.scattered:
            self.sliced(chrom, plus and plus.summary, minus and minus.summary, some.first, some.count,
                        [t.edges if t else [[[], []], [[], []]] for t in (plus, minus)])
        elif self.eng.rank == 0:
            self.whole(chrom, plus and plus.summary, minus and minus.summary)
        for t in (plus, minus):
            if t:
                t.summary.close()

    def finish(self) -> None:
        self.flush()
        if self.scattered:
            self.join()
        if self._model is not None:
            self._model.close()

    def whole(self, chrom: str, plus, minus) -> None:
        """One rank holds the whole tables (either may be None)."""
        res = self.model.sites(plus, minus, self._seq(chrom))
        self.eng.stats['cluster_sites'] += len(res['pos'])
        if len(res['pos']):
            with open(self.path(chrom), 'wb') as fh:
                fh.write(b''.join(self.cluster.site_text_parts(chrom, self.mo['Base'], res)))

    def sliced(self, chrom: str, plus, minus, first: int, count: int, edges) -> None:
        """After the reduce-scatter: this rank's slice [first, first + count) of both strands; the 26 counters beyond either end come from
        the edges every rank publishes through the control plane, the bases from this rank's slice +- 27 of the sequence."""
        mine = {"first": int(first), "count": int(count), "edges": edges}
        everyone = self.gather({"cluster": mine}) if self.eng.world > 1 else [{"cluster": mine}]
        halo = self.cluster.halo_from_edges(first, count, [e["cluster"] for e in everyone])
        seq = self._seq(chrom)
        lo, hi = max(0, first - self.cluster.HALO - 1), min(len(seq), first + count + self.cluster.HALO + 1)
        res = self.model.sites(plus, minus, seq[lo:max(lo, hi)], first, count, from_slice=True, halo=halo, seq_first=lo)
        self.eng.stats['cluster_sites'] += len(res['pos'])
        sizes = []
        for name, text in zip(('plus', 'minus'), self.cluster.site_text_parts(chrom, self.mo['Base'], res)):
            with open('%s.%s.part%d' % (self.path(chrom), name, self.eng.rank), 'wb') as fh:
                fh.write(text)
            sizes.append(len(text))
        self.parts[chrom] = sizes

    def join(self) -> None:
        """Rank 0: all '+' parts of a contig in rank order, then all '-' parts - the order of the tools' file."""
        world = self.eng.world
        sizes = self.gather({"cluster_parts": self.parts}) if world > 1 else [{"cluster_parts": self.parts}]
        if self.eng.rank != 0:
            return
        for chrom in sorted(self.parts):
            names = ['%s.%s.part%d' % (self.path(chrom), name, r) for name in ('plus', 'minus') for r in range(world)]
            want = [sizes[r]["cluster_parts"].get(chrom, [0, 0])[k] for k in range(2) for r in range(world)]
            _join_parts(self.path(chrom), names, want, 'clusterCpG')


def _join_parts(path: str, names: List[str], sizes: List[int], what: str) -> bool:
    """Rank 0: the ranks' part files `names`, in that order, become the file `path` - if they hold anything at all - and are removed.  A part must
    have the size its rank reported.  -> True if the file was written"""
    written = sum(sizes) > 0
    if written:
        with open(path, 'wb') as out:
            for nm, size in zip(names, sizes):
                with open(nm, 'rb') as fh:
                    data = fh.read()
                if len(data) != size:
                    raise RuntimeError('%s part %s has %d bytes, its rank reported %d' % (what, nm, len(data), size))
                out.write(data)
    for nm in names:
        if os.path.exists(nm):
            os.remove(nm)
    return written


class StreamEngine:
    """Rank-local streaming detect: pulls worker batches, keeps per contig x strand counters, merges at the end."""

    def __init__(self, moptions, backend, rank: int = 0, world: int = 1):
        self.mo, self.backend, self.rank, self.world = moptions, backend, rank, world
        self.summaries = {}
        self.ref_len: Dict[str, int] = {}
        self.errors: Dict[str, List[str]] = defaultdict(list)
        self.stats = defaultdict(float)

    def _summary(self, chrom: str, strand: str, need_len: int):
        """The counters of one contig x strand, at least need_len positions long.  With a reference length (FASTA or
        container metadata) they are allocated once; otherwise they grow geometrically as reads reach further."""
        key = (chrom, strand)
        want = max(self.ref_len.get(chrom, 0), need_len, 1)
        s = self.summaries.get(key)
        if s is None:
            s = self.summaries[key] = self.backend.new_summary(want)
        elif s.length < want:
            s.grow(want if chrom in self.ref_len else int(want * 1.5))
        return s

    def set_reference_lengths(self, lengths: Dict[str, int]):
        for c, ln in lengths.items():
            self.ref_len[c] = max(self.ref_len.get(c, 0), int(ln))

    def consume(self, pb: Prepared):
        t0 = time.perf_counter()
        for k, v in pb.errors.items():
            self.errors[k].extend(v)
        self.backend.submit(pb, self._summary)
        self.stats['submit'] += time.perf_counter() - t0
        self.stats['windows'] += pb.n_windows
        self.stats['rows'] += pb.n_rows
        self.stats['reads'] += pb.n_reads
        self.stats['batches'] += 1
        for k, v in pb.timing.items():
            self.stats['prep_' + k] += v

    def run(self, batches: Iterable, feeders: int = 2, make_normalizer=None):
        """batches: iterable of file lists (a shared queue drained by all ranks, or this rank's static shard).
        `feeders` threads prepare batches ahead of the device queue (numpy / zlib / the C ABI release the GIL)."""
        t_start = time.perf_counter()
        it = iter(batches)
        lock = threading.Lock()
        ready: "queue.Queue" = queue.Queue(maxsize=max(2, feeders))
        tl = threading.local()

        def normalizer():
            if make_normalizer is None:
                return None
            if not hasattr(tl, 'norm'):
                tl.norm = make_normalizer()
            return tl.norm

        def feed():
            while True:
                with lock:
                    try:
                        files = next(it)
                    except StopIteration:
                        files = None
                if files is None:
                    ready.put(None)
                    return
                try:
                    ready.put(prepare_batch(self.mo, files, normalizer))
                except BaseException as exc:      # surfaces in the consumer: a failed batch must not be dropped silently
                    ready.put(exc)
                    return

        threads = [threading.Thread(target=feed, daemon=True) for _ in range(max(1, feeders))]
        for t in threads:
            t.start()
        done = 0
        while done < len(threads):
            t0 = time.perf_counter()
            item = ready.get()
            self.stats['wait_feed'] += time.perf_counter() - t0
            if item is None:
                done += 1
            elif isinstance(item, BaseException):
                raise item
            else:
                self.consume(item)
        self._drain_device()
        self._end_of_run(t_start)

    def _drain_device(self) -> None:
        t0 = time.perf_counter()
        self.backend.sync()
        self.stats['drain'] += time.perf_counter() - t0

    def _end_of_run(self, t_start: float) -> None:
        self.stats['detect_wall'] += time.perf_counter() - t_start
        for k, v in getattr(self.backend, 'timing', {}).items():
            self.stats['submit_' + k] += v

    def run_processes(self, work, n_procs: int, device: int, ctx=None, make_backend=None):
        """Same as run(), with the batches prepared by `n_procs` feeder processes that drain `work` (a multiprocessing queue
        of (files, ...) items shared by all ranks and filled before the run starts).  make_backend: create the device backend
        only after the feeders have been started, so that they prepare the first batches while the model loads."""
        import multiprocessing
        import shutil
        t_start = time.perf_counter()
        ctx = ctx or multiprocessing.get_context('spawn')
        shm_dir = shm_dir_for(self.mo)
        os.makedirs(shm_dir, exist_ok=True)
        ready = ctx.Queue(maxsize=max(4, 2 * n_procs))
        slot_bytes, free_slots, slot_buffer = self._hand_over_slots(ctx, shm_dir, n_procs)
        sig = None
        if self.mo.get('signal_server', True) and (make_backend is not None or hasattr(self.backend, 'device')):
            sig = self._start_signal_servers(ctx, n_procs, device)
        procs = [ctx.Process(target=feeder_process_main, daemon=True,
                             args=(self.mo, work, ready, device, shm_dir, i, free_slots, slot_bytes, sig and sig['requests'],
                                   sig['answers'][i] if sig else None)) for i in range(n_procs)]
        for pr in procs:
            pr.start()
        self.stats['at_feeders_started'] = time.perf_counter() - t_start
        clean = False
        try:
            if make_backend is not None:
                t0 = time.perf_counter()
                self.backend = make_backend()
                self.stats['backend_init'] += time.perf_counter() - t0
            if sig is not None and hasattr(self.backend, 'signal_results'):
                self.backend.signal_results, self.backend.signal_blocks = sig['results'], sig['blocks']
            self.stats['at_backend_ready'] = time.perf_counter() - t_start
            self._consume_ready(ready, procs, slot_buffer, free_slots, t_start)
            self.stats['at_last_batch'] = time.perf_counter() - t_start
            self._drain_device()
            self.stats['at_drained'] = time.perf_counter() - t_start
            clean = True
        finally:
            for pr in procs:
                if clean:                # every feeder has sent its end marker: it is on its way out
                    pr.join(timeout=10)
                if pr.is_alive():        # the run is failing (or a feeder hangs): feeders may be blocked on a queue for good
                    pr.terminate()
            if sig is not None:
                for _ in sig['threads']:
                    sig['requests'].put(None)
                for th in sig['threads']:
                    th.join(timeout=10)
            shutil.rmtree(shm_dir, ignore_errors=True)
        self.stats['at_feeders_gone'] = time.perf_counter() - t_start
        self._end_of_run(t_start)

    def _hand_over_slots(self, ctx, shm_dir: str, n_procs: int):
        """-> (slot_bytes, free_slots, slot_buffer).  Hand-over slots: files in shm_dir, mapped once by both sides, that the feeders fill and this
        process copies into its page-locked staging memory (an upload straight from a shared-memory mapping ran at 0.7 GB/s, and page-locking the
        mapping itself faulted the GPU).  A batch larger than a slot falls back to a file of its own.  free_slots: the queue of slot numbers the
        feeders take from (None: no slots, every batch in a file of its own); slot_buffer(i): the mapping of slot i, made on first use."""
        slot_bytes = int(self.mo.get('feeder_slot_mb', 128)) << 20
        n_slots = n_procs + 4 if self.mo.get('feeder_slots', True) else 0
        try:
            st = os.statvfs(shm_dir)
            n_slots = min(n_slots, int(0.5 * st.f_bavail * st.f_frsize) // slot_bytes)
        except OSError:
            n_slots = 0
        slots, free_slots = {}, None
        if n_slots >= 4:
            free_slots = ctx.Queue()
            for i in range(n_slots):
                fd = os.open(os.path.join(shm_dir, 'slot_%d' % i), os.O_CREAT | os.O_RDWR | os.O_TRUNC, 0o600)
                os.ftruncate(fd, slot_bytes)
                os.close(fd)
                free_slots.put(i)

        def slot_buffer(i):
            if i not in slots:
                slots[i] = map_file(os.path.join(shm_dir, 'slot_%d' % i), slot_bytes)
            return slots[i]

        return slot_bytes, free_slots, slot_buffer

    def _start_signal_servers(self, ctx, n_procs: int, device: int):
        """The signal stage of this process' feeders: the request queue, an answer queue per feeder, what the threads hand to the batch loop,
        and the started threads - each with its own dm_signal handle / stream"""
        sig = {'requests': ctx.Queue(), 'answers': [ctx.Queue() for _ in range(n_procs)], 'results': SignalResults(), 'blocks': DeviceBlockPool(device)}
        n_threads = max(1, int(self.mo.get('signal_servers', os.environ.get('DEEPMOD_SIGNAL_SERVERS', 2))))
        sig['threads'] = [threading.Thread(target=signal_server, daemon=True,
                                           args=(sig['requests'], sig['answers'], device, self.stats, sig['results'], sig['blocks'])) for _ in range(n_threads)]
        for th in sig['threads']:
            th.start()
        return sig

    def _consume_ready(self, ready, procs, slot_buffer, free_slots, t_start: float) -> None:
        """The batch loop of run_processes: descriptions from `ready` until every feeder has sent its end marker"""
        done = 0
        while done < len(procs):
            t0 = time.perf_counter()
            try:
                item = ready.get(timeout=5.0)
            except queue.Empty:
                if not any(pr.is_alive() for pr in procs) and ready.empty():
                    raise RuntimeError('feeder processes ended without finishing their batches (exit codes %s)'
                                       % [pr.exitcode for pr in procs])
                self.stats['wait_feed'] += time.perf_counter() - t0
                continue
            self.stats['wait_feed'] += time.perf_counter() - t0
            if item is None:
                done += 1
            elif 'failed' in item:
                raise RuntimeError('a feeder process failed:\n' + item['failed'])
            else:
                self.stats.setdefault('at_first_batch', time.perf_counter() - t_start)
                pb = prepared_from_shm(item, slot_buffer)
                if item.get('slot') is not None:
                    pb.on_done = (lambda i=item['slot']: free_slots.put(i))
                    self.stats['slot_batches'] += 1
                self.consume(pb)

    def finalize(self, gather, scatter_fn=None, write: bool = True, reduce_fn=None) -> Dict[Tuple[str, str], bytes]:
        """Merge over ranks and write the BED files.
        gather(obj) -> list of every rank's obj (control plane).  Data plane, world > 1:
          * scatter_fn(summary) -> (first, count): the summary's counters are summed over the ranks and THIS rank is left with the
            slice [first, first + count) (dm_summary_reduce_scatter).  Every rank fetches and formats its slice and writes it as a
            part file; rank 0 concatenates the parts in rank order (BED lines are sorted by position, so that IS the file).  No rank
            ever holds, downloads or formats a whole contig - for a human genome that is 74 GB of counters and 6e8 lines.
          * reduce_fn(summary) (fallback when no scatter_fn is given): sum into rank 0, which fetches and formats everything.
        All ranks walk the union of contig x strand keys in the same order.  Returns the BED bytes rank 0 assembled."""
        t0 = time.perf_counter()
        mine = {"%s\t%s" % k: self.summaries[k].length for k in self.summaries}
        lens = dict(self.ref_len)
        everyone = gather({"keys": mine, "len": lens}) if self.world > 1 else [{"keys": mine, "len": lens}]
        keys = sorted(set(k for e in everyone for k in e["keys"]))
        beds, parts = {}, {}
        # (moptions['force_scatter_merge']: the scatter form on a single rank too - how the GPU tests run this code path on one GPU)
        scattered = scatter_fn is not None and (self.world > 1 or bool(self.mo.get('force_scatter_merge')))
        # --clusterCpG: both strands of a contig go through the cluster stage as a pair, before either table is closed
        stage = _ClusterStage(self, gather, scattered) if (self.mo.get('clusterCpG') and write) else None
        if not scattered and self.world == 1 and len(keys) >= 1:
            self._merge_single_rank(keys, lens, stage, write, beds)
            keys = []
        for key in keys:
            chrom, strand = key.split("\t")
            length = max([e["keys"].get(key, 0) for e in everyone] + [e["len"].get(chrom, 0) for e in everyone])
            if stage is not None:
                length = max([length] + [e["keys"].get("%s\t%s" % (chrom, st), 0) for e in everyone for st in '+-'])    # common to both strands
            s = self.summaries.get((chrom, strand))
            if s is None:                               # this rank saw no read of that contig x strand: zeros
                s = self.summaries[(chrom, strand)] = self.backend.new_summary(length)
            s.grow(length)                              # exactly the common length (no growth slack): equal counts on every rank
            if scattered:
                self._scatter_table(key, s, scatter_fn, stage, write, beds, parts)
            else:
                self._reduce_table(key, s, reduce_fn, stage, write, beds)
            if stage is None:
                s.close()
        self.summaries = {}
        if stage is not None:
            stage.finish()
        if scattered and write:
            # every rank's parts are on disk once its sizes have been gathered; rank 0 joins them
            sizes = gather({"parts": parts}) if self.world > 1 else [{"parts": parts}]
            if self.rank == 0:
                for key in keys:
                    path = self._bed_path(*key.split("\t"))
                    if _join_parts(path, [path + '.part%d' % r for r in range(self.world)], [e["parts"].get(key, 0) for e in sizes], 'BED'):
                        beds[tuple(key.split("\t"))] = None      # (the reference writes no file for an empty table, myDetect.py:1109)
        self.stats['merge+bed'] += time.perf_counter() - t0
        return beds

    def _bed_path(self, chrom: str, strand: str) -> str:
        return '%s/mod_pos.%s%s.%s.bed' % (self.mo['outFolder'], chrom, strand, self.mo['Base'])

    def _fetch_format_write(self, key: str, write: bool):
        """one rank, one table: download the counters, format, write (all outside the interpreter lock) -> (BED bytes or None: written to its file, bytes written)"""
        from . import summary as dmsum
        chrom, strand = key.split("\t")
        s = self.summaries[(chrom, strand)]
        touch, cov, mod = s.fetch()
        s.close()
        if not write:
            return dmsum.bed_lines(chrom, strand, self.mo['Base'], touch, cov, mod), 0
        # slices of the table formatted side by side and written in order; the text of a large contig is never held whole
        fh, nbytes = None, 0
        for part in dmsum.bed_parts(chrom, strand, self.mo['Base'], touch, cov, mod):
            if fh is None:                      # the reference writes no file for an empty table (myDetect.py:1109)
                fh = open(self._bed_path(chrom, strand), 'wb')
            fh.write(part)
            nbytes += len(part)                 # (summed by the caller: several of these run side by side)
        if fh is not None:
            fh.close()
        return (b'' if fh is None else None), nbytes

    def _merge_single_rank(self, keys, lens, stage, write: bool, beds) -> None:
        """A single rank: the tables are independent (own counters, own stream, own file) - contig x strand tables side by side"""
        from concurrent.futures import ThreadPoolExecutor
        for key in keys:
            chrom, strand = key.split("\t")
            self.summaries[(chrom, strand)].grow(max(self.summaries[(chrom, strand)].length, lens.get(chrom, 0)))
        if stage is not None:
            for chrom in sorted(set(key.split("\t")[0] for key in keys)):
                pair = [self.summaries.get((chrom, st)) for st in '+-']
                for s in pair:
                    if s is not None:
                        s.grow(max(t.length for t in pair if t is not None))      # one common length
                stage.whole(chrom, *pair)
        # a table in flight holds 3 x length int32 on the host plus its text: at most ~2.5e8 positions (3 GB of counters) at a time,
        # i.e. eight E. coli-sized tables side by side but one chr1-sized table after the other
        longest = max(self.summaries[tuple(key.split("\t"))].length for key in keys)
        with ThreadPoolExecutor(finalize_threads(len(keys), longest)) as pool:
            for key, (bed, nbytes) in zip(keys, pool.map(lambda key: self._fetch_format_write(key, write), keys)):
                beds[tuple(key.split("\t"))] = bed
                self.stats['bed_bytes'] += nbytes

    def _scatter_table(self, key: str, s, scatter_fn, stage, write: bool, beds, parts) -> None:
        """Reduce-scatter: this rank's slice of the all-rank sums, as a part file (parts[key]: its size) or, without `write`, as beds[key]"""
        from . import summary as dmsum
        chrom, strand = key.split("\t")
        s.sync()                                # every rank: positions this rank dropped as out of range fail the run here
        first, count = scatter_fn(s)
        touch, cov, mod = s.fetch_slice()
        if stage is not None:
            stage.keep(chrom, strand, s, first, count, cov, mod)
        if write:
            parts[key] = 0
            with open(self._bed_path(chrom, strand) + '.part%d' % self.rank, 'wb') as fh:
                for part in dmsum.bed_parts(chrom, strand, self.mo['Base'], touch, cov, mod, first_pos=first):
                    fh.write(part)
                    parts[key] += len(part)
        else:
            part = dmsum.bed_lines(chrom, strand, self.mo['Base'], touch, cov, mod, first_pos=first)
            parts[key] = len(part)
            beds[(chrom, strand)] = part        # (tests: the caller joins the ranks' parts itself)
        self.stats['bed_bytes'] += parts[key]

    def _reduce_table(self, key: str, s, reduce_fn, stage, write: bool, beds) -> None:
        """Reduce to rank 0, which fetches, formats and writes the whole table"""
        from . import summary as dmsum
        chrom, strand = key.split("\t")
        if self.world > 1:
            s.sync()
            reduce_fn(s)
        if self.rank == 0:
            touch, cov, mod = s.fetch()
            bed = dmsum.bed_lines(chrom, strand, self.mo['Base'], touch, cov, mod)
            beds[(chrom, strand)] = bed
            if write and len(bed) > 0:          # the reference writes no file for an empty table (myDetect.py:1109)
                with open(self._bed_path(chrom, strand), 'wb') as fh:
                    fh.write(bed)
        if stage is not None:
            stage.keep(chrom, strand, s)


# ---------------------------------------------------------------------------------------------
# process entry: one rank = one GPU
# ---------------------------------------------------------------------------------------------


def _drain(q):
    while True:
        try:
            item = q.get(block=False)
        except Exception:
            return
        yield item[0]


def stream_rank_main(moptions, rank: int, world: int, device: int, work, result_q=None, feeders: int = 2, feeder_procs: int = 0):
    """Body of one GPU process.  `work`: a shared queue of (files, subfolder, batchid) items drained by all ranks,
    or a list of file lists (static shard).  feeder_procs > 0 (queue only): batches are prepared by that many feeder
    processes of this rank; otherwise by `feeders` threads.  Returns / posts {'errors', 'stats'}."""
    from . import comm as dmcomm
    rdv = None
    if world > 1:       # collectively, before any work: a rank that cannot join fails the run at once, not after its share of the reads
        rdv = dmcomm.FileRendezvous(os.path.join(moptions['outFolder'], '.rendezvous'), rank, world)
    try:
        return _stream_rank_body(moptions, rank, world, device, work, result_q, feeders, feeder_procs, rdv)
    except BaseException as exc:
        if rdv is not None:
            rdv.abort('%s: %s' % (type(exc).__name__, exc))      # the other ranks stop waiting for this one within milliseconds
        raise


def _stream_rank_body(moptions, rank, world, device, work, result_q, feeders, feeder_procs, rdv):
    from . import comm as dmcomm, signal as dmsignal
    communicator = None
    if world > 1:
        communicator = dmcomm.Communicator.from_rendezvous(device, rdv)
        if rank == 0 and moptions.get('outLevel', 2) <= 1:      # --outLevel 0 / 1: which collective library merges the counters of this run
            path, version = dmcomm.rccl_info()
            print('RCCL: %d ranks over %s (ncclGetVersion %d%s)' % (world, path, version, '; DEEPMOD_RCCL_LIBRARY' if os.environ.get('DEEPMOD_RCCL_LIBRARY') else ''), flush=True)
    use_procs = feeder_procs > 0 and hasattr(work, 'get')
    backend = None if use_procs else HipBackend(moptions, device)       # with feeder processes: created once they are running
    eng = StreamEngine(moptions, backend, rank, world)
    if moptions.get('_t_manager'):
        eng.stats['at_rank_start'] = time.time() - moptions['_t_manager']     # process start-up + imports of this rank
    if moptions.get('Ref') and os.path.isfile(moptions['Ref']):
        from . import readmap
        eng.set_reference_lengths({c: len(s) for c, s in readmap.read_fasta(moptions['Ref']).items()})
    if use_procs:
        eng.run_processes(work, feeder_procs, device, make_backend=lambda: HipBackend(moptions, device))
        backend = eng.backend
    else:
        batches = _drain(work) if hasattr(work, 'get') else iter(work)
        eng.run(batches, feeders=feeders, make_normalizer=lambda: dmsignal.SignalNormalizer(device))
    if communicator is not None:
        rounds = iter(range(1 << 30))
        gather = lambda obj: rdv.all_gather_json('finalize_%d' % next(rounds), obj)
        scatter_fn = lambda s: s.reduce_scatter(communicator)
    else:
        gather = scatter_fn = None
    eng.finalize(gather, scatter_fn)
    if moptions.get('_t_manager'):
        eng.stats['at_bed_written'] = time.time() - moptions['_t_manager']
    if communicator is not None:
        eng.stats.update({'comm_' + k: v for k, v in communicator.stats().items()})
        communicator.close()
    backend.close()
    if moptions.get('_t_manager'):
        eng.stats['at_rank_end'] = time.time() - moptions['_t_manager']
    out = {'rank': rank, 'errors': dict(eng.errors), 'stats': dict(eng.stats)}
    if result_q is not None:
        result_q.put(out)
    return out
