"""Batch backends for the streaming driver (cli.py).

``DeviceStream`` is the product path: host batches live in pinned memory
(``dcr_host_alloc``), each ``submit`` is one asynchronous ``dcr_submit``
(H2D on a copy stream, the kernels on the compute stream, D2H of the fields
the writer needs on a second copy stream) and ``result`` waits for that
slot only, so the ingest of batch k+1 and the writing of batch k-1 overlap
the device work of batch k (north_star: "a writer that streams results back
through hipMemcpyAsync on side streams").

``CallBackend`` wraps a synchronous ``(packed, params) -> (ss, ds, info)``
callable (the C oracle in CPU tests, test infrastructure only).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import native_io
from .batch import DcrOut, OUT_COLS, OUT_SCALARS

# fields of the single-strand results the writer reads (dcr_fmt_out); pos,
# n_cig and cigar of single-strand records stay on the device unless the
# single-strand records themselves are written (SS_FIELDS_FULL)
SS_FIELDS = ("status", "mapq", "len", "n_de", "D", "M", "E", "seq", "qual", "d", "e")
SS_FIELDS_FULL = SS_FIELDS + ("pos", "n_cig", "cigar")
DS_FIELDS = tuple(OUT_SCALARS) + tuple(OUT_COLS)


class Pinned:
    """A pinned host allocation (hipHostMalloc) viewed as a uint8 numpy array."""

    def __init__(self, lib, nbytes):
        self._lib = lib
        self.nbytes = max(int(nbytes), 16)
        self.ptr = lib.dcr_host_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError(f"dcr_host_alloc({self.nbytes}) failed")
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * self.nbytes).from_address(self.ptr))

    def free(self):
        if self.ptr:
            self._lib.dcr_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pinned_allocator(lib, keep):
    def alloc(nbytes):
        p = Pinned(lib, nbytes)
        keep.append(p)
        return p.array
    return alloc


class _HostOut:
    """Pinned host arrays receiving one slot's outputs (grow-only)."""

    def __init__(self, lib):
        self.lib = lib
        self.cap = None
        self.mem = None
        self.arr = {}

    def ensure(self, n_ss, c_ss, n_ds, c_ds, n_reads, ss_fields=SS_FIELDS):
        need = (n_ss, c_ss, n_ds, c_ds, n_reads)
        if self.cap is not None and all(a >= b for a, b in zip(self.cap, need)) and \
                set(self.arr["ss"]) == set(ss_fields):
            return
        cap = tuple(int(max(b, 1) * 1.25) + 64 for b in need)
        specs = []
        for kind, fields, nrec, ncol in (("ss", ss_fields, cap[0], cap[1]), ("ds", DS_FIELDS, cap[2], cap[3])):
            for k in fields:
                dt = OUT_SCALARS.get(k) or OUT_COLS[k]
                specs.append((kind, k, np.dtype(dt), nrec if k in OUT_SCALARS else ncol))
        specs.append(("rs", "status", np.dtype(np.int32), cap[4]))
        total = sum(((dt.itemsize * n + 255) & ~255) for _, _, dt, n in specs)
        if self.mem is not None:
            self.mem.free()
        self.mem = Pinned(self.lib, total)
        self.arr = {"ss": {}, "ds": {}, "rs": {}}
        off = 0
        for kind, k, dt, n in specs:
            self.arr[kind][k] = self.mem.array[off:off + dt.itemsize * n].view(dt)
            off += (dt.itemsize * n + 255) & ~255
        self.cap = cap

    def dcr_out(self, kind):
        o = DcrOut()
        for k, _ in DcrOut._fields_:
            a = self.arr[kind].get(k)
            setattr(o, k, a.ctypes.data if a is not None else None)
        return o

    def fmt_out(self, kind):
        o = native_io.FmtOut()
        for k, _ in native_io.FmtOut._fields_:
            a = self.arr[kind].get(k)
            setattr(o, k, a.ctypes.data if a is not None else None)
        return o


class WMeta(ctypes.Structure):
    _fields_ = [("names", ctypes.c_void_p), ("n_names", ctypes.c_int64), ("fam_code", ctypes.c_void_p),
                ("fam_rx", ctypes.c_void_p), ("fam_tid", ctypes.c_void_p)]


class WMetaSs(ctypes.Structure):
    _fields_ = [("sub_flag", ctypes.c_void_p), ("sub_mi", ctypes.c_void_p), ("sub_rx", ctypes.c_void_p)]


class WRes(ctypes.Structure):
    _fields_ = [("bgzf", ctypes.c_void_p), ("cap_bgzf", ctypes.c_int64), ("fam_fail", ctypes.c_void_p),
                ("ds_len", ctypes.c_void_p), ("totals", ctypes.c_void_p)]


class _WriterOut:
    """Pinned host arrays of one slot's device-writer results (grow-only)."""

    def __init__(self, lib):
        self.lib = lib
        self.cap_f = 0
        self.cap_b = 0
        self.small = None
        self.blocks = None

        self.filt = None                 # pinned fam_filt, made when a filter is first set
        self.met = None                  # pinned dcr_metrics, made when metrics are first on
        self.bmet = None                 # pinned dcr_base_metrics, made when base metrics are first on
        self.ovl = None                  # pinned fam_ovl, made when --mate_overlap is first set
        self.gmet = None                 # pinned dcr_genome_metrics, made when a genome is first set

    def ensure(self, n_fam, bgzf_bytes, filt=False, met=False, bmet=False, ovl=False, gmet=False):
        if n_fam > self.cap_f or self.small is None:
            self.cap_f = int(n_fam * 1.25) + 64
            self.small = Pinned(self.lib, 12 * self.cap_f + 64)
            a = self.small.array
            self.fam_fail = a[:4 * self.cap_f].view(np.int32)
            self.ds_len = a[4 * self.cap_f:12 * self.cap_f].view(np.int32)
            self.totals = a[12 * self.cap_f:12 * self.cap_f + 24].view(np.int64)
        if filt and (self.filt is None or self.filt.nbytes < 4 * self.cap_f):
            self.filt = Pinned(self.lib, 4 * self.cap_f)
            self.fam_filt = self.filt.array.view(np.int32)
        if ovl and (self.ovl is None or self.ovl.nbytes < 12 * self.cap_f):
            if self.ovl is not None:
                self.ovl.free()
            self.ovl = Pinned(self.lib, 12 * self.cap_f)
            self.fam_ovl = self.ovl.array.view(np.int32)
        if met and self.met is None:
            from .params import MET_WORDS
            self.met = Pinned(self.lib, 8 * MET_WORDS)
            self.metrics = self.met.array[:8 * MET_WORDS].view(np.uint64)
        if bmet and self.bmet is None:
            from .params import BMET_WORDS
            self.bmet = Pinned(self.lib, 8 * BMET_WORDS)
            self.base_metrics = self.bmet.array[:8 * BMET_WORDS].view(np.uint64)
        if gmet and self.gmet is None:
            from .params import GMET_WORDS
            self.gmet = Pinned(self.lib, 8 * GMET_WORDS)
            self.genome_metrics = self.gmet.array[:8 * GMET_WORDS].view(np.uint64)
        if bgzf_bytes > self.cap_b:
            self.cap_b = int(bgzf_bytes * 1.25) + (1 << 20)
            self.blocks = Pinned(self.lib, self.cap_b)

    def wres(self):
        r = WRes()
        r.bgzf, r.cap_bgzf = self.blocks.ptr, self.cap_b
        r.fam_fail, r.ds_len, r.totals = self.fam_fail.ctypes.data, self.ds_len.ctypes.data, self.totals.ctypes.data
        return r


class WriterResult:
    """One batch through the device writer: per-family outcomes (0: written),
    duplex lengths, and the BGZF blocks of the records of every family that
    does not fail.  With the single-strand stream (dcr_submit_write_ss) also
    ``ss_bgzf`` / ``ss_record_bytes``: the blocks of those families' four
    single-strand records; None without it.  With a consensus filter set
    ``fam_filt``: the per-family outcome words (low byte not 0: dropped, its
    records are not in the streams); None without one.  With ``metrics`` on,
    ``metrics``: the batch's dcr_metrics as uint64 words (the slot's pinned
    block, overwritten when the slot is submitted again); None without.  With
    ``base_metrics`` on, ``base_metrics``: the batch's dcr_base_metrics in the
    same way; None without.  With ``mate_overlap`` set, ``fam_ovl``: compared,
    disagree, changed per family (int32 [3 * n_fam]); None without.  With a
    genome set, ``genome_metrics``: the batch's dcr_genome_metrics as the other
    blocks; None without."""

    def __init__(self, stream, slot, out, n_fam, out_ss=None, filtered=False, metrics=False, base_metrics=False,
                 overlap=False, genome=False):
        self._stream, self._slot = stream, slot
        self.fam_fail = out.fam_fail[:n_fam]
        self.fam_filt = out.fam_filt[:n_fam] if filtered else None
        self.metrics = out.metrics if metrics else None
        self.base_metrics = out.base_metrics if base_metrics else None
        self.fam_ovl = out.fam_ovl[:3 * n_fam] if overlap else None
        self.genome_metrics = out.genome_metrics if genome else None
        self.ds_len = out.ds_len[:2 * n_fam]
        self.bgzf_bytes, self.record_bytes, self.blocks = (int(x) for x in out.totals[:3])
        self.bgzf = out.blocks.array[:self.bgzf_bytes]
        self.ss_bgzf = self.ss_record_bytes = None
        if out_ss is not None:
            self.ss_bgzf_bytes, self.ss_record_bytes, self.ss_blocks = (int(x) for x in out_ss.totals[:3])
            self.ss_bgzf = out_ss.blocks.array[:self.ss_bgzf_bytes]

    def _fetch_records(self, what_off, what_bytes, n_rec):
        lib, ctx = self._stream.lib, self._stream.ctx._ctx
        from . import _lib
        end = np.zeros(1, np.int64)
        _lib._check(lib.dcr_slot_fetch(ctx, self._slot, what_off, n_rec, 1, end.ctypes.data))
        buf = np.zeros(max(int(end[0]), 1), np.uint8)
        _lib._check(lib.dcr_slot_fetch(ctx, self._slot, what_bytes, 0, int(end[0]), buf.ctypes.data))
        return buf[:int(end[0])]

    def record_bytes_of(self, n_fam):
        """Formatted records of families [0, n_fam) (fetched from the device slot)."""
        return self._fetch_records(1, 0, 2 * n_fam)

    def ss_record_bytes_of(self, n_fam):
        """Formatted single-strand records of families [0, n_fam)."""
        return self._fetch_records(4, 3, 4 * n_fam)


class DeviceStream:
    """Asynchronous batches on one GPU context (``_lib.Context``).  With
    ``device_writer`` the records are formatted and BGZF-compressed on the
    device (dcr_submit_write); otherwise the kernel outputs come back for the
    host writer (dcr_submit).

    ``ss_output`` (set per run, cli.main): the single-strand records are
    wanted too: host batches carry their metadata, the device writer makes
    their stream (dcr_submit_write_ss) and the host path downloads their pos,
    n_cig and cigar.

    ``filter`` (set per run too): a params.ConsensusFilter or None.  The
    device writer applies it (dcr_set_filter) and ``result`` carries
    ``fam_filt``; on the host path the caller filters (native_io.apply_filter).
    Its per-base rules (dcr_set_base_filter) exist on the device writer only:
    the column of a base is known to the kernels alone.

    ``metrics`` (set per run too): the device writer counts the consensus QC
    tables (dcr_set_metrics) and ``result`` carries them as ``metrics``; on the
    host path the caller counts (native_io.metrics).

    ``base_tags`` (set per run too, --per_base_tags): the device writer writes
    the ten per-column tags of the duplex records, and sd / se of the
    single-strand ones, per base of SEQ (dcr_set_base_tags).  Device writer
    only, for the per-base rules' reason; the host path ignores it.

    ``base_metrics`` (set per run too, --base_metrics_output): the device
    writer counts the per-base duplex QC tables (dcr_set_base_metrics) and
    ``result`` carries them as ``base_metrics``.  Device writer only, for the
    same reason.

    ``mate_overlap`` (set per run too, --mate_overlap): 0, params.OVL_MASK or
    params.OVL_CONSENSUS.  The device writer reconciles the overlapping mates
    (dcr_set_mate_overlap) and ``result`` carries ``fam_ovl``; on the host path
    the caller does (native_io.apply_overlap).

    ``set_allele_sites`` (called per run too, --allele_sites): the device
    writer counts the alleles at the sites into a table on the context
    (dcr_set_allele_sites), which ``allele_counts`` fetches; on the host path
    the caller counts (native_io.allele_counts).

    ``genome`` (set per run too, --genome): a params.Genome or None.  The
    device writer uploads it once (dcr_set_genome, with the first batch), counts
    the errors against it and ``result`` carries them as ``genome_metrics``; on
    the host path the caller counts (native_io.genome_metrics), and the
    single-strand pos, n_cig and cigar are downloaded for it.  None frees the
    device copy with the next batch or ``close``."""

    def __init__(self, ctx, n_slots=2, owns_ctx=False, device_writer=True, persistent=False):
        """``persistent``: ``close`` only drains the slots (the context and the
        released host batches stay for the next run, cli.default_backend);
        ``close(final=True)`` frees them."""
        from . import _lib
        self.ctx = ctx
        self.owns_ctx = owns_ctx
        self.persistent = persistent
        self.closed = False
        self._spare = {}                 # reads -> [HostBatch] released by earlier runs
        self.device_writer = device_writer
        self.ss_output = False
        self.filter = None
        self.metrics = False
        self.base_tags = False
        self.base_metrics = False
        self.mate_overlap = 0
        self.allele = None               # (keys, min base quality) of set_allele_sites, or None
        self.genome = None
        self.wouts_ss = None
        self.lib = _lib.load()
        self.n_slots = n_slots
        self.outs = [_HostOut(self.lib) for _ in range(n_slots)]
        self.wouts = [_WriterOut(self.lib) for _ in range(n_slots)]
        self.busy = [False] * n_slots
        self.next_slot = 0
        self._pins = []

    def host_batch(self, reads=1 << 20):
        spare = self._spare.get((reads, self.ss_output))
        if spare:
            return spare.pop()
        return native_io.HostBatch(reads=reads, alloc=pinned_allocator(self.lib, self._pins),
                                   ss_meta=self.ss_output)

    def set_allele_sites(self, keys, min_base_quality=0):
        """``keys``: params.allele_keys' sites, or None (off).  On the device
        writer every call with keys starts a fresh zeroed table on the context,
        which the batches submitted from now on count into."""
        self.allele = None if keys is None or len(keys) == 0 else (keys, int(min_base_quality))
        if self.device_writer:
            self.ctx.set_allele_sites(*(self.allele or (None,)))

    def allele_counts(self):
        """The device writer's table so far (uint64 [sites, 8]); waits for the batches submitted."""
        return self.ctx.allele_counts()

    def release(self, batches):
        """Host batches a run is done with, kept for the next run (persistent)."""
        if self.persistent and not self.closed:
            for hb in batches:
                self._spare.setdefault((hb.reads, hb.ss_meta), []).append(hb)

    def submit(self, hb):
        slot = self.next_slot
        self.next_slot = (slot + 1) % self.n_slots
        if self.busy[slot]:
            raise RuntimeError("DeviceStream: slot reused before its result was taken")
        s = hb.s
        if self.device_writer:
            from . import _lib
            wo = self.wouts[slot]
            # compressed records are far smaller than the kernel outputs; grown on demand
            filtered = self.filter is not None
            counted = bool(self.metrics)
            based = bool(self.base_metrics)
            ovl = int(self.mate_overlap or 0)
            gen = self.genome is not None
            wo.ensure(s.n_fam, max(64 << 20, 2 * s.n_bases // 3), filtered, counted, based, ovl != 0, gen)
            # the context may serve other streams: its filter, metrics and tags are this stream's for this batch
            self.ctx.set_filter(self.filter)
            self.ctx.set_metrics(counted)
            self.ctx.set_base_tags(self.base_tags)
            self.ctx.set_base_metrics(based)
            self.ctx.set_mate_overlap(ovl)
            self.ctx.set_genome(self.genome)
            if gen:
                _lib._check(self.lib.dcr_slot_genome_metrics_out(self.ctx._ctx, slot, wo.gmet.ptr))
            if ovl:
                _lib._check(self.lib.dcr_slot_overlap_out(self.ctx._ctx, slot, wo.ovl.ptr))
            if based:
                _lib._check(self.lib.dcr_slot_base_metrics_out(self.ctx._ctx, slot, wo.bmet.ptr))
            if counted:
                _lib._check(self.lib.dcr_slot_metrics_out(self.ctx._ctx, slot, wo.met.ptr))
            if filtered:
                _lib._check(self.lib.dcr_slot_filter_out(self.ctx._ctx, slot, wo.filt.ptr))
            self._b = hb.batch_struct()
            m = WMeta()
            m.names, m.n_names = hb.a["names"].ctypes.data, s.n_names
            m.fam_code, m.fam_rx, m.fam_tid = (hb.a["fam_code"].ctypes.data, hb.a["fam_rx"].ctypes.data,
                                               hb.a["fam_tid"].ctypes.data)
            self._wres = wo.wres()
            if self.ss_output:
                if self.wouts_ss is None:
                    self.wouts_ss = [_WriterOut(self.lib) for _ in range(self.n_slots)]
                ws = self.wouts_ss[slot]
                ws.ensure(s.n_fam, max(64 << 20, 2 * s.n_bases // 3))
                ms = WMetaSs()
                ms.sub_flag, ms.sub_mi, ms.sub_rx = (hb.a["sub_flag"].ctypes.data, hb.a["sub_mi"].ctypes.data,
                                                     hb.a["sub_rx"].ctypes.data)
                self._wres_ss = ws.wres()
                _lib._check(self.lib.dcr_submit_write_ss(self.ctx._ctx, slot, ctypes.byref(self._b), ctypes.byref(m),
                                                         ctypes.byref(ms), ctypes.byref(self._wres),
                                                         ctypes.byref(self._wres_ss)))
                self.busy[slot] = True
                return (slot, s.n_fam, True, filtered, counted, based, ovl != 0, gen)
            _lib._check(self.lib.dcr_submit_write(self.ctx._ctx, slot, ctypes.byref(self._b), ctypes.byref(m),
                                                  ctypes.byref(self._wres)))
            self.busy[slot] = True
            return (slot, s.n_fam, False, filtered, counted, based, ovl != 0, gen)
        out = self.outs[slot]
        out.ensure(4 * s.n_fam, s.ss_cols, 2 * s.n_fam, s.ds_cols, s.n_reads,
                   SS_FIELDS_FULL if self.ss_output or self.genome is not None else SS_FIELDS)
        self._b = hb.batch_struct()
        so, do = out.dcr_out("ss"), out.dcr_out("ds")
        from . import _lib
        _lib._check(self.lib.dcr_submit(self.ctx._ctx, slot, ctypes.byref(self._b), ctypes.byref(so),
                                        ctypes.byref(do), None))
        self.busy[slot] = True
        return slot

    def result(self, handle):
        from . import _lib
        if self.device_writer:
            slot, n_fam = handle[:2]
            wo = self.wouts[slot]
            ws = self.wouts_ss[slot] if handle[2] else None
            r = wo.wres()
            if ws is not None:
                rc = self.lib.dcr_wait_write_ss(self.ctx._ctx, slot, ctypes.byref(r), ctypes.byref(ws.wres()))
            else:
                rc = self.lib.dcr_wait_write(self.ctx._ctx, slot, ctypes.byref(r))
            self.busy[slot] = False
            grown = False
            for o, what in ((wo, 2), (ws, 5)):
                if rc == 3 and o is not None and int(o.totals[0]) > o.cap_b:   # DCR_ECAPACITY: grow, fetch again
                    n = int(o.totals[0])
                    tot = o.totals[:3].copy()
                    o.ensure(n_fam, n)
                    o.totals[:3] = tot
                    _lib._check(self.lib.dcr_slot_fetch(self.ctx._ctx, slot, what, 0, n, o.blocks.ptr))
                    grown = True
            if not grown:
                _lib._check(rc)
            return WriterResult(self, slot, wo, n_fam, ws, handle[3], handle[4], handle[5], handle[6], handle[7])
        slot = handle
        _lib._check(self.lib.dcr_wait(self.ctx._ctx, slot))
        self.busy[slot] = False
        out = self.outs[slot]
        return out.fmt_out("ss"), out.fmt_out("ds"), None

    def close(self, final=False):
        if self.closed:
            return
        for slot in range(self.n_slots):
            if self.busy[slot]:
                if self.device_writer:
                    self.lib.dcr_wait_write(self.ctx._ctx, slot, ctypes.byref(self.wouts[slot].wres()))
                else:
                    self.lib.dcr_wait(self.ctx._ctx, slot)
                self.busy[slot] = False
        if self.device_writer and self.ctx.genome is not None:
            self.genome = None
            self.ctx.set_genome(None)    # set per run: a kept backend does not keep the genome
        if self.persistent and not final:
            return
        self.closed = True
        self._spare.clear()
        for p in self._pins:
            p.free()
        self._pins.clear()
        for o in self.outs:
            if o.mem is not None:
                o.mem.free()
        for w in self.wouts + (self.wouts_ss or []):
            for m in (w.small, w.blocks, w.filt, w.met, w.bmet, w.ovl, w.gmet):
                if m is not None:
                    m.free()
        if self.owns_ctx:
            self.ctx.close()


class CallBackend:
    """Synchronous backend over ``fn(packed, params) -> (ss, ds, info)``."""

    def __init__(self, fn, params):
        self.fn, self.params = fn, params
        self.ss_output = False
        self.filter = None               # applied by the caller (native_io.apply_filter)
        self.metrics = False             # counted by the caller (native_io.metrics)
        self.mate_overlap = 0            # applied by the caller (native_io.apply_overlap)
        self.allele = None               # counted by the caller (native_io.allele_counts)
        self.genome = None               # counted by the caller (native_io.genome_metrics)
        self._res = {}
        self._k = 0

    def host_batch(self, reads=1 << 20):
        return native_io.HostBatch(reads=reads, ss_meta=self.ss_output)

    def set_allele_sites(self, keys, min_base_quality=0):
        self.allele = None if keys is None or len(keys) == 0 else (keys, int(min_base_quality))

    def submit(self, hb):
        ss, ds, info = self.fn(hb.packed(), self.params)
        self._k += 1
        rs = None if info is None else np.ascontiguousarray(info["status"], np.int32)
        self._res[self._k] = (ss, ds, rs)
        return self._k

    def result(self, h):
        ss, ds, rs = self._res.pop(h)
        self._keep = (ss, ds, rs)
        return native_io.fmt_out(ss), native_io.fmt_out(ds), rs

    def close(self):
        self._res.clear()
