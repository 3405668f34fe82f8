"""Command line drop-in for the reference script's ``main``
(DuplexUMIConsensusReads.py:1426-1650): same flags (``parse_args`` :10-91),
same output files, same stdout, same record order.

The per-record work runs natively (libdcr_io.so, include/dcr_io.h):

* the ingest reads the BAM (threaded BGZF inflate), applies ``pass_filters``
  (:1135-1181), groups MI runs (:1185-1217), checks and splits families and
  downsamples with CPython's MT19937 (:100-188), and packs whole batches of
  families into pinned host memory;
* the device runs the six ``make_consensus_read`` calls of every family of a
  batch (:1560-1582) in one asynchronous submit (stream.DeviceStream);
* the writer formats the duplex records (:1352-1419) and deflates BGZF
  blocks on a worker pool; excluded reads and filtered families are copied
  through as stored.

``--single_strand_output FILE`` (not a reference flag) also writes the four
single-strand consensus reads of every written family, which the reference
builds (``make_consensus_read(method="single_strand")`` :1564-1569) and drops.

``--filter_*`` (not reference flags either) mask weak duplex bases and drop
families whose duplex records have too little support or too many
disagreements (include/dcr.h ``dcr_filter``): the step that otherwise follows
on the written file.  ``--filter_min_base_reads``, ``--filter_max_base_error_rate``
and ``--filter_require_strand_agreement`` mask single duplex bases by the
raw-read support and the strand agreement at the base's own alignment column
(``dcr_base_filter``; device writer only).  Off by default; without one
nothing changes.

``--metrics_output FILE.json`` (not a reference flag) writes the consensus QC
tables (include/dcr.h ``dcr_metrics``): family sizes, strand depths, error
rates, base qualities and errors by read position of the consensus as called,
before any filter; counted on the device beside the writer.  Off by default.

``--base_metrics_output FILE.json`` (not a reference flag) writes the per-base
duplex QC tables (include/dcr.h ``dcr_base_metrics``): which strand called which
base, the strands' depths and error rates per base, qualities by agreement and
all of it by cycle, of the consensus as called, before any filter; counted on
the device over the per-base filters' column maps (device writer only).  Off
by default.

``--per_base_tags`` (not a reference flag) writes the depth, error and strand
tags ``ad bd cd ae be ce ac bc aq bq`` (and ``sd se`` of the single-strand
reads) with one value per base of ``SEQ``, as ``B:s`` arrays and strings of the
read's length, instead of the reference's lists per alignment column
(include/dcr.h ``dcr_set_base_tags``; device writer only).  Off by default;
without it no output byte changes.

``--mate_overlap mask|consensus`` (not a reference flag) reconciles the two
duplex reads of a family where both cover the same reference position
(include/dcr.h ``dcr_set_mate_overlap``): ``mask`` turns disagreeing bases into
'N', ``consensus`` keeps the better base at the difference of the qualities and
adds the qualities of agreeing bases (at most 93).  Only ``SEQ`` and ``QUAL`` of
the duplex reads change; the step comes after the QC tables and before any
``--filter_*``.  Off by default; without it no output byte changes.

``--allele_sites FILE --allele_counts_output FILE.tsv`` (not reference flags;
each needs the other) count, per listed reference position, how many written
families show A, C, G, T, N, a deletion or two disagreeing reads (include/dcr.h
``dcr_set_allele_sites``): a family counts once where its two reads overlap.
The records count as they are written, after ``--mate_overlap`` and every
``--filter_*``; ``--allele_min_base_quality Q`` makes a base below Q count as
N.  Off by default; no other output byte changes with them.

``--genome FILE.fa --genome_metrics_output FILE.json`` (not reference flags;
each needs the other) count the consensus against a reference FASTA
(include/dcr.h ``dcr_genome_metrics``): per level (the single-strand records,
counted whether or not they are written, and the duplex records) the aligned
bases, matches, mismatches, the substitution spectrum with and without its two
neighbours, and the mismatches by cycle and by quality, of the consensus as
called, before ``--mate_overlap`` and any ``--filter_*``.  The FASTA is plain
text; only the sequences of the input header are kept, and their lengths must
be the header's.  Off by default; no other output byte changes with them, and
the summary gains one line.

Batches are pipelined: a thread ingests batch k+1 while the device runs batch
k and the main thread writes batch k-1.

Failure semantics follow the reference: everything the reference writes
before it stops (consensus records of earlier families; side-file records up
to the failing family, ``dcr_host_batch.tab_*_cut``) is written, then its
exception, or its message and ``sys.exit(1)``, is raised at that family.
"""
from __future__ import annotations

import argparse
import contextlib
from concurrent.futures import ThreadPoolExecutor
import ctypes
import io
import os
import queue
import random
import shutil
import socket
import subprocess
import sys
import threading
import time
from typing import Optional

import numpy as np

from . import native_io
from . import params as params_mod
from .params import ConsensusFilter, ConsensusParams

SPLIT_NAMES = {0: "A1", 1: "B2", 2: "B1", 3: "A2"}      # split_dict (:1511)
EQX_LINE = 'Symbols "x" and "=" were found in CIGAR strings and were changed to "M"'   # :375
STAGE_LINES = ("\t\t * Reconstruct alignment in progress", "\t\t * Call consensus in progress",
               "\t\t * Adjust consensus fields in progress")                            # :1318-1341
BADCHAR_LINE = ("\n ERROR: input values to nucleotide/INDEL list in function call_consensus() and subfunction "
                "most_likely_nucleotide() are different than the allowed ones. \n Please check documentation")


def parse_args(argv):
    """The reference's flags (:10-91), names and defaults unchanged."""
    ap = argparse.ArgumentParser(description="call consensus reads from paired-end, Duplex-UMI reads, "
                                             "preserving mapping information")
    ap.add_argument("-i", "--input_file", required=True, type=str)
    ap.add_argument("-o", "--output_file", required=False, default=None, type=str)
    ap.add_argument("-v", "--verbose", action="store_true")
    ap.add_argument("-q", "--min_map_quality", required=False, default=20, type=int)
    ap.add_argument("--min_base_quality", required=False, default=20, type=int)
    ap.add_argument("--min_reads", required=False, default=1, type=int)
    ap.add_argument("--max_reads", required=False, default=100, type=int)
    ap.add_argument("--max_base_quality", required=False, default=60, type=int)
    ap.add_argument("--base_quality_shift", required=False, default=0, type=int)
    ap.add_argument("--error_rate_post_labeling", required=False, default=0, type=int)
    ap.add_argument("--error_rate_pre_labeling", required=False, default=0, type=int)
    ap.add_argument("--deletion_score", required=False, default=30, type=int)
    ap.add_argument("--no_insertion_score", required=False, default=30, type=int)
    # not reference flags: batching and codec knobs (they do not change any record)
    ap.add_argument("--batch_reads", required=False, default=int(os.environ.get("DCR_BATCH_READS", 1 << 19)), type=int,
                    help=argparse.SUPPRESS)   # DCR_BATCH_READS: A/B runs of the bench, which calls main() without flags
    ap.add_argument("--threads", required=False, default=0, type=int, help=argparse.SUPPRESS)
    ap.add_argument("--compression_level", required=False, default=6, type=int, help=argparse.SUPPRESS)
    ap.add_argument("--device", required=False, default=0, type=int, help=argparse.SUPPRESS)
    # one process per GPU over ranges of whole families (sharded mode below)
    ap.add_argument("--gpus", required=False, default=1, type=int, help=argparse.SUPPRESS)
    # not a reference flag: the four single-strand consensus reads of every
    # written family (make_consensus_read method="single_strand", which the
    # reference builds and drops) into a BAM of their own
    ap.add_argument("--single_strand_output", required=False, default=None, type=str)
    # not reference flags: the consensus filters (include/dcr.h dcr_filter); any one turns them on
    ap.add_argument("--filter_min_base_quality", required=False, default=None, metavar="Q",
                    type=params_mod.filter_min_base_quality,
                    help="mask duplex bases below Q: 'N' with quality min(q, 2)")
    ap.add_argument("--filter_min_reads", required=False, default=None, metavar="T[,A[,B]]",
                    type=params_mod.filter_min_reads,
                    help="keep a duplex read with aD + bD >= T, max(aD, bD) >= A, min(aD, bD) >= B")
    ap.add_argument("--filter_max_read_error_rate", required=False, default=None, metavar="C[,S]",
                    type=params_mod.filter_max_read_error_rate, help="keep a duplex read with cE <= C, aE and bE <= S")
    ap.add_argument("--filter_max_no_call_fraction", required=False, default=None, metavar="X",
                    type=params_mod.filter_max_no_call_fraction,
                    help="keep a duplex read with at most X of its bases 'N' after masking")
    ap.add_argument("--filter_min_mean_base_quality", required=False, default=None, metavar="Q",
                    type=params_mod.filter_min_mean_base_quality,
                    help="keep a duplex read whose mean base quality after masking is at least Q")
    # the per-base rules (include/dcr.h dcr_base_filter): by the support and agreement at the base's own column
    ap.add_argument("--filter_min_base_reads", required=False, default=None, metavar="T[,A[,B]]",
                    type=params_mod.filter_min_base_reads,
                    help="mask a duplex base unless, at its column, aD + bD >= T, max(aD, bD) >= A, min(aD, bD) >= B")
    ap.add_argument("--filter_max_base_error_rate", required=False, default=None, metavar="X",
                    type=params_mod.filter_max_base_error_rate,
                    help="mask a duplex base whose column has aE + bE > X * (aD + bD)")
    ap.add_argument("--filter_require_strand_agreement", action="store_true",
                    help="mask a duplex base where the two single-strand consensus reads disagree (cE > 0)")
    # not a reference flag: the consensus QC tables (include/dcr.h dcr_metrics) as JSON
    ap.add_argument("--metrics_output", required=False, default=None, type=str, metavar="FILE.json",
                    help="count family sizes, strand depths, error rates, qualities and errors by read position "
                         "of the consensus reads as called (before any --filter_*) into FILE.json")
    # not a reference flag: the per-base duplex QC tables (include/dcr.h dcr_base_metrics) as JSON
    ap.add_argument("--base_metrics_output", required=False, default=None, type=str, metavar="FILE.json",
                    help="count, per base of the duplex consensus reads as called (before any --filter_*), the "
                         "strands' calls against each other, their depths and error rates, the qualities by "
                         "agreement and all of it by cycle into FILE.json")
    # not a reference flag: the per-column tags per base of SEQ (include/dcr.h dcr_set_base_tags)
    ap.add_argument("--per_base_tags", action="store_true",
                    help="write ad bd cd ae be ce as B:s arrays and ac bc aq bq as strings with one value per base "
                         "of SEQ (sd se of --single_strand_output likewise) instead of lists per alignment column")
    # not a reference flag: the two duplex reads of a family where they overlap (include/dcr.h dcr_set_mate_overlap)
    ap.add_argument("--mate_overlap", required=False, default=None, metavar="mask|consensus",
                    type=params_mod.mate_overlap,
                    help="where the two duplex reads of a family cover the same reference position: 'mask' turns "
                         "disagreeing bases into 'N'; 'consensus' keeps the base of the higher quality at the "
                         "difference of the two and gives agreeing bases the sum (at most 93)")
    # not reference flags: duplex allele counts at given sites (include/dcr.h dcr_set_allele_sites)
    ap.add_argument("--allele_sites", required=False, default=None, type=str, metavar="FILE",
                    help="sites to count alleles at: lines name<TAB>pos (1-based) or BED name<TAB>start<TAB>end "
                         "(0-based, every position of [start, end)); needs --allele_counts_output")
    ap.add_argument("--allele_counts_output", required=False, default=None, type=str, metavar="FILE.tsv",
                    help="per site of --allele_sites, how many written families show A, C, G, T, N, a deletion or "
                         "two disagreeing reads (a family counts once where its two reads overlap) into FILE.tsv")
    ap.add_argument("--allele_min_base_quality", required=False, default=0, metavar="Q",
                    type=params_mod.allele_min_base_quality,
                    help="for --allele_counts_output: a base below Q counts as N")
    # not reference flags: errors against a reference FASTA (include/dcr.h dcr_genome_metrics)
    ap.add_argument("--genome", required=False, default=None, type=str, metavar="FILE.fa",
                    help="the genome the input was aligned to, plain-text FASTA; needs --genome_metrics_output")
    ap.add_argument("--genome_metrics_output", required=False, default=None, type=str, metavar="FILE.json",
                    help="count the single-strand and the duplex consensus reads as called against --genome: aligned "
                         "bases, mismatches, the substitution spectrum, and the mismatches by cycle and quality into "
                         "FILE.json")
    args = ap.parse_args(argv)
    if (args.genome is None) != (args.genome_metrics_output is None):
        raise ValueError("--genome and --genome_metrics_output need each other")
    if (args.allele_sites is None) != (args.allele_counts_output is None):
        raise ValueError("--allele_sites and --allele_counts_output need each other")
    return args


class ReferenceExit(SystemExit):
    """The reference prints an error and calls sys.exit(1)."""


def badchar_column(hb, f: int, k: int, min_base_quality: int):
    """The column most_likely_nucleotide prints before exiting on an invalid
    letter (:582-585), for single-strand consensus k of processed family f.

    Error reporting only (the device already decided the outcome): the reads
    are preprocessed as :191-325 do and laid out as reconstruct_alignment
    (:458-545) does until the first column holding a letter outside
    A T C G N a t c g n + -."""
    a = hb.a
    allowed = set("ATCGNatcgn+-")
    pos, cig, seq = [], [], []
    for r in range(int(a["sub_off"][4 * f + k]), int(a["sub_off"][4 * f + k + 1])):
        o, n = int(a["seq_off"][r]), int(a["seq_len"][r])
        s = a["bases"][o:o + n].tobytes().decode("latin-1")
        q = a["quals"][o:o + n]
        c0 = int(a["cig_off"][r])
        ops, s5, s3, inseq = [], 0, 0, False
        for w in a["cigar"][c0:c0 + int(a["cig_n"][r])]:
            op, ln = int(w) & 15, int(w) >> 4
            if op == 4:
                if not inseq:
                    s5 = ln
                else:
                    s3 = ln
            elif op != 5:
                inseq = True
                ops.append((op, ln))
        keep = slice(s5, -s3) if s3 else slice(s5, None)
        s, q = s[keep], q[keep]
        s = "".join("N" if qq < min_base_quality else ch for ch, qq in zip(s, q))
        tn = len(s) - len(s.rstrip("N"))
        s = s[:len(s) - tn]
        exp = [0 if op in (7, 8) else op for op, ln in ops for _ in range(ln)]
        pos.append(int(a["read_pos"][r]))
        cig.append(exp[:len(exp) - tn])
        seq.append(s)
    lo, hi = min(pos), max(p + len(s) for p, s in zip(pos, seq))
    ic, iz = [0] * len(pos), [0] * len(pos)
    for p in range(lo, hi):
        cur = [c[i] if i < len(c) else 99 for c, i in zip(cig, ic)]
        col = []
        if 1 in cur:
            for r, op in enumerate(cur):
                if op == 1:
                    col.append(seq[r][iz[r]].lower())
                    ic[r] += 1
                    iz[r] += 1
                else:
                    col.append("+")
        else:
            for r in range(len(pos)):
                if p < pos[r] or iz[r] >= len(seq[r]):
                    col.append("N")
                elif cig[r][ic[r]] == 2:
                    col.append("-")
                    ic[r] += 1
                else:
                    col.append(seq[r][iz[r]])
                    ic[r] += 1
                    iz[r] += 1
        if any(ch not in allowed for ch in col):
            return np.array(col)
    return None


_BACKENDS = {}        # device -> DeviceStream kept for later runs in this process


def default_backend(params: ConsensusParams, device: int = 0):
    """The HIP library on ``device`` (fails loudly without it: no CPU fallback).

    The context (stream, workspace, slots) and its pinned host batches are
    made once per process and device and reused by later ``main`` calls (a
    service that converts many BAMs, or the bench's repeated passes), as a
    caching host allocator would: the first call pays the allocation."""
    from . import _lib
    from .stream import DeviceStream
    if os.environ.get("DCR_BACKEND_CACHE") == "0":        # A/B runs: a fresh context per call
        return DeviceStream(_lib.Context(params, device=device), owns_ctx=True)
    be = _BACKENDS.get(device)
    if be is None or be.closed:
        ctx = _lib.Context(params, device=device)
        be = DeviceStream(ctx, owns_ctx=True, persistent=True)
        _BACKENDS[device] = be
        if len(_BACKENDS) == 1:
            import atexit
            atexit.register(_close_backends)
    elif be.ctx.params != params:
        be.ctx.set_params(params)
    return be


def _close_backends():
    for be in _BACKENDS.values():
        be.close(final=True)
    _BACKENDS.clear()
    if _INFLATERS:
        native_io.set_inflate_hook(None)
        for inf, _ in _INFLATERS.values():
            inf.close()
        _INFLATERS.clear()


_INFLATERS = {}       # device -> (_lib.Inflater, its hook), kept for later runs in this process


def gpu_inflate(device: int = 0):
    """BGZF inflate on ``device`` for the ingests this process opens from now
    on (include/dcr_inflate.h; the native ingest hands each chunk's members to
    the device inflater and takes its chunk buffers page-locked from it).
    One inflater per process and device, kept like the backend.

    On by default, DCR_GPU_INFLATE=0 keeps the host inflate pool.  The
    ingest streams the input's members to the device in spans launched ahead
    of the reader: measured whole-node on C2 it beats the host
    pool at input levels 1 and 6 (profiles/r03m).  A member is still ~4 ms of
    serial decode on one wavefront, so the per-chunk launches tried first
    lost (profiles/r03g, r03h)."""
    if os.environ.get("DCR_GPU_INFLATE") == "0":
        if native_io._HOOK is not None:
            native_io.set_inflate_hook(None)
        return None
    got = _INFLATERS.get(device)
    if got is None:
        from . import _lib
        inf = _lib.Inflater(device)
        got = (inf, inf.hook())
        _INFLATERS[device] = got
        if len(_INFLATERS) == 1 and not _BACKENDS:
            import atexit
            atexit.register(_close_backends)
    native_io.set_inflate_hook(got[1])
    return got[0]


def _as_backend(backend, params, device=0, ss_output=False, flt=None, metrics=False, base_tags=False,
                base_metrics=False, mate_overlap=0, allele=None, genome=None):
    """``ss_output``: this run also writes the single-strand records (a
    property of the run, set on the backend each time: the default backend
    is kept across runs).  ``flt``: this run's ConsensusFilter or None,
    set each time in the same way; so are ``metrics`` (--metrics_output),
    ``base_tags`` (--per_base_tags), ``base_metrics``
    (--base_metrics_output) and ``mate_overlap`` (--mate_overlap: 0 or a
    params.OVL_* mode; the rule needs only the written record, so every
    backend that carries the attribute supports it)."""
    if backend is None:
        be = default_backend(params, device)
    elif hasattr(backend, "submit"):
        be = backend
    else:
        from .stream import CallBackend
        be = CallBackend(backend, params)
    if hasattr(be, "ss_output"):
        be.ss_output = ss_output
    elif ss_output:
        raise ValueError("this backend cannot produce the single-strand records")
    if flt is not None and flt.base_active and not getattr(be, "device_writer", False):
        # the column of a base is only known on the device (the kernels' maps)
        raise ValueError("this backend cannot apply the per-base filters")
    if hasattr(be, "filter"):
        be.filter = flt
    elif flt is not None:
        raise ValueError("this backend cannot apply the consensus filters")
    if hasattr(be, "metrics"):
        be.metrics = metrics
    elif metrics:
        raise ValueError("this backend cannot count the consensus metrics")
    if base_tags and not getattr(be, "device_writer", False):
        # no host formatter for them: the column of a base is only known on the device
        raise ValueError("this backend cannot write the per-base tags")
    if hasattr(be, "base_tags"):
        be.base_tags = base_tags
    if base_metrics and not getattr(be, "device_writer", False):
        # no host path, for the tags' reason
        raise ValueError("this backend cannot count the per-base metrics")
    if hasattr(be, "base_metrics"):
        be.base_metrics = base_metrics
    if hasattr(be, "mate_overlap"):
        be.mate_overlap = mate_overlap or 0
    elif mate_overlap:
        raise ValueError("this backend cannot reconcile the overlapping mates")
    # --allele_sites: (keys, min base quality) or None; set each time, so a kept backend starts a fresh table
    if hasattr(be, "set_allele_sites"):
        be.set_allele_sites(*(allele or (None,)))
    elif allele:
        raise ValueError("this backend cannot count the alleles")
    # --genome: the params.Genome or None; set each time too
    if hasattr(be, "genome"):
        be.genome = genome
    elif genome is not None:
        raise ValueError("this backend cannot count against a genome")
    return be


OUTPUT_FORMAT_ERROR = ("ERROR: output file is not specified in the right format. \n Please specify the file name of a "
                       "valid .bam file. Include the format in the file name.")      # :1491


def _check_ss_output(args, say=True):
    """--single_strand_output must name a .bam file, as -o must (:1488-1492)."""
    if args.single_strand_output is not None and not args.single_strand_output.endswith(".bam"):
        if say:
            print(OUTPUT_FORMAT_ERROR)
        raise ReferenceExit(1)


def _check_metrics_output(args, say=True):
    """--metrics_output, --base_metrics_output and --genome_metrics_output
    must name .json files; they are created here, before the pass and before
    any output file, so a bad path fails early."""
    paths = [p for p in (args.metrics_output, args.base_metrics_output, args.genome_metrics_output) if p is not None]
    for path in paths:
        if not path.endswith(".json"):
            if say:
                print(OUTPUT_FORMAT_ERROR)
            raise ReferenceExit(1)
    made = []
    try:
        for path in paths:
            open(path, "a").close()
            made.append(path)
    except BaseException:
        for path in made:               # neither file from a run that never starts
            with contextlib.suppress(OSError):
                os.remove(path)
        raise


def _finish_metrics(path, total, done, to_json=None):
    """The run's counters as JSON when it completed; otherwise no file (the
    counters of the families after a failing one cannot be separated out).
    ``to_json``: params.metrics_json, or base_metrics_json for
    --base_metrics_output."""
    if path is None:
        return
    if done and total is not None:
        with open(path, "w") as f:
            f.write((to_json or params_mod.metrics_json)(total))
    else:
        with contextlib.suppress(OSError):
            os.remove(path)


def _load_genome(args, header, stats=None):
    """--genome: the FASTA reduced to the sequences of the input's ``header``
    (params.load_genome; a compressed file, a wrong length or a name that
    occurs twice is a ValueError, raised here before any output file exists).
    Sets ``args.genome_data`` to the params.Genome, or None without the
    option."""
    args.genome_data = None
    if args.genome is None:
        return
    if not args.genome_metrics_output.endswith(".json"):
        return                              # _check_metrics_output reports it
    args.genome_data = params_mod.load_genome(args.genome, params_mod.header_sequences(header))
    if stats is not None:
        stats["genome_load_s"] = args.genome_data.load_s


def _genome_summary(c, total):
    """The summary's counters of a block (``_print_summary``)."""
    if total is not None:
        c["genome_levels"] = params_mod.genome_totals(total)


def _check_allele_output(args, header, say=True):
    """--allele_counts_output must name a .tsv file, as the metrics files name
    .json ones; the sites of --allele_sites are read against the input's
    ``header`` (a bad line is a ValueError before any file exists) and the
    file is created here, before the pass.  Sets ``args.allele`` to (keys,
    --allele_min_base_quality, reference names), or None without the option."""
    args.allele = None
    path = args.allele_counts_output
    if path is None:
        return
    if not path.endswith(".tsv"):
        if say:
            print(OUTPUT_FORMAT_ERROR)
        raise ReferenceExit(1)
    refs = params_mod.header_references(header)
    keys = params_mod.allele_keys(args.allele_sites, refs)
    open(path, "a").close()
    args.allele = (keys, args.allele_min_base_quality, refs)


def _finish_allele(args, total, done):
    """The run's table as TSV when it completed; otherwise no file, as the metrics."""
    path = args.allele_counts_output
    if path is None:
        return
    if done and total is not None and getattr(args, "allele", None) is not None:
        with open(path, "w") as f:
            f.write(params_mod.allele_tsv(args.allele[0], total, args.allele[2]))
    else:
        with contextlib.suppress(OSError):
            os.remove(path)


def _allele_summary(c, total):
    """The summary's counters of a table (``_print_summary``)."""
    if total is not None:
        (c["allele_sites"], c["allele_covered"], c["allele_molecules"],
         c["allele_discordant"]) = params_mod.allele_totals(total)


def _raise_reference(kind: str, msg: str = ""):
    if kind == "exit":
        raise ReferenceExit(1)
    exc = {"IndexError": IndexError, "TypeError": TypeError, "ValueError": ValueError,
           "OverflowError": OverflowError, "AttributeError": AttributeError}.get(kind)
    if kind == "UnicodeEncodeError":
        raise UnicodeEncodeError("ascii", "", 0, 1, "ordinal not in range(128)")
    raise (exc or RuntimeError)(msg or f"reference would raise {kind} here")


class _Driver:
    def __init__(self, args, params, backend, ing, cons, excl, unproc, sscs=None):
        """``sscs``: the writer of the single-strand records' file, or None."""
        self.args, self.params, self.backend = args, params, backend
        self.ing, self.cons, self.excl, self.unproc, self.sscs = ing, cons, excl, unproc, sscs
        self.verbose = args.verbose
        self.filter = ConsensusFilter.from_args(args)
        # families dropped by the filter, per reason, and bases masked in the written ones (the summary's counters)
        self.filter_counts = {} if self.filter is None else dict(
            {"filter_dropped": 0, "filter_masked": 0}, **{"filter_" + name: 0 for _, name in params_mod.FILT_REASONS})
        # --mate_overlap: the mode and the counters of the families written (the summary's)
        self.overlap = args.mate_overlap or 0
        self.overlap_counts = {} if not self.overlap else {"overlap_compared": 0, "overlap_disagree": 0,
                                                           "overlap_changed": 0}
        # per-stage busy seconds and totals (bench.py --e2e reports them)
        self.trace = None          # optional [(stage, t0, t1)] (bench.py)
        self.ends_at_eof = True    # False for a sharded range that stops before the end
        self.stats = {"batches": 0, "consensus_records": 0, "consensus_bases": 0, "ingest_s": 0.0,
                      "submit_s": 0.0, "wait_s": 0.0, "write_s": 0.0, "idle_s": 0.0}
        if self.filter is not None:
            self.stats.update(filter_dropped_families=0, filter_masked_bases=0)
        self.stats.update(self.overlap_counts)
        # --metrics_output: the batches' counters summed at once (a device slot's block is overwritten on reuse)
        self.metrics_total = np.zeros(params_mod.MET_WORDS, np.uint64) if args.metrics_output is not None else None
        self.base_metrics_total = (np.zeros(params_mod.BMET_WORDS, np.uint64)
                                   if args.base_metrics_output is not None else None)
        # --allele_sites: (keys, min base quality); the table is summed here on the host path and
        # fetched from the device writer's context once, after the last batch
        al = getattr(args, "allele", None)
        self.allele = None if al is None or len(al[0]) == 0 else (al[0], al[1])
        self.allele_total = None if al is None else np.zeros((len(al[0]), params_mod.ALLELE_COLS), np.uint64)
        # --genome: the batches' blocks summed as the other tables'
        self.genome = getattr(args, "genome_data", None)
        self.genome_total = np.zeros(params_mod.GMET_WORDS, np.uint64) if self.genome is not None else None

    # -- stdout of one batch, in the reference's order --------------------------
    def _prints(self, hb, fail_f, kind, which, last_batch):
        a = hb.a
        F = hb.n_fam
        eqx = a["fam_eqx"][:4 * F]
        if not self.verbose and fail_f >= F and not eqx.any():
            return
        if not self.verbose:
            # only the =/X lines (:374-375), per processed family in order
            nz = np.nonzero(eqx.reshape(F, 4).any(axis=1))[0] if F else []
            for f in nz:
                if f > fail_f:
                    break
                for k in range(4):
                    if f == fail_f and not self._ss_started(k, kind, which):
                        break
                    for _ in range(int(eqx[4 * f + k])):
                        print(EQX_LINE)
            return
        max_reads = self.params.max_reads
        n_tab = hb.s.n_tab
        for t in range(n_tab):
            kind_t, p = int(a["tab_kind"][t]), int(a["tab_proc"][t])
            code = hb.name(a["tab_code"][t])
            sampled = int(a["tab_sampled"][t])
            for k in range(4):                                              # :183-186
                if sampled >> k & 1:
                    print("Family", code, "subfamily", SPLIT_NAMES[k], "has been randomly downsampled to",
                          max_reads, "reads to form consensus read")
            if kind_t == native_io.FAM_FILTERED:
                print("Not enough reads in family", code, "to form consensus reads \n")       # :180
                continue
            failing = p == fail_f
            self._trim_prints(hb, p, kind if failing else None, which if failing else None)
            if failing and which >= 8:
                return
            for k in range(4):
                if failing and which == k and kind == "TypeError":
                    print("Single-strand consensus for subfamily", code, SPLIT_NAMES[k], "in progress")
                    return
                print("Single-strand consensus for subfamily", code, SPLIT_NAMES[k], "in progress")   # :1566-1567
                for _ in range(int(eqx[4 * p + k])):
                    print(EQX_LINE)
                if failing and which == k:
                    self._stage_prints(kind)
                    return
                for line in STAGE_LINES:
                    print(line)
            print("Double-strand consensus for family", code, "in progress")                    # :1578-1579
            for j in range(2):
                if failing and which == 4 + j and kind != "UnicodeEncodeError":
                    self._stage_prints(kind)
                    return
                for line in STAGE_LINES:
                    print(line)
                if failing and which == 4 + j:
                    return
            # the family the input's end completes (a range that ends early
            # completes its last family on the next family's first read)
            is_last = last_batch and t == n_tab - 1 and self.ends_at_eof
            print("Consensus reads for family", code,
                  "have been sucessfully writen \n" if is_last else "have been sucessfully written \n")  # :1597, :1631

    @staticmethod
    def _ss_started(k, kind, which):
        """Were subfamily k's =/X lines printed before the failure?"""
        if which >= 8:
            return False
        if which >= 4 or k < which:
            return True
        return k == which and kind != "TypeError"

    @staticmethod
    def _stage_prints(kind):
        """Stage lines printed before a consensus call fails (:1318-1341)."""
        n = {"exit": 2, "TypeError": 0}.get(kind, 3)
        for line in STAGE_LINES[:n]:
            print(line)

    def _trim_prints(self, hb, p, kind, which):
        """Verbose '3-prime N trimming' lines (:306-310): one per trailing 'N'
        after clip removal and masking, printing the masked sequence."""
        a = hb.a
        mb = self.params.min_base_quality
        r0, r1 = int(a["sub_off"][4 * p]), int(a["sub_off"][4 * p + 4])
        for r in range(r0, r1):
            o, n = int(a["seq_off"][r]), int(a["seq_len"][r])
            if n == 0:
                return
            cig = a["cigar"][int(a["cig_off"][r]):int(a["cig_off"][r]) + int(a["cig_n"][r])]
            s5 = s3 = 0
            inseq = False
            for c in cig:
                op, ln = int(c) & 15, int(c) >> 4
                if op == 4:
                    if not inseq:
                        s5 = ln
                    else:
                        s3 = ln
                elif op != 5:
                    inseq = True
            seq = a["bases"][o + s5:o + n - s3].copy()
            q = a["quals"][o + s5:o + n - s3]
            seq[q < mb] = ord("N")
            text = seq.tobytes().decode("latin-1")
            tn = len(text) - len(text.rstrip("N"))
            for _ in range(tn):
                print("3-prime N trimming has been performed on read", text)

    # -- one batch --------------------------------------------------------------
    def finish(self, hb, handle, last_batch):
        t0 = time.perf_counter()
        res = self.backend.result(handle)
        t1 = time.perf_counter()
        if self.trace is not None:
            self.trace.append(("wait", t0, t1))
        F = hb.n_fam
        st = self.stats
        if getattr(self.backend, "device_writer", False):
            # records formatted and compressed on the device (dcr_submit_write)
            nz = np.flatnonzero(res.fam_fail)
            fail_f = int(nz[0]) if len(nz) else F
            kind, which = None, -1
            if fail_f < F:
                code = int(res.fam_fail[fail_f])
                kind, which = native_io.FAIL_NAMES.get(code & 0xff), code >> 8
            self._prints(hb, fail_f, kind, which, last_batch)
            if fail_f == F:
                self.cons.put_blocks(res.bgzf, res.record_bytes)
            elif fail_f:
                self.cons.write(res.record_bytes_of(fail_f))
            if self.sscs is not None:
                # as `for r in single_consensus: write(r)` beside :1593-1594
                if fail_f == F:
                    self.sscs.put_blocks(res.ss_bgzf, res.ss_record_bytes)
                elif fail_f:
                    self.sscs.write(res.ss_record_bytes_of(fail_f))
            lens = res.ds_len[:2 * fail_f]
            filt = res.fam_filt[:fail_f] if self.filter is not None else None
            ovl = res.fam_ovl[:3 * fail_f] if self.overlap else None
            if self.metrics_total is not None:
                self.metrics_total += res.metrics
            if self.base_metrics_total is not None:
                self.base_metrics_total += res.base_metrics
            if self.genome_total is not None:
                self.genome_total += res.genome_metrics
        else:
            ss, ds, rstat = res
            fail_f, kind, which = native_io.first_failure(hb, ss, ds, F, rstat)
            self._prints(hb, fail_f, kind, which, last_batch)
            if self.metrics_total is not None:
                # before the filter, which masks the duplex arrays in place
                self.metrics_total += native_io.metrics(hb, ss, ds, fail_f)
            if self.genome_total is not None:
                # the consensus as called too: before the overlap step and the filter
                self.genome_total += native_io.genome_metrics(hb, ss, ds, self.genome, fail_f)
            # after the tables (the consensus as called), before the filter (which sees what this leaves)
            ovl = native_io.apply_overlap(hb, ss, ds, self.overlap, fail_f) if self.overlap else None
            filt = native_io.apply_filter(hb, ss, ds, self.filter, fail_f) if self.filter is not None else None
            if self.allele is not None and fail_f:
                # the records as they are written: after the overlap step and the filter
                native_io.allele_counts(hb, ds, self.allele[0], self.allele[1], fail_f, filt, self.allele_total)
            self.cons.write_consensus(hb, ss, ds, fail_f, filt)
            if self.sscs is not None:
                self.sscs.write_consensus_ss(hb, ss, fail_f, filt)
            lens = np.ctypeslib.as_array(ctypes.cast(ds.len, ctypes.POINTER(ctypes.c_int32)), (2 * F,))[:2 * fail_f] \
                if F else np.zeros(0, np.int32)
        st["batches"] += 1
        if filt is None:
            st["consensus_records"] += 2 * fail_f
            st["consensus_bases"] += int(lens.sum())
        else:
            # written records only; the families before a failure are filtered as any other
            why = filt & 0xff
            kept = why == 0
            st["consensus_records"] += 2 * int(kept.sum())
            st["consensus_bases"] += int(lens.reshape(-1, 2)[kept].sum())
            fc = self.filter_counts
            fc["filter_dropped"] += int((~kept).sum())
            fc["filter_masked"] += int((filt[kept] >> 8).sum())
            for bit, name in params_mod.FILT_REASONS:
                fc["filter_" + name] += int(((why & bit) != 0).sum())
            st["filter_dropped_families"], st["filter_masked_bases"] = fc["filter_dropped"], fc["filter_masked"]
        if ovl is not None:
            # written families only: the families before a failure count, the dropped ones do not
            per = ovl.reshape(-1, 3) if filt is None else ovl.reshape(-1, 3)[(filt & 0xff) == 0]
            for i, key in enumerate(("overlap_compared", "overlap_disagree", "overlap_changed")):
                self.overlap_counts[key] += int(per[:, i].sum())
            st.update(self.overlap_counts)
        st["wait_s"] += t1 - t0
        if fail_f < F:
            t = int(np.nonzero(hb.a["tab_proc"][:hb.s.n_tab] == fail_f)[0][0])
            exc_cut, filt_cut = int(hb.a["tab_exc_cut"][t]), int(hb.a["tab_filt_cut"][t])
        else:
            exc_cut, filt_cut = hb.s.n_side_exc, hb.s.n_side_filt
        self.excl.write(hb.a["side_exc"][:exc_cut])
        self.unproc.write(hb.a["side_filt"][:filt_cut])
        st["write_s"] += time.perf_counter() - t1
        if self.trace is not None:
            self.trace.append(("write", t1, time.perf_counter()))
        if fail_f < F:
            if kind == "exit":
                col = badchar_column(hb, fail_f, which, self.params.min_base_quality) if which < 4 else None
                if col is not None:
                    print("nucleotides = ", col)
                print(BADCHAR_LINE)
            _raise_reference(kind)
        if hb.end_kind == native_io.END_ERROR:
            ek, msg = hb.error()
            if ek == "exit":
                print(msg)
            _raise_reference(ek, msg)

    def run(self, batch_reads):
        """Ingest thread -> device -> writer, in input order."""
        n_buf = 4                       # filling, queued, on the device, being written
        free = queue.Queue()
        t0 = time.perf_counter()
        batches = [self.backend.host_batch(batch_reads) for _ in range(n_buf)]
        for hb in batches:
            free.put(hb)
        self.stats["alloc_s"] = time.perf_counter() - t0
        ready = queue.Queue()
        stop = threading.Event()

        first = [True]

        def fill(hb):
            """The next batch into ``hb``; a family larger than its capacities
            gets a batch twice as large, and so on (batch boundaries, and so
            --batch_reads, never change the outputs).  Returns the batch filled."""
            while True:
                try:
                    self.ing.next(hb)
                    return hb
                except native_io.IOError_ as e:
                    if "exceeds the batch capacities" not in str(e) or hb.reads >= (1 << 28):
                        raise
                hb = self.backend.host_batch(2 * hb.reads)
                batches.append(hb)

        def ingest():
            try:
                while not stop.is_set():
                    hb = free.get()
                    if hb is None:
                        return
                    t0 = time.perf_counter()
                    if first[0] and hb.s.cap_reads >= (1 << 18):
                        # the first batch at an eighth of the capacities: the
                        # device starts on it while the rest of the pipeline
                        # fills (batch boundaries never change the outputs); a
                        # family too large for it takes the full batch
                        first[0] = False
                        hb0 = hb
                        caps = (hb.s.cap_fam, hb.s.cap_tab, hb.s.cap_reads, hb.s.cap_cigar, hb.s.cap_bases)
                        hb.s.cap_fam, hb.s.cap_tab = caps[0] // 8, caps[1] // 8
                        hb.s.cap_reads, hb.s.cap_cigar, hb.s.cap_bases = caps[2] // 8, caps[3] // 8, caps[4] // 8
                        try:
                            self.ing.next(hb)
                        except native_io.IOError_ as e:
                            if "exceeds the batch capacities" not in str(e):
                                raise
                            (hb.s.cap_fam, hb.s.cap_tab, hb.s.cap_reads, hb.s.cap_cigar, hb.s.cap_bases) = caps
                            hb = fill(hb)
                        finally:
                            s = hb0.s
                            (s.cap_fam, s.cap_tab, s.cap_reads, s.cap_cigar, s.cap_bases) = caps
                    else:
                        first[0] = False
                        hb = fill(hb)
                    t1 = time.perf_counter()
                    self.stats["ingest_s"] += t1 - t0
                    if self.trace is not None:
                        self.trace.append(("ingest", t0, t1))
                    ready.put(hb)
                    if hb.end_kind != native_io.END_FULL:
                        return
            except BaseException as e:      # surfaced in the main thread
                ready.put(e)

        th = threading.Thread(target=ingest, name="dcr-ingest", daemon=True)
        th.start()
        pending = None
        try:
            while True:
                t0 = time.perf_counter()
                hb = ready.get()
                self.stats["idle_s"] += time.perf_counter() - t0
                if isinstance(hb, BaseException):
                    raise hb
                t0 = time.perf_counter()
                handle = self.backend.submit(hb)
                t1 = time.perf_counter()
                self.stats["submit_s"] += t1 - t0
                if self.trace is not None:
                    self.trace.append(("submit", t0, t1))
                if pending is not None:
                    self.finish(*pending, last_batch=False)
                    free.put(pending[0])
                pending = (hb, handle)
                if hb.end_kind != native_io.END_FULL:
                    break
            self.finish(*pending, last_batch=True)
            pending = None
            if self.allele is not None and getattr(self.backend, "device_writer", False):
                self.allele_total = self.backend.allele_counts()
        finally:
            stop.set()
            free.put(None)
            th.join()
            t0 = time.perf_counter()
            if self.allele is not None and getattr(self.backend, "device_writer", False):
                with contextlib.suppress(Exception):    # a kept backend does not keep the table
                    self.backend.set_allele_sites(None)
            self.backend.close()
            if hasattr(self.backend, "release"):
                self.backend.release(batches)
            self.stats["backend_close_s"] = time.perf_counter() - t0


def main(argv: Optional[list] = None, backend=None, rng=random, stats: Optional[dict] = None) -> int:
    """``main`` (:1426-1650).  ``backend`` defaults to the HIP library;
    ``stats`` (optional) receives per-stage times and output totals."""
    t_start = time.perf_counter()
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    params = ConsensusParams.from_args(args)
    group = _shard_group()
    if group is not None:
        return _main_sharded(args, params, backend, rng, stats, group)
    if args.gpus > 1:
        return _launch_ranks(argv, args.gpus)
    if backend is None:
        gpu_inflate(args.device)       # the GPU path reads its input through the device inflater too
    try:
        ing = native_io.Ingest(args.input_file, params.min_map_quality, params.min_reads, params.max_reads,
                               params.min_base_quality, args.threads, ss_meta=args.single_strand_output is not None)
        if args.verbose:
            print(args.input_file, "has been read.")
    except Exception:
        print("ERROR: input file not found. \n Please specify file name of a valid .bam file. "
              "Include the format in the file name.")
        raise ReferenceExit(1)
    if args.output_file is None:
        consensus_filename = "%s_cons.bam" % args.input_file[:-4]
    elif args.output_file.endswith(".bam"):
        consensus_filename = args.output_file
    else:
        print(OUTPUT_FORMAT_ERROR)
        raise ReferenceExit(1)
    _check_ss_output(args)
    ss_path = args.single_strand_output
    try:
        _load_genome(args, ing.header, stats)       # before any file is created
        _check_allele_output(args, ing.header)
        try:
            _check_metrics_output(args)
        except BaseException:
            _finish_allele(args, None, False)
            raise
    except BaseException:
        ing.close()
        raise
    met_path, met_total, done = args.metrics_output, None, False
    bmet_path, bmet_total = args.base_metrics_output, None
    gmet_path, gmet_total = args.genome_metrics_output, None
    al_total = None
    try:
        be = _as_backend(backend, params, args.device, ss_path is not None, ConsensusFilter.from_args(args),
                         met_path is not None, args.per_base_tags, bmet_path is not None, args.mate_overlap,
                         args.allele and args.allele[:2], args.genome_data)
        cons, excl, unproc, *rest = _open_writers(
            [consensus_filename, "%s_filteredreads.bam" % consensus_filename[:-4],
             "%s_filteredfamilies.bam" % consensus_filename[:-4]] + ([ss_path] if ss_path else []), ing.header, args,
            ing)
    except BaseException:
        _finish_metrics(met_path, None, False)      # no empty metrics file from a run that never started
        _finish_metrics(bmet_path, None, False)
        _finish_metrics(gmet_path, None, False)
        _finish_allele(args, None, False)
        raise
    sscs = rest[0] if rest else None
    ing.set_rng_state(rng.getstate())
    t_open = time.perf_counter()
    try:
        drv = _Driver(args, params, be, ing, cons, excl, unproc, sscs)
        met_total, bmet_total, gmet_total = drv.metrics_total, drv.base_metrics_total, drv.genome_total
        if stats is not None and "trace" in stats:
            drv.trace = stats["trace"]
        try:
            drv.run(max(args.batch_reads, 1))
        finally:
            if stats is not None:
                stats.update(drv.stats)
                stats["open_s"] = t_open - t_start
                stats["run_s"] = time.perf_counter() - t_open
        c = ing.counters()
        if stats is not None:
            stats.update(c)
        c.update(drv.filter_counts)
        c.update(drv.overlap_counts)
        al_total = drv.allele_total
        _allele_summary(c, al_total)
        _genome_summary(c, gmet_total)
        if args.verbose:
            print("\n Input file has been completely read \n")
        _print_summary(c)
        done = True
    finally:
        t_close = time.perf_counter()
        try:
            rng.setstate(ing.rng_state(rng.getstate()))
        finally:
            try:
                _close_all(excl.close, unproc.close, cons.close, *((sscs.close,) if sscs else ()))
            finally:
                t_wclose = time.perf_counter()
                try:
                    ing.close()
                finally:
                    try:
                        _finish_metrics(met_path, met_total, done)
                    finally:
                        try:
                            _finish_metrics(bmet_path, bmet_total, done, params_mod.base_metrics_json)
                        finally:
                            try:
                                _finish_metrics(gmet_path, gmet_total, done, params_mod.genome_metrics_json)
                            finally:
                                _finish_allele(args, al_total, done)
        if stats is not None:
            stats["close_s"] = time.perf_counter() - t_close
            stats["close_writers_s"] = t_wclose - t_close
    return 0


def _close_all(*closers):
    """Call every closer even when one raises; re-raise the first error."""
    err = None
    for fn in closers:
        try:
            fn()
        except BaseException as e:          # noqa: BLE001 - re-raised below
            if err is None:
                err = e
    if err is not None:
        raise err


def _open_writers(paths, header, args, ing=None):
    """BGZF writers for ``paths``; when one fails to open, the ones already
    open are closed (and ``ing`` with them) before the error propagates."""
    ws = []
    try:
        for p in paths:
            ws.append(native_io.BgzfWriter(p, header, args.compression_level, args.threads))
    except BaseException:
        _close_all(*(w.close for w in ws), *((ing.close,) if ing is not None else ()))
        raise
    return ws


def _print_summary(c):
    """The closing counts (:1642-1649)."""
    passed_reads, excluded_reads = c["passed"], c["excluded"]
    processed, excluded = c["processed"], c["filtered"]
    tot_r, tot_f = passed_reads + excluded_reads, processed + excluded
    print("\n A total of %d reads (%.2f %%) passed the initial quality filters." %
          (passed_reads, passed_reads / tot_r * 100))
    print("\n A total of %d reads (%.2f %%) were filtered out." % (excluded_reads, excluded_reads / tot_r * 100))
    print("\n A total of %d families (%.2f %%) were successfully processed to generate a consensus read." %
          (processed, processed / tot_f * 100))
    print("\n A total of %d families (%.2f %%) were filtered out due to not enough reads to generate a "
          "consensus read." % (excluded, excluded / tot_f * 100))
    if "filter_dropped" in c:
        # only with a --filter_* option: of the processed families
        dropped = c["filter_dropped"]
        print("\n A total of %d families (%.2f %%) were removed by the consensus filters."
              % (dropped, dropped / max(processed, 1) * 100))
        print("\n Families removed per rule: " + ", ".join("%s %d" % (name, c["filter_" + name])
                                                            for _, name in params_mod.FILT_REASONS))
        print("\n A total of %d bases were masked in the consensus reads that were written." % c["filter_masked"])
    if "overlap_compared" in c:
        # only with --mate_overlap: of the consensus reads that were written
        print("\n A total of %d reference positions covered by both reads of a pair were compared."
              % c["overlap_compared"])
        print("\n A total of %d of them held two different bases." % c["overlap_disagree"])
        print("\n A total of %d bases were changed where the reads of a pair overlap." % c["overlap_changed"])
    if "allele_sites" in c:
        # only with --allele_sites: the families that were written, each once per site
        print("\n Allele counts at %d sites: %d sites covered, %d molecules counted, %d of them discordant."
              % (c["allele_sites"], c["allele_covered"], c["allele_molecules"], c["allele_discordant"]))
    if "genome_levels" in c:
        # only with --genome: the consensus as called, per level
        print("\n Against the genome: " + "; ".join(
            "%s consensus %d aligned bases, %d mismatches, %d per million" % ((name.replace("_", "-"),) + tuple(t))
            for name, t in zip(params_mod.GMET_LEVELS, c["genome_levels"])) + ".")


# -- sharded mode: one process per GPU over ranges of whole families ---------------
#
# ``--gpus N`` relaunches the CLI as N ranks (torch.distributed.run, gloo for
# the small control messages; no data-path collective).  Rank 0 finds N-1
# split points, each the first read of a family (native_io.split_points);
# every rank runs the ordinary pipeline over its range into part files, and
# rank 0 concatenates the parts in order under the header, prints the ranks'
# stdout in order and the summary.  The result is the single-process result:
#   * a family never straddles two ranks, and a range that ends early
#     completes its last family there, as the reference does when the next
#     family's first read arrives;
#   * random.sample draws: the (population, size) of every call depends only
#     on the data, so each rank's exact starting state is the state after
#     the calls of the ranks before it.  A rank's ingest asks for that state
#     at its first random.sample call and waits for the earlier ranks' calls
#     (their own passes, or host-only count passes started on demand:
#     _StateExchange); no rank runs twice, and an input that is never
#     downsampled neither counts nor waits;
#   * the first failing rank ends the output exactly as the reference stops:
#     its parts are already cut where the reference stops writing, later
#     ranks are dropped and its exception is raised.

_EXC = {c.__name__: c for c in (IndexError, TypeError, ValueError, OverflowError, AttributeError, KeyError,
                                 ZeroDivisionError, UnicodeEncodeError)}
_BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _shard_group():
    """(dist, rank, world) when this process is a rank of the sharded CLI
    (DCR_SHARD=1, set by _launch_ranks, in a torch.distributed group of more
    than one process), else None.  torch is only imported in that case."""
    if os.environ.get("DCR_SHARD") != "1":
        return None
    import torch.distributed as dist
    if not dist.is_initialized():
        if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
            return None
        # gloo announces its connections on file descriptor 1: keep them out
        # of the CLI's stdout
        sys.stdout.flush()
        saved, null = os.dup(1), os.open(os.devnull, os.O_WRONLY)
        os.dup2(null, 1)
        try:
            dist.init_process_group("gloo")
        finally:
            os.dup2(saved, 1)
            os.close(saved)
            os.close(null)
    if dist.get_world_size() <= 1:
        return None
    return dist, dist.get_rank(), dist.get_world_size()


def _rank_device(args, local):
    """--device + the local rank, wrapped over the visible GPUs (counting them
    does not initialise the GPU on this stack)."""
    try:
        import torch
        n = torch.cuda.device_count()
    except Exception:
        n = 0
    return args.device + (local % n if n else local)


def _launch_ranks(argv, n):
    """N ranks of this CLI, one per GPU, started before anything here touches a GPU."""
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    rest = []
    skip = False
    for a in argv:                       # drop --gpus N / --gpus=N
        if skip:
            skip = False
            continue
        if a == "--gpus":
            skip = True
            continue
        if a.startswith("--gpus="):
            continue
        rest.append(a)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "duplexumiconsensusreads_amd.cli", *rest]
    env = dict(os.environ, DCR_SHARD="1")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def _run_range(args, params, backend, path, rng, rng_state, rng_range, parts, device, gate=None, header=b""):
    """The ordinary pipeline over one range of families into ``parts``;
    stdout, outcome, counters and random.sample calls in a dict.  ``gate``
    (optional): the ingest's state gate (native_io.Ingest.set_state_gate).
    ``header``: rank 0 writes the final files themselves, header first."""
    res = {"status": "ok", "exc_args": (), "calls": [], "counters": None, "stdout": "", "stats": {},
           "sizes": [0] * len(parts)}
    out = io.StringIO()
    if backend is None:
        gpu_inflate(device)
    ing = native_io.Ingest(path, params.min_map_quality, params.min_reads, params.max_reads,
                           params.min_base_quality, args.threads, rng_range[0], rng_range[1],
                           ss_meta=len(parts) > 3)
    be = _as_backend(backend, params, device, len(parts) > 3, ConsensusFilter.from_args(args),
                     args.metrics_output is not None, args.per_base_tags, args.base_metrics_output is not None,
                     args.mate_overlap, args.allele and args.allele[:2], args.genome_data)
    cons, excl, unproc, *rest = _open_writers(parts, header, args, ing)
    sscs = rest[0] if rest else None
    ing.set_rng_state(rng_state)
    if gate is not None:
        ing.set_state_gate(gate)
    drv = _Driver(args, params, be, ing, cons, excl, unproc, sscs)
    drv.ends_at_eof = rng_range[1] == -1
    try:
        with contextlib.redirect_stdout(out):
            drv.run(max(args.batch_reads, 1))
    except ReferenceExit as e:
        res["status"], res["exc_args"] = "exit", (e.code,)
    except tuple(_EXC.values()) as e:
        res["status"], res["exc_args"] = type(e).__name__, e.args
    except Exception as e:                  # not a reference outcome: reported as is
        res["status"], res["exc_args"] = "error", (repr(e),)
    finally:
        res["calls"] = ing.sample_calls()
        res["counters"] = dict(ing.counters(), **drv.filter_counts, **drv.overlap_counts)
        res["metrics"] = drv.metrics_total
        res["base_metrics"] = drv.base_metrics_total
        res["allele_counts"] = drv.allele_total
        res["genome_metrics"] = drv.genome_total
        res["stats"] = dict(drv.stats)
        res["stdout"] = out.getvalue()
        try:
            _close_all(excl.close, unproc.close, cons.close, *((sscs.close,) if sscs else ()))
        finally:
            ing.close()
        res["sizes"] = [os.path.getsize(p) for p in parts]
    return res


def _count_calls(path, params, rng_range, threads, stop, batch_reads=1 << 19):
    """The (population, size) of every random.sample call of one range, by a
    host-only ingest (host inflate, no device work, batches discarded): the
    calls depend only on the data (family and subfamily sizes), not on the
    generator's state.  Returns None (nothing to publish: the rank's own pass
    publishes) unless the ingest reached the end of the range or stopped where
    the reference stops; a stop request also gives None.  Batches are sized as
    the CLI's (``--batch_reads``), so a family the CLI can hold fits here."""
    ing = native_io.Ingest(path, params.min_map_quality, params.min_reads, params.max_reads,
                           params.min_base_quality, threads, rng_range[0], rng_range[1], host_inflate=True)
    complete = False
    try:
        hb = native_io.HostBatch(reads=max(batch_reads, 1))
        while not stop.is_set():
            ing.next(hb)
            if hb.end_kind != native_io.END_FULL:
                complete = True              # END_EOF, or END_ERROR: the calls up to the reference's stop
                break
    except Exception:  # noqa: BLE001 - an unfinished count is not published
        complete = False
    finally:
        calls = ing.sample_calls()
        ing.close()
    return calls if complete else None


class _StateExchange:
    """Rerun-free random.sample states for the sharded CLI.

    Rank r's exact starting state is the state after every call of the ranks
    before it.  Each rank's ingest is gated (``gate``): a rank that reaches
    its first random.sample call asks for that state, and waits only then; a
    rank that never samples never waits (its output does not depend on the
    state).  The calls of rank q are published in the process group's store
    by whichever finishes first: rank q's own pass, or a host-only count
    pass over rank q's range (``_count_calls``) that rank q starts in a
    thread once any rank has asked.  Nothing is counted, and nothing waits,
    for an input that is never downsampled."""

    _seq = 0

    _FAILED = b"failed"

    def __init__(self, dist, rank, world, s0, path, params, rng_range, threads, batch_reads=1 << 19):
        from datetime import timedelta
        _StateExchange._seq += 1       # every rank opens its exchanges in the same order
        self.store = dist.distributed_c10d._get_default_store()
        self.pre = "dcr_shard/%d/" % _StateExchange._seq
        self.rank, self.world, self.s0 = rank, world, s0
        self.wait_timeout = timedelta(hours=6)
        self.lock = threading.Lock()
        self.published = False
        self.gated_state = None
        self.wait_s = 0.0
        self.counted = False
        self.stop = threading.Event()
        self.th = None
        if rng_range is not None and rank < world - 1:
            # only later ranks read this rank's calls
            self.th = threading.Thread(target=self._counter, args=(path, params, rng_range, threads, batch_reads),
                                       name="dcr-count", daemon=True)
            self.th.start()

    def publish(self, calls):
        """``calls``: this range's random.sample calls; None marks the rank as
        failed before it knew them (a later rank's gate then raises instead
        of waiting for calls that never come)."""
        with self.lock:
            if self.published:
                return
            self.published = True
        val = self._FAILED if calls is None else np.asarray(calls, np.int32).reshape(-1).tobytes()
        self.store.set(self.pre + "calls%d" % self.rank, val)

    def _counter(self, path, params, rng_range, threads, batch_reads):
        from datetime import timedelta
        while not self.stop.is_set():
            try:
                self.store.wait([self.pre + "need"], timedelta(milliseconds=200))
                break
            except Exception:  # noqa: BLE001 - the store's timeout
                continue
        if self.stop.is_set() or self.published:
            return
        self.counted = True
        calls = _count_calls(path, params, rng_range, threads, self.stop, batch_reads)
        if calls is not None and not self.stop.is_set():
            self.publish(calls)

    def gate(self):
        """The ingest's state gate: the state after ranks 0..rank-1's calls."""
        t0 = time.perf_counter()
        self.store.set(self.pre + "need", b"1")
        keys = [self.pre + "calls%d" % q for q in range(self.rank)]
        if keys:
            self.store.wait(keys, self.wait_timeout)
        state = self.s0
        for k in keys:
            val = self.store.get(k)
            if val == self._FAILED:
                raise RuntimeError("%s: an earlier rank failed before publishing its random.sample calls" % k)
            flat = np.frombuffer(val, np.int32)
            state = native_io.py_replay(state, [(int(flat[2 * i]), int(flat[2 * i + 1]))
                                                for i in range(len(flat) // 2)])
        self.gated_state = state
        self.wait_s += time.perf_counter() - t0
        return state

    def close(self):
        self.stop.set()
        if self.th is not None:
            self.th.join()


def _copy_range(src, dst_fd, n, dst_off):
    """Bytes [0, n) of the file ``src`` into ``dst_fd`` at ``dst_off``, in the
    kernel (copy_file_range: no user-space round trip; a reflink where the
    file system has one)."""
    with open(src, "rb") as f:
        fd, done = f.fileno(), 0
        while done < n:
            try:
                k = os.copy_file_range(fd, dst_fd, n - done, done, dst_off + done)
            except OSError:
                k = 0
            if k <= 0:                      # no copy_file_range here: pread / pwrite
                chunk = os.pread(fd, min(n - done, 64 << 20), done)
                if not chunk:
                    raise IOError(f"{src}: short part file")
                k = os.pwrite(dst_fd, chunk, dst_off + done)
            done += k


def _part_dir(finals):
    """Where ranks 1..N-1 write their parts: a memory-backed directory when
    there is one with room (DCR_PART_DIR overrides), else beside the output.
    A part is written once there during the pass and once into the final
    file at the merge, from memory (no second trip through the file system)."""
    d = os.environ.get("DCR_PART_DIR")
    if d:
        return d
    try:
        st = os.statvfs("/dev/shm")
        if st.f_bavail * st.f_frsize >= (16 << 30):
            return "/dev/shm"
    except OSError:
        pass
    return os.path.dirname(os.path.abspath(finals[0]))


def _write_part_at(part, final, n, off, threads=4, mapped=False):
    """``n`` bytes of ``part`` written into ``final`` at ``off`` by a few
    threads, the part mapped.  ``mapped``: the final file's range is already
    allocated (rank 0's posix_fallocate before the offsets are broadcast), so
    the range is mapped too and the slices are plain memory copies (page
    faults of one file proceed in parallel, buffered writes to it take the
    inode lock in turn: 200 MB in 0.075 s against 0.15 s by pwrite on ext4).
    Otherwise the slices are pwritten from the mapped part (page-cache writes
    from user memory run about twice the rate of copy_file_range between two
    files)."""
    import mmap
    if not n:
        return
    fd = os.open(final, os.O_RDWR if mapped else os.O_WRONLY)
    try:
        with open(part, "rb") as f:
            mm = mmap.mmap(f.fileno(), n, prot=mmap.PROT_READ)
        step = max(1 << 20, -(-n // threads))
        step = (step + 4095) & ~4095
        starts = range(0, n, step)
        # a mapping past the end of the file faults (SIGBUS): map only a range the file holds
        if mapped and os.fstat(fd).st_size >= off + n:
            a0 = off & ~(mmap.ALLOCATIONGRANULARITY - 1)
            dm = mmap.mmap(fd, off + n - a0, offset=a0)
            views = [np.frombuffer(dm, np.uint8)[off - a0:], np.frombuffer(mm, np.uint8)]
            try:
                def copy(a):
                    np.copyto(views[0][a:a + step], views[1][a:a + step])
                with ThreadPoolExecutor(threads) as ex:
                    list(ex.map(copy, starts))
            finally:
                views.clear()                # the arrays export the mappings: released before closing
                dm.close()
                mm.close()
            return
        try:
            view = memoryview(mm)

            def put(a):
                b = min(a + step, n)
                while a < b:
                    a += os.pwrite(fd, view[a:b], off + a)
            if n <= step:
                put(0)
            else:
                with ThreadPoolExecutor(threads) as ex:
                    list(ex.map(put, starts))
        finally:
            view.release()
            mm.close()
    finally:
        os.close(fd)


def _merge_parallel(dist, rank, finals, header, args, sizes, upto, parts):
    """The output files, each byte written once into them.  Rank 0 wrote its
    range straight into the final files (header, records, EOF); rank r > 0
    writes its part (without its EOF block) at rank 0's length minus its EOF
    plus the sizes of parts 1..r-1, an exclusive scan of the part sizes every
    rank holds (``sizes[r][k]``), all ranks at once, into ranges rank 0 has
    allocated (posix_fallocate) before it broadcasts the offsets; rank 0 then
    puts the BGZF EOF block at the end."""
    eof = len(_BGZF_EOF)
    nf = len(finals)                         # 3, or 4 with the single-strand records' file
    if rank == 0:
        for k in range(nf):
            if sizes[0][k] == 0:             # rank 0 never opened its writers: the header alone
                w = native_io.BgzfWriter(finals[k], header, args.compression_level, args.threads)
                w.close()
                sizes[0][k] = os.path.getsize(finals[k])

    def ends_of(s0):
        return [s0[k] - eof + sum(max(sizes[r][k] - eof, 0) for r in range(1, upto)) for k in range(nf)]
    mapped = False
    if rank == 0 and upto > 1:
        # the finals' whole length allocated before any rank writes: the
        # ranks then copy into mapped ranges (no fault can meet a missing
        # block or the end of the file); a file system without fallocate
        # keeps the pwrite path
        mapped = True
        for k, e in enumerate(ends_of([sizes[0][j] for j in range(nf)])):
            fd = os.open(finals[k], os.O_RDWR)
            try:
                start = sizes[0][k] - eof
                if e + eof > start:
                    os.posix_fallocate(fd, start, e + eof - start)
            except OSError:
                mapped = False
            finally:
                os.close(fd)
    obj = [[sizes[0][k] for k in range(nf)], mapped]
    dist.broadcast_object_list(obj, src=0)
    s0, mapped = obj
    ends = ends_of(s0)
    for k in range(nf):
        off = s0[k] - eof
        for r in range(1, upto):
            n = max(sizes[r][k] - eof, 0)
            if r == rank and n:
                _write_part_at(parts[k], finals[k], n, off, mapped=mapped)
            off += n
    if rank == 0:
        for k in range(nf):
            fd = os.open(finals[k], os.O_WRONLY)
            try:
                os.pwrite(fd, _BGZF_EOF, ends[k])
                if os.fstat(fd).st_size != ends[k] + eof:   # already so when the finals were allocated
                    os.ftruncate(fd, ends[k] + eof)
            finally:
                os.close(fd)
    dist.barrier()


def _main_sharded(args, params, backend, rng, stats, group):
    dist, rank, world = group
    path = args.input_file
    try:
        header = native_io.bam_header(path)
        in_ok = True
    except Exception:
        in_ok = False
    if not in_ok:
        if rank == 0:
            print("ERROR: input file not found. \n Please specify file name of a valid .bam file. "
                  "Include the format in the file name.")
        raise ReferenceExit(1)
    if rank == 0 and args.verbose:
        print(path, "has been read.")
    if args.output_file is None:
        consensus_filename = "%s_cons.bam" % path[:-4]
    elif args.output_file.endswith(".bam"):
        consensus_filename = args.output_file
    else:
        if rank == 0:
            print(OUTPUT_FORMAT_ERROR)
        raise ReferenceExit(1)
    _check_ss_output(args, say=rank == 0)
    _load_genome(args, header, stats)       # every rank loads the FASTA itself
    _check_allele_output(args, header, say=rank == 0)   # every rank reads the sites: the ranks' tables line up
    _check_metrics_output(args, say=rank == 0)      # every rank: a bad path ends them all before any collective
    finals = [consensus_filename, "%s_filteredreads.bam" % consensus_filename[:-4],
              "%s_filteredfamilies.bam" % consensus_filename[:-4]]
    if args.single_strand_output is not None:
        finals.append(args.single_strand_output)
    obj = [native_io.split_points(path, world, params) if rank == 0 else None,
           rng.getstate() if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    splits, s0 = obj
    pts = [0] + [v for v in splits if v != -1]
    ranges = [(pts[i], pts[i + 1] if i + 1 < len(pts) else -1) for i in range(len(pts))]
    mine = ranges[rank] if rank < len(ranges) else None
    # rank 0 writes the final files themselves; the others write parts that
    # the merge puts in place once their offsets are known
    if rank == 0:
        parts = list(finals)
    else:
        pd = _part_dir(finals)
        parts = [os.path.join(pd, "%s.%d.part%d" % (os.path.basename(f), os.getppid(), rank)) for f in finals]
    local = int(os.environ.get("LOCAL_RANK", rank))
    device = _rank_device(args, local) if backend is None else args.device
    empty = {"status": "ok", "exc_args": (), "calls": [], "counters": None, "stdout": "", "stats": {},
             "sizes": [0] * len(finals)}
    result, used, rounds = empty, None, 0
    xch = _StateExchange(dist, rank, world, s0, path, params, mine, args.threads, args.batch_reads)
    done = False
    try:
        if mine is not None:
            result = _run_range(args, params, backend, path, rng, s0, mine, parts, device,
                                gate=xch.gate if rank > 0 else None, header=header if rank == 0 else b"")
            used, rounds = (xch.gated_state or s0), 1
        done = True
    finally:
        # this rank's calls for the later ranks (if no count pass published
        # them first); a rank that raised before knowing them publishes the
        # failure marker, so no later rank's gate waits for them
        xch.publish(result["calls"] if done else None)
        xch.close()
    # a safety net only: with the gate, a rank sampled from its exact state
    while True:
        results = [None] * world
        dist.all_gather_object(results, result)
        # this rank's exact starting state: the calls of the (ok) ranks before it
        state, target = s0, None
        for r in range(rank):
            if results[r]["status"] != "ok":
                break
            state = native_io.py_replay(state, results[r]["calls"])
        else:
            target = state
        # a rank that never sampled does not depend on the state
        again = bool(mine is not None and target is not None and result["calls"] and target != used)
        flags = [None] * world
        dist.all_gather_object(flags, again)
        if not any(flags):
            break
        if again:
            result = _run_range(args, params, backend, path, rng, target, mine, parts, device,
                                header=header if rank == 0 else b"")
            used = target
            rounds += 1
    if stats is not None:
        stats.update(result["stats"])
        stats["shard_rounds"] = rounds
        stats["state_wait_s"] = xch.wait_s
        stats["count_pass"] = xch.counted
    # the first failing rank ends the output as the reference stops; later
    # ranks are dropped (every rank derives the same cut from the results)
    fail = next((r for r in range(world) if results[r]["status"] != "ok"), None)
    upto = min((fail + 1) if fail is not None else world, len(ranges))
    t_merge = time.perf_counter()
    _merge_parallel(dist, rank, finals, header, args, [list(results[r]["sizes"]) for r in range(world)], upto,
                    parts)
    if stats is not None:
        stats["merge_s"] = time.perf_counter() - t_merge
    if rank == 0:
        sys.stdout.write("".join(results[r]["stdout"] for r in range(upto)))
        state = s0
        for r in range(upto):
            state = native_io.py_replay(state, results[r]["calls"])
        if stats is not None:
            stats["ranks"] = [results[r]["stats"] for r in range(world)]
    if rank != 0:
        for p in parts:
            if os.path.exists(p):
                os.remove(p)
        return 0
    rng.setstate(state)
    if fail is None:
        tot = {}
        for r in range(min(world, len(ranges))):
            for k, v in (results[r]["counters"] or {}).items():
                tot[k] = tot.get(k, 0) + v
        al_total = None
        if args.allele is not None:
            # integer sums too: a family is counted by the rank that writes it
            al_total = np.zeros((len(args.allele[0]), params_mod.ALLELE_COLS), np.uint64)
            for r in range(min(world, len(ranges))):
                if results[r].get("allele_counts") is not None:
                    al_total += results[r]["allele_counts"]
            _allele_summary(tot, al_total)
        gmet = None
        if args.genome_data is not None:
            gmet = np.zeros(params_mod.GMET_WORDS, np.uint64)
            for r in range(min(world, len(ranges))):
                if results[r].get("genome_metrics") is not None:
                    gmet += results[r]["genome_metrics"]
            _genome_summary(tot, gmet)
        if args.verbose:
            print("\n Input file has been completely read \n")
        _print_summary(tot)
        _finish_allele(args, al_total, True)
        _finish_metrics(args.genome_metrics_output, gmet, True, params_mod.genome_metrics_json)
        if args.metrics_output is not None:
            # integer sums: the ranks' totals add up to the single-process run's
            met = np.zeros(params_mod.MET_WORDS, np.uint64)
            for r in range(min(world, len(ranges))):
                if results[r].get("metrics") is not None:
                    met += results[r]["metrics"]
            _finish_metrics(args.metrics_output, met, True)
        if args.base_metrics_output is not None:
            bmet = np.zeros(params_mod.BMET_WORDS, np.uint64)
            for r in range(min(world, len(ranges))):
                if results[r].get("base_metrics") is not None:
                    bmet += results[r]["base_metrics"]
            _finish_metrics(args.base_metrics_output, bmet, True, params_mod.base_metrics_json)
        return 0
    _finish_metrics(args.metrics_output, None, False)
    _finish_metrics(args.base_metrics_output, None, False)
    _finish_metrics(args.genome_metrics_output, None, False)
    _finish_allele(args, None, False)
    st, ea = results[fail]["status"], results[fail]["exc_args"]
    if st == "exit":
        raise ReferenceExit(*ea)
    if st in _EXC:
        raise _EXC[st](*ea)
    raise RuntimeError(f"rank {fail}: {ea[0] if ea else st}")


if __name__ == "__main__":
    sys.exit(main())
