"""Consensus parameters and the host-built tables the kernels consume.

The reference reads its parameters from module globals set in ``main``
(DuplexUMIConsensusReads.py:1432-1469) and evaluates, for every aligned entry,
``10 ** (-q / 10)`` and the post-UMI adjustment (:665-676), then for every
column ``int(round(-10 * math.log10(e'), 0))`` (:699-709).  The device must be
bit-exact with those Python/glibc results, so everything transcendental is
tabulated here on the host with the reference's own expressions:

* ``match[v] = 1 - p'(v)`` and ``mismatch[v] = p'(v) / 5`` for quality codes
  0..255 plus the '+' and '-' rows (the two factors of :594-600);
* ``post_threshold = 1 - 10 ** (-min_base_quality / 10)`` (:679-680);
* ``qthresh``: the exact double boundaries at which the consensus quality
  changes, found by bisection over the IEEE-754 ordering with ``math.log10``
  (so the device only compares doubles).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import struct

import numpy as np

LUT_PLUS, LUT_DEL, LUT_N = 256, 257, 258
MAX_QTHRESH = 257


@dataclasses.dataclass(frozen=True)
class ConsensusParams:
    """The numeric CLI flags of the reference (:10-91), same defaults."""
    min_map_quality: int = 20        # -q
    min_base_quality: int = 20
    min_reads: int = 1
    max_reads: int = 100
    max_base_quality: int = 60
    base_quality_shift: int = 0
    error_rate_post_labeling: int = 0
    error_rate_pre_labeling: int = 0
    deletion_score: int = 30
    no_insertion_score: int = 30

    @classmethod
    def from_args(cls, args):
        return cls(min_map_quality=args.min_map_quality, min_base_quality=args.min_base_quality,
                   min_reads=args.min_reads, max_reads=args.max_reads,
                   max_base_quality=args.max_base_quality,
                   base_quality_shift=args.base_quality_shift,
                   error_rate_post_labeling=args.error_rate_post_labeling,
                   error_rate_pre_labeling=args.error_rate_pre_labeling,
                   deletion_score=args.deletion_score, no_insertion_score=args.no_insertion_score)

    @classmethod
    def from_oracle_dict(cls, d):
        """Map the golden-fixture parameter names onto the CLI names."""
        return cls(min_base_quality=d["seqQ_threshold"], min_reads=d["min_reads"],
                   max_reads=d["max_reads"], max_base_quality=d["max_base_quality"],
                   base_quality_shift=d["base_quality_shift"], error_rate_post_labeling=d["post"],
                   error_rate_pre_labeling=d["pre"], deletion_score=d["deletion_score"],
                   no_insertion_score=d["no_insertion_score"])


def _post_adjust(ps: float, post: int) -> float:
    # :669 / :672 / :676, Python evaluation order
    return post * (1 - ps) + (1 - post) * ps + post * ps * 4 / 5


def error_probabilities(p: ConsensusParams):
    """p'(v) for v = 0..255, then '+' and '-' (:665-676)."""
    out = []
    for v in range(256):
        qa = min(v - p.base_quality_shift, p.max_base_quality)
        out.append(_post_adjust(10 ** (-qa / 10), p.error_rate_post_labeling))
    out.append(_post_adjust(10 ** (-p.no_insertion_score / 10), p.error_rate_post_labeling))
    out.append(_post_adjust(10 ** (-p.deletion_score / 10), p.error_rate_post_labeling))
    return out


def phred_raw(x: float) -> int:
    """``int(round(-10 * math.log10(x), 0))`` for finite x > 0 (:704)."""
    return int(round(-10 * math.log10(x), 0))


def _d2u(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _u2d(u: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", u))[0]


_MIN_POS = 1                       # bits of the smallest subnormal
_MAX_FIN = _d2u(1.7976931348623157e308)


def first_x_with_phred_at_most(k: int) -> float:
    """Smallest positive finite double x with phred_raw(x) <= k
    (phred_raw is non-increasing in x; bisection on the bit pattern)."""
    lo, hi = _MIN_POS, _MAX_FIN
    if phred_raw(_u2d(hi)) > k:
        return math.inf
    if phred_raw(_u2d(lo)) <= k:
        return _u2d(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if phred_raw(_u2d(mid)) <= k:
            hi = mid
        else:
            lo = mid
    return _u2d(hi)


def quality_thresholds(max_q: int):
    """qthresh[i] = first x with phred_raw(x) <= i - 1, i = 0..max_q."""
    return [first_x_with_phred_at_most(i - 1) for i in range(max_q + 1)]


def consensus_quality(x: float, max_q: int, qthresh) -> int:
    """Device rule (also used by tests to pin the table against :699-709)."""
    if not (x > 0):            # x <= 0 or NaN: the reference's ValueError branch
        return max_q
    c = sum(1 for t in qthresh if x >= t)
    return max_q - c


class DcrParams(ctypes.Structure):
    """Mirror of ``dcr_params`` (include/dcr.h)."""
    _fields_ = [("min_base_quality", ctypes.c_int32), ("max_base_quality", ctypes.c_int32),
                ("base_quality_shift", ctypes.c_int32), ("error_rate_post_labeling", ctypes.c_int32),
                ("error_rate_pre_labeling", ctypes.c_int32), ("deletion_score", ctypes.c_int32),
                ("no_insertion_score", ctypes.c_int32), ("n_qthresh", ctypes.c_int32),
                ("match", ctypes.c_double * LUT_N), ("mismatch", ctypes.c_double * LUT_N),
                ("post_threshold", ctypes.c_double),
                ("qthresh", ctypes.c_double * MAX_QTHRESH)]


_CACHE = {}


def build_dcr_params(p: ConsensusParams) -> DcrParams:
    if p in _CACHE:
        return _CACHE[p]
    if not (0 <= p.max_base_quality <= MAX_QTHRESH - 1):
        raise ValueError(f"--max_base_quality must be in [0, {MAX_QTHRESH - 1}]")
    s = DcrParams()
    s.min_base_quality = p.min_base_quality
    s.max_base_quality = p.max_base_quality
    s.base_quality_shift = p.base_quality_shift
    s.error_rate_post_labeling = p.error_rate_post_labeling
    s.error_rate_pre_labeling = p.error_rate_pre_labeling
    s.deletion_score = p.deletion_score
    s.no_insertion_score = p.no_insertion_score
    for i, pe in enumerate(error_probabilities(p)):
        s.match[i] = 1 - pe          # :598
        s.mismatch[i] = pe / 5       # :600 (len(likelihoods) - 1 == 5)
    s.post_threshold = 1 - 10 ** (-p.min_base_quality / 10)
    th = quality_thresholds(p.max_base_quality)
    s.n_qthresh = len(th)
    for i, t in enumerate(th):
        s.qthresh[i] = t
    _CACHE[p] = s
    return s


# ---- consensus filters (include/dcr.h dcr_filter; not reference flags) ----------
FILT_MIN_READS, FILT_ERROR_RATE, FILT_NO_CALL, FILT_MEAN_QUAL, FILT_MASK_BASES = 1, 2, 4, 8, 16
FILT_REASONS = ((FILT_MIN_READS, "min_reads"), (FILT_ERROR_RATE, "max_read_error_rate"),
                (FILT_NO_CALL, "max_no_call_fraction"), (FILT_MEAN_QUAL, "min_mean_base_quality"))


class DcrFilter(ctypes.Structure):
    """Mirror of ``dcr_filter`` (include/dcr.h)."""
    _fields_ = [("active", ctypes.c_int32), ("min_base_quality", ctypes.c_int32),
                ("min_reads", ctypes.c_int32 * 3), ("reserved0", ctypes.c_int32),
                ("max_error_rate", ctypes.c_double * 2), ("max_no_call_fraction", ctypes.c_double),
                ("min_mean_base_quality", ctypes.c_double)]


# ---- per-base consensus filters (include/dcr.h dcr_base_filter) ------------------
BF_MIN_READS, BF_ERROR_RATE, BF_AGREEMENT = 1, 2, 4


class DcrBaseFilter(ctypes.Structure):
    """Mirror of ``dcr_base_filter`` (include/dcr.h)."""
    _fields_ = [("active", ctypes.c_int32), ("min_reads", ctypes.c_int32 * 3), ("max_error_rate", ctypes.c_double)]


# ---- consensus QC tables (include/dcr.h dcr_metrics; --metrics_output) ----------
MET_READS_BINS, MET_DEPTH_BINS, MET_ERR_BINS, MET_QUAL_BINS, MET_COL_BINS = 256, 64, 1002, 256, 512


class DcrMetrics(ctypes.Structure):
    """Mirror of ``dcr_metrics`` (include/dcr.h): every field uint64."""
    _fields_ = [("n", ctypes.c_uint64 * 8),
                ("ss_reads", ctypes.c_uint64 * MET_READS_BINS * 4),
                ("ds_depth", ctypes.c_uint64 * MET_DEPTH_BINS * MET_DEPTH_BINS),
                ("err_c", ctypes.c_uint64 * MET_ERR_BINS), ("err_s", ctypes.c_uint64 * MET_ERR_BINS),
                ("ss_qual", ctypes.c_uint64 * MET_QUAL_BINS), ("ds_qual", ctypes.c_uint64 * MET_QUAL_BINS),
                ("col", ctypes.c_uint64 * MET_COL_BINS * 3 * 2)]


MET_WORDS = ctypes.sizeof(DcrMetrics) // 8       # 10,716
MET_N_NAMES = ("families", "ss_bases", "ds_bases", "ds_no_calls", "ss_columns", "ds_columns")


def metrics_fields(words):
    """The tables of a ``uint64[MET_WORDS]`` block as a dict of array views,
    shaped as the struct's fields."""
    words = np.asarray(words).reshape(-1)
    if len(words) != MET_WORDS:
        raise ValueError("not a dcr_metrics block")
    out = {}
    for name, ct in DcrMetrics._fields_:
        f = getattr(DcrMetrics, name)
        shape, t = [], ct
        while hasattr(t, "_length_"):
            shape.append(t._length_)
            t = t._type_
        out[name] = words[f.offset // 8:(f.offset + f.size) // 8].reshape(shape)
    return out


def _trimmed(a):
    """A dense list without its trailing zeros."""
    nz = np.flatnonzero(a)
    return [int(v) for v in a[:int(nz[-1]) + 1]] if len(nz) else []


def metrics_json(words) -> str:
    """The ``--metrics_output`` file of a counter block: sorted keys and fixed
    separators, so the same counters always give the same bytes."""
    import json
    m = metrics_fields(words)
    doc = {"version": 1,
           "bins": {"ss_reads_max": MET_READS_BINS - 1, "ds_depth_max": MET_DEPTH_BINS - 1,
                    "column_max": MET_COL_BINS - 1, "error_rate_other": MET_ERR_BINS - 1}}
    for i, name in enumerate(MET_N_NAMES):
        doc[name] = int(m["n"][i])
    doc["ss_reads"] = {k: _trimmed(m["ss_reads"][i]) for i, k in enumerate(("A1", "B2", "B1", "A2"))}
    doc["ss_qual"], doc["ds_qual"] = _trimmed(m["ss_qual"]), _trimmed(m["ds_qual"])
    doc["ds_depth"] = [[int(h), int(lo), int(m["ds_depth"][h, lo])] for h, lo in zip(*np.nonzero(m["ds_depth"]))]
    for k in ("err_c", "err_s"):
        doc[k] = [[int(b), int(m[k][b])] for b in np.flatnonzero(m[k])]
    doc["col"] = {}
    for i, kind in enumerate(("ss", "ds")):
        rec = _trimmed(m["col"][i, 0])
        doc["col"][kind] = {"records": rec, "depth": [int(v) for v in m["col"][i, 1, :len(rec)]],
                            "errors": [int(v) for v in m["col"][i, 2, :len(rec)]]}
    return json.dumps(doc, sort_keys=True, separators=(",", ":")) + "\n"


# ---- per-base duplex QC tables (include/dcr.h dcr_base_metrics; --base_metrics_output) ----
BMET_DEPTH_BINS, BMET_ERR_BINS, BMET_QUAL_BINS, BMET_CYC_BINS = 64, 1002, 256, 512


class DcrBaseMetrics(ctypes.Structure):
    """Mirror of ``dcr_base_metrics`` (include/dcr.h): every field uint64."""
    _fields_ = [("n", ctypes.c_uint64 * 8),
                ("pair", ctypes.c_uint64 * 5 * 5 * 2),
                ("depth", ctypes.c_uint64 * BMET_DEPTH_BINS * BMET_DEPTH_BINS),
                ("err", ctypes.c_uint64 * BMET_ERR_BINS),
                ("qual", ctypes.c_uint64 * BMET_QUAL_BINS * 3),
                ("cyc", ctypes.c_uint64 * BMET_CYC_BINS * 6 * 2)]


BMET_WORDS = ctypes.sizeof(DcrBaseMetrics) // 8       # 12,068
BMET_N_NAMES = ("records", "bases", "both_strands", "a_only", "b_only", "neither", "disagree", "duplex_errors")
BMET_CYC_NAMES = ("bases", "no_calls", "disagree", "single", "depth", "errors")


def base_metrics_fields(words):
    """The tables of a ``uint64[BMET_WORDS]`` block as a dict of array views,
    shaped as the struct's fields."""
    words = np.asarray(words).reshape(-1)
    if len(words) != BMET_WORDS:
        raise ValueError("not a dcr_base_metrics block")
    out = {}
    for name, ct in DcrBaseMetrics._fields_:
        f = getattr(DcrBaseMetrics, name)
        shape, t = [], ct
        while hasattr(t, "_length_"):
            shape.append(t._length_)
            t = t._type_
        out[name] = words[f.offset // 8:(f.offset + f.size) // 8].reshape(shape)
    return out


def base_metrics_json(words) -> str:
    """The ``--base_metrics_output`` file of a counter block: sorted keys and
    fixed separators, so the same counters always give the same bytes."""
    import json
    m = base_metrics_fields(words)
    doc = {"version": 1,
           "bins": {"depth_max": BMET_DEPTH_BINS - 1, "cycle_max": BMET_CYC_BINS - 1,
                    "error_rate_other": BMET_ERR_BINS - 1, "error_rate_scale": 1000}}
    for i, name in enumerate(BMET_N_NAMES):
        doc[name] = int(m["n"][i])
    doc["pair"] = {"codes": "ACGTN", "read1": [[int(v) for v in row] for row in m["pair"][0]],
                   "read2": [[int(v) for v in row] for row in m["pair"][1]]}
    doc["depth"] = [[int(h), int(lo), int(m["depth"][h, lo])] for h, lo in zip(*np.nonzero(m["depth"]))]
    doc["err"] = [[int(b), int(m["err"][b])] for b in np.flatnonzero(m["err"])]
    doc["qual"] = {k: _trimmed(m["qual"][i]) for i, k in enumerate(("agree", "disagree", "single"))}
    doc["cycle"] = {}
    for j, read in enumerate(("read1", "read2")):
        n = len(_trimmed(m["cyc"][j, 0]))
        doc["cycle"][read] = {k: [int(v) for v in m["cyc"][j, w, :n]] for w, k in enumerate(BMET_CYC_NAMES)}
    return json.dumps(doc, sort_keys=True, separators=(",", ":")) + "\n"


def _numbers(text, conv, most, what):
    parts = text.split(",")
    if not 1 <= len(parts) <= most:
        raise ValueError(f"{what}: 1 to {most} comma-separated values, got {text!r}")
    vals = [conv(p) for p in parts]          # ValueError on a malformed number
    return vals + [vals[-1]] * (most - len(vals))


def filter_min_base_quality(text):
    v = int(text)
    if v < 0:
        raise ValueError("--filter_min_base_quality must be >= 0")
    return v


def filter_min_reads(text):
    """``T[,A[,B]]``: missing values repeat the last; T >= A >= B."""
    t, a, b = _numbers(text, int, 3, "--filter_min_reads")
    if not (t >= a >= b):
        raise ValueError("--filter_min_reads T,A,B needs T >= A >= B")
    return (t, a, b)


def _unit(text):
    v = float(text)
    if not 0.0 <= v <= 1.0:                   # NaN fails too
        raise ValueError(f"{text!r} is not in [0, 1]")
    return v


def filter_max_read_error_rate(text):
    """``C[,S]``: duplex and single-strand bounds; S defaults to C."""
    return tuple(_numbers(text, _unit, 2, "--filter_max_read_error_rate"))


def filter_max_no_call_fraction(text):
    return _unit(text)


def filter_min_base_reads(text):
    """``T[,A[,B]]`` per base: parsed and checked as ``--filter_min_reads`` is."""
    t, a, b = _numbers(text, int, 3, "--filter_min_base_reads")
    if not (t >= a >= b):
        raise ValueError("--filter_min_base_reads T,A,B needs T >= A >= B")
    return (t, a, b)


def filter_max_base_error_rate(text):
    return _unit(text)


def filter_min_mean_base_quality(text):
    v = float(text)
    if not 0.0 <= v < math.inf:
        raise ValueError("--filter_min_mean_base_quality must be a finite number >= 0")
    return v


# ---- overlapping mates (include/dcr.h dcr_set_mate_overlap; --mate_overlap) ------
OVL_OFF, OVL_MASK, OVL_CONSENSUS = 0, 1, 2
OVL_MODES = {"mask": OVL_MASK, "consensus": OVL_CONSENSUS}


def mate_overlap(text):
    """``mask`` or ``consensus``: the DCR_OVL_* mode."""
    if text not in OVL_MODES:
        raise ValueError("--mate_overlap must be 'mask' or 'consensus'")
    return OVL_MODES[text]


# ---- allele counts at given sites (include/dcr.h dcr_set_allele_sites; --allele_sites) ----
ALLELE_COLS = 8
ALLELE_MAX_SITES = 1 << 24
ALLELE_NAMES = ("A", "C", "G", "T", "N", "del", "discordant", "both")
ALLELE_HEADER = "#chrom\tpos\t" + "\t".join(ALLELE_NAMES) + "\tdepth\n"


def allele_min_base_quality(text):
    """``--allele_min_base_quality``: an int >= 0."""
    v = int(text)
    if v < 0:
        raise ValueError("--allele_min_base_quality must be >= 0")
    return v


def header_references(header: bytes):
    """The reference names of a BAM header as stored (magic, text, references)."""
    if header[:4] != b"BAM\1":
        raise ValueError("not a BAM header")
    (l_text,) = struct.unpack_from("<i", header, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", header, p)
    p += 4
    names = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", header, p)
        names.append(header[p + 4:p + 4 + ln - 1].decode("latin-1"))
        p += 4 + ln + 4
    return names


def allele_keys(path, references):
    """The sites of an ``--allele_sites`` file as the keys dcr_set_allele_sites
    takes: int64 ``tid << 32 | pos`` (pos 0-based), sorted by (tid, pos),
    duplicates merged.  Empty lines and lines starting with '#' are ignored;
    ``name<TAB>pos`` is one site, pos 1-based; ``name<TAB>start<TAB>end[...]``
    is BED, every position of [start, end), 0-based.  ``references``: the
    names of the input header, whose index is the tid.  A line that is
    neither, names no reference or holds a position outside the reference
    coordinates is a ValueError naming the line; so are more than
    ALLELE_MAX_SITES sites."""
    tid_of = {}
    for i, name in enumerate(references):
        tid_of.setdefault(name, i)
    spans = []
    with open(path, "r", encoding="latin-1") as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            where = "%s line %d" % (path, no)
            cols = line.split("\t")
            if len(cols) < 2:
                raise ValueError("%s: expected name<TAB>pos or name<TAB>start<TAB>end" % where)
            if cols[0] not in tid_of:
                raise ValueError("%s: %r is not a reference of the input header" % (where, cols[0]))
            try:
                nums = [int(c) for c in cols[1:3]]
            except ValueError:
                raise ValueError("%s: a position is not an integer" % where) from None
            if len(nums) == 1:
                start, end = nums[0] - 1, nums[0]
                if start < 0:
                    raise ValueError("%s: a 1-based position must be at least 1" % where)
            else:
                start, end = nums
                if start < 0:
                    raise ValueError("%s: negative start" % where)
                if end <= start:
                    raise ValueError("%s: end must be above start" % where)
            if end > (1 << 31):
                raise ValueError("%s: position beyond 2^31" % where)
            spans.append((tid_of[cols[0]], start, end))
    spans.sort()
    merged = []
    for tid, start, end in spans:
        if merged and merged[-1][0] == tid and start <= merged[-1][2]:
            merged[-1][2] = max(merged[-1][2], end)
        else:
            merged.append([tid, start, end])
    n = sum(end - start for _, start, end in merged)
    if n > ALLELE_MAX_SITES:
        raise ValueError("%s: %d sites, more than %d" % (path, n, ALLELE_MAX_SITES))
    if not merged:
        return np.zeros(0, np.int64)
    return np.concatenate([(np.int64(tid) << np.int64(32)) + np.arange(start, end, dtype=np.int64)
                           for tid, start, end in merged])


def allele_tsv(keys, table, references) -> str:
    """The ``--allele_counts_output`` file of a table (uint64 [len(keys), 8]):
    the header line, then one line per site in the keys' order with pos 1-based
    and depth the sum of the seven call columns; plain decimal integers, so the
    same counters always give the same bytes."""
    keys = np.asarray(keys, np.int64)
    table = np.asarray(table, np.uint64).reshape(len(keys), ALLELE_COLS)
    depth = table[:, :7].sum(axis=1, dtype=np.uint64)
    out = [ALLELE_HEADER]
    for k, row, d in zip(keys.tolist(), table.tolist(), depth.tolist()):
        out.append("%s\t%d\t%s\t%d\n" % (references[k >> 32], (k & 0xffffffff) + 1, "\t".join(map(str, row)), d))
    return "".join(out)


def allele_totals(table):
    """(sites, sites with depth > 0, molecules counted, discordant) of a table: the summary's line."""
    table = np.asarray(table, np.uint64).reshape(-1, ALLELE_COLS)
    depth = table[:, :7].sum(axis=1, dtype=np.uint64)
    return len(table), int((depth > 0).sum()), int(depth.sum()), int(table[:, 6].sum())


# ---- errors against a genome (include/dcr.h dcr_genome_metrics; --genome, --genome_metrics_output) ----
GMET_CYC_BINS, GMET_QUAL_BINS = 512, 256


class DcrGenomeMetrics(ctypes.Structure):
    """Mirror of ``dcr_genome_metrics`` (include/dcr.h): every field uint64."""
    _fields_ = [("n", ctypes.c_uint64 * 12 * 2),
                ("sub", ctypes.c_uint64 * 4 * 4 * 2 * 2),
                ("tri", ctypes.c_uint64 * 4 * 4 * 4 * 4 * 2 * 2),
                ("cyc", ctypes.c_uint64 * GMET_CYC_BINS * 2 * 2 * 2),
                ("qual", ctypes.c_uint64 * GMET_QUAL_BINS * 2 * 2)]


GMET_WORDS = ctypes.sizeof(DcrGenomeMetrics) // 8       # 6,232
GMET_LEVELS = ("single_strand", "duplex")
GMET_N_NAMES = ("records", "aligned_bases", "matches", "mismatches", "no_calls", "genome_unknown", "insertions",
                "inserted_bases", "deletions", "deleted_positions")


def genome_metrics_fields(words):
    """The tables of a ``uint64[GMET_WORDS]`` block as a dict of array views,
    shaped as the struct's fields."""
    words = np.asarray(words).reshape(-1)
    if len(words) != GMET_WORDS:
        raise ValueError("not a dcr_genome_metrics block")
    out = {}
    for name, ct in DcrGenomeMetrics._fields_:
        f = getattr(DcrGenomeMetrics, name)
        shape, t = [], ct
        while hasattr(t, "_length_"):
            shape.append(t._length_)
            t = t._type_
        out[name] = words[f.offset // 8:(f.offset + f.size) // 8].reshape(shape)
    return out


def genome_metrics_json(words) -> str:
    """The ``--genome_metrics_output`` file of a counter block: named keys,
    integers only, sorted keys and fixed separators, so the same counters
    always give the same bytes."""
    import json
    m = genome_metrics_fields(words)
    doc = {"version": 1, "bins": {"cycle_max": GMET_CYC_BINS - 1}, "codes": "ACGT"}
    for lv, level in enumerate(GMET_LEVELS):
        d = {name: int(m["n"][lv, i]) for i, name in enumerate(GMET_N_NAMES)}
        d["sub"], d["tri"], d["cycle"] = {}, {}, {}
        for j, read in enumerate(("read1", "read2")):
            d["sub"][read] = [[int(v) for v in row] for row in m["sub"][lv, j]]
            t = m["tri"][lv, j]
            d["tri"][read] = [[int(a), int(b), int(c), int(x), int(t[a, b, c, x])] for a, b, c, x in zip(*np.nonzero(t))]
            n = len(_trimmed(m["cyc"][lv, j, 0]))
            d["cycle"][read] = {"compared": [int(v) for v in m["cyc"][lv, j, 0, :n]],
                                "mismatches": [int(v) for v in m["cyc"][lv, j, 1, :n]]}
        n = len(_trimmed(m["qual"][lv, 0]))
        d["qual"] = {"compared": [int(v) for v in m["qual"][lv, 0, :n]],
                     "mismatches": [int(v) for v in m["qual"][lv, 1, :n]]}
        doc[level] = d
    return json.dumps(doc, sort_keys=True, separators=(",", ":")) + "\n"


def genome_totals(words):
    """Per level (aligned bases, mismatches, mismatches per million compared
    bases, an integer quotient): the summary's line."""
    n = genome_metrics_fields(words)["n"]
    out = []
    for lv in range(2):
        cmp_, mis = int(n[lv, 2]) + int(n[lv, 3]), int(n[lv, 3])
        out.append((int(n[lv, 1]), mis, mis * 1000000 // cmp_ if cmp_ else 0))
    return out


def header_sequences(header: bytes):
    """(name, length) of the references of a BAM header as stored."""
    names = header_references(header)
    (l_text,) = struct.unpack_from("<i", header, 4)
    p = 8 + l_text + 4
    out = []
    for name in names:
        (ln,) = struct.unpack_from("<i", header, p)
        (length,) = struct.unpack_from("<i", header, p + 4 + ln)
        out.append((name, length))
        p += 4 + ln + 4
    return out


_GENOME_LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _GENOME_LUT[ord(_c)] = _GENOME_LUT[ord(_c.lower())] = _i
for _c in b"\n\r":
    _GENOME_LUT[_c] = 255               # line ends: no base
del _i, _c


@dataclasses.dataclass(frozen=True, eq=False)
class Genome:
    """A genome as dcr_set_genome takes it: ``codes`` uint8, one per base (A C
    G T 0..3, anything else 4), the sequences of ``names`` back to back;
    ``ref_off`` int64 [len(names) + 1]; a sequence the FASTA lacks has length
    0.  ``load_s``: what the loading took."""
    codes: np.ndarray
    ref_off: np.ndarray
    names: tuple
    load_s: float = 0.0


def load_genome(path, sequences) -> Genome:
    """The FASTA ``path`` (plain text; ``.gz`` / ``.bgz`` or gzip bytes are a
    ValueError) reduced to the ``sequences`` [(name, length)] of the input
    header, in that order.  A sequence's name is the text after '>' up to the
    first whitespace; upper and lower case fold together; the lines may have
    any lengths, end in LF or CRLF, and the last needs no line end.  Sequences
    the header does not name are skipped; one of the header that the file lacks
    is absent (length 0).  A sequence whose length differs from the header's,
    and a name that occurs twice in the file, are ValueErrors naming it.  A
    ``.fai`` beside the file is not needed and not read.  The bytes go through
    one lookup table and one mask per kept sequence (numpy), never a loop per
    line."""
    import time
    t0 = time.perf_counter()
    if path.endswith((".gz", ".bgz")):
        raise ValueError("--genome %s: a compressed FASTA is not supported, give the plain text" % path)
    data = np.fromfile(path, np.uint8)
    if len(data) >= 2 and data[0] == 0x1f and data[1] == 0x8b:
        raise ValueError("--genome %s: a compressed FASTA is not supported, give the plain text" % path)
    if not sequences:
        raise ValueError("--genome: the input header names no sequence")
    want = {}
    for t, (name, _) in enumerate(sequences):
        want.setdefault(name, t)
    # the header lines: '>' at the start of the file or after a line end
    gt = np.flatnonzero(data == ord(">"))
    gt = gt[(gt == 0) | (data[np.maximum(gt, 1) - 1] == 10)]
    if len(data) and (len(gt) == 0 or gt[0] != 0) and np.any(_GENOME_LUT[data[:int(gt[0]) if len(gt) else None]] != 255):
        raise ValueError("--genome %s: text before the first '>' line" % path)
    ends = np.append(gt[1:], len(data))
    seen, spans = set(), {}
    for start, end in zip(gt.tolist(), ends.tolist()):         # one step per sequence
        width = 256
        while True:
            line = data[start:min(start + width, end)]
            nl = np.flatnonzero(line == 10)
            if len(nl) or start + width >= end:
                break
            width *= 16
        body = start + (int(nl[0]) + 1 if len(nl) else len(line))
        text = line[1:int(nl[0]) if len(nl) else len(line)].tobytes().decode("latin-1").split()
        name = text[0] if text else ""
        if name in seen:
            raise ValueError("--genome %s: the sequence %r occurs twice" % (path, name))
        seen.add(name)
        if name in want:
            spans[want[name]] = (body, end)
    lengths = [ln if t in spans else 0 for t, (_, ln) in enumerate(sequences)]
    ref_off = np.zeros(len(sequences) + 1, np.int64)
    np.cumsum(lengths, out=ref_off[1:])
    codes = np.empty(int(ref_off[-1]), np.uint8)
    for t, (body, end) in sorted(spans.items()):
        seq = _GENOME_LUT[data[body:end]]
        seq = seq[seq != 255]
        if len(seq) != lengths[t]:
            raise ValueError("--genome %s: the sequence %r has %d bases, the input header says %d"
                             % (path, sequences[t][0], len(seq), lengths[t]))
        codes[int(ref_off[t]):int(ref_off[t + 1])] = seq
    return Genome(codes, ref_off, tuple(name for name, _ in sequences), time.perf_counter() - t0)


@dataclasses.dataclass(frozen=True)
class ConsensusFilter:
    """The ``--filter_*`` options, parsed; None = that rule is off."""
    min_base_quality: object = None          # int
    min_reads: object = None                 # (T, A, B)
    max_read_error_rate: object = None       # (C, S)
    max_no_call_fraction: object = None      # float
    min_mean_base_quality: object = None     # float
    # the per-base rules (include/dcr.h dcr_base_filter; device writer only)
    min_base_reads: object = None            # (T, A, B)
    max_base_error_rate: object = None       # float
    require_strand_agreement: bool = False

    @classmethod
    def from_args(cls, args):
        """The filter of a parsed command line, or None when no option is given."""
        f = cls(args.filter_min_base_quality, args.filter_min_reads, args.filter_max_read_error_rate,
                args.filter_max_no_call_fraction, args.filter_min_mean_base_quality,
                getattr(args, "filter_min_base_reads", None), getattr(args, "filter_max_base_error_rate", None),
                bool(getattr(args, "filter_require_strand_agreement", False)))
        return f if f.active or f.base_active else None

    @property
    def base_active(self) -> int:
        """The DCR_BF_* bits of the per-base rules that are on."""
        return ((BF_MIN_READS if self.min_base_reads is not None else 0)
                | (BF_ERROR_RATE if self.max_base_error_rate is not None else 0)
                | (BF_AGREEMENT if self.require_strand_agreement else 0))

    def as_base_struct(self):
        """``dcr_base_filter`` of the per-base rules, or None when none is on."""
        if not self.base_active:
            return None
        s = DcrBaseFilter()
        s.active = self.base_active
        clamp = lambda v: max(-(1 << 31), min(v, (1 << 31) - 1))      # noqa: E731
        for i, v in enumerate(self.min_base_reads or (0, 0, 0)):
            s.min_reads[i] = clamp(v)
        s.max_error_rate = self.max_base_error_rate or 0.0
        return s

    @property
    def active(self) -> int:
        return ((FILT_MASK_BASES if self.min_base_quality is not None else 0)
                | (FILT_MIN_READS if self.min_reads is not None else 0)
                | (FILT_ERROR_RATE if self.max_read_error_rate is not None else 0)
                | (FILT_NO_CALL if self.max_no_call_fraction is not None else 0)
                | (FILT_MEAN_QUAL if self.min_mean_base_quality is not None else 0))

    def as_struct(self) -> DcrFilter:
        s = DcrFilter()
        s.active = self.active
        s.min_base_quality = min(self.min_base_quality or 0, 256)     # quality bytes are below 256
        clamp = lambda v: max(-(1 << 31), min(v, (1 << 31) - 1))      # noqa: E731
        for i, v in enumerate(self.min_reads or (0, 0, 0)):
            s.min_reads[i] = clamp(v)
        for i, v in enumerate(self.max_read_error_rate or (0.0, 0.0)):
            s.max_error_rate[i] = v
        s.max_no_call_fraction = self.max_no_call_fraction or 0.0
        s.min_mean_base_quality = self.min_mean_base_quality or 0.0
        return s
