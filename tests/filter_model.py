"""The consensus filters (include/dcr.h ``dcr_filter``, ``--filter_*``)
restated in plain Python over decoded BAM records, the dict form
``tests.test_ss_output.records`` returns.

Duplex records come in pairs (paired-end 1, 2) per family.  ``aD bD aE bE
cE`` are read from the record's own tags; ``E`` is ``round(float(tag), 3)``:
the tag is a float32 and the value the filter compares is the double already
rounded to three decimals.

    flt = Filter(min_base_quality=20, min_reads=(3, 2, 1), ...)
    kept_ds, words = apply(flt, ds_records)
    kept_ss = keep_ss(words, ss_records)
"""
import dataclasses

MIN_READS, ERROR_RATE, NO_CALL, MEAN_QUAL = 1, 2, 4, 8


@dataclasses.dataclass
class Filter:
    min_base_quality: object = None        # int
    min_reads: object = None               # (T, A, B)
    max_read_error_rate: object = None     # (C, S)
    max_no_call_fraction: object = None    # float
    min_mean_base_quality: object = None   # float

    def argv(self):
        """The command line options of this filter (floats by repr: exact)."""
        out = []
        if self.min_base_quality is not None:
            out += ["--filter_min_base_quality", str(self.min_base_quality)]
        if self.min_reads is not None:
            out += ["--filter_min_reads", ",".join(str(v) for v in self.min_reads)]
        if self.max_read_error_rate is not None:
            out += ["--filter_max_read_error_rate", ",".join(repr(float(v)) for v in self.max_read_error_rate)]
        if self.max_no_call_fraction is not None:
            out += ["--filter_max_no_call_fraction", repr(float(self.max_no_call_fraction))]
        if self.min_mean_base_quality is not None:
            out += ["--filter_min_mean_base_quality", repr(float(self.min_mean_base_quality))]
        return out


def tag(rec, name):
    for t in rec["tags"]:
        if t[0] == name:
            return t[2]
    raise KeyError(name)


def scalars(rec):
    """aD, bD, aE, bE, cE of a duplex record."""
    return (int(tag(rec, "aD")), int(tag(rec, "bD")), round(float(tag(rec, "aE")), 3),
            round(float(tag(rec, "bE")), 3), round(float(tag(rec, "cE")), 3))


def mask(flt, rec):
    """(the record after masking, bases masked): every base whose quality is
    below min_base_quality becomes 'N' with quality min(q, 2); nothing else
    of the record changes."""
    if flt.min_base_quality is None:
        return rec, 0
    seq, qual, n = list(rec["seq"]), list(rec["qual"]), 0
    for i, q in enumerate(qual):
        if q < flt.min_base_quality:
            seq[i], qual[i] = "N", min(q, 2)
            n += 1
    return dict(rec, seq="".join(seq), qual=qual), n


def reasons(flt, rec):
    """Reason bits of one (masked) duplex record; 0: it passes."""
    aD, bD, aE, bE, cE = scalars(rec)
    why = 0
    if flt.min_reads is not None:
        t, a, b = flt.min_reads
        if not (aD + bD >= t and max(aD, bD) >= a and min(aD, bD) >= b):
            why |= MIN_READS
    if flt.max_read_error_rate is not None:
        c, s = flt.max_read_error_rate
        if not (cE <= c and aE <= s and bE <= s):
            why |= ERROR_RATE
    L = len(rec["seq"])
    if flt.max_no_call_fraction is not None:
        if float(rec["seq"].count("N")) > flt.max_no_call_fraction * float(L):
            why |= NO_CALL
    if flt.min_mean_base_quality is not None:
        if float(sum(rec["qual"])) < flt.min_mean_base_quality * float(L):
            why |= MEAN_QUAL
    return why


def apply(flt, ds_records):
    """(the duplex records written, the outcome word of every family) for the
    duplex records of whole families, two per family in order."""
    assert len(ds_records) % 2 == 0
    kept, words = [], []
    for f in range(len(ds_records) // 2):
        pair, why, masked = [], 0, 0
        for rec in ds_records[2 * f:2 * f + 2]:
            m, n = mask(flt, rec)
            pair.append(m)
            masked += n
            why |= reasons(flt, m)
        words.append(why | masked << 8)
        if why == 0:                       # the pair rule: both or neither
            kept += pair
    return kept, words


def keep_ss(words, ss_records):
    """The single-strand records written: the four of every kept family."""
    assert len(ss_records) == 4 * len(words)
    return [r for f, w in enumerate(words) if w & 0xff == 0 for r in ss_records[4 * f:4 * f + 4]]
