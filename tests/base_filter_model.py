"""The per-base consensus filters (include/dcr.h ``dcr_base_filter``,
``--filter_min_base_reads``, ``--filter_max_base_error_rate``,
``--filter_require_strand_agreement``) restated in plain Python over the
oracle's alignment (``oracle.dcr_oracle.consensus_core`` / ``reconstruct``).

Level 1: ``columns(cons)`` gives, for every base of a consensus record, the
d-index of the alignment column it came from.  Level 2: ``sources(a, b)``
lays the two single-strand consensus reads out as the duplex call does and
gives, per duplex alignment column, the base index of either strand.
``base_map`` joins them; ``masked_bases`` applies the rules; ``apply`` masks
decoded duplex records (the dict form ``tests.test_ss_output.records``
returns), together with ``--filter_min_base_quality`` and before the record
rules of tests/filter_model.py.

    res = family(subfamilies, P)               # cores of one family, or None
    masks = family_masks(bf, res)              # [masked base indices of ds 0, of ds 1]
    kept, words = apply(flt, ds_records, all_masks)
"""
import dataclasses

from oracle import dcr_oracle as O
from tests import filter_model as fm


@dataclasses.dataclass
class BaseFilter:
    min_base_reads: object = None              # (T, A, B)
    max_base_error_rate: object = None         # float
    require_strand_agreement: bool = False

    def argv(self):
        out = []
        if self.min_base_reads is not None:
            out += ["--filter_min_base_reads", ",".join(str(v) for v in self.min_base_reads)]
        if self.max_base_error_rate is not None:
            out += ["--filter_max_base_error_rate", repr(float(self.max_base_error_rate))]
        if self.require_strand_agreement:
            out += ["--filter_require_strand_agreement"]
        return out


def columns(cons):
    """Level 1.  (col, aln, n_de): for base i of the record's seq, ``col[i]``
    is the d-index and ``aln[i]`` the alignment column it came from; ``n_de``
    is the number of d-indices (the columns whose cons is not '+')."""
    cons = list(cons)
    t5 = 0
    while t5 < len(cons) and cons[t5] == "N":
        t5 += 1
    t3 = len(cons)
    while t3 > 0 and cons[t3 - 1] == "N":
        t3 -= 1
    col, aln, j = [], [], 0
    for t, c in enumerate(cons):
        if c == "+":
            continue
        if t5 <= t < t3 and c != "-":
            col.append(j)
            aln.append(t)
        j += 1
    return col, aln, j


def sources(a, b):
    """Level 2.  Per strand, per duplex alignment column: the index of the
    strand's base there, or None ('N' padding, '-', '+').  The layout is
    ``reconstruct`` itself, run over base indices instead of letters."""
    idx = [[str(i) for i in range(len(core["seq"]))] for core in (a, b)]
    al, _, _ = O.reconstruct([a["pos"], b["pos"]], [a["cigar"], b["cigar"]], idx, [a["qual"], b["qual"]])
    return [[int(v) if v.isdigit() else None for v in row] for row in al]


def base_map(a, b, r):
    """For every base i of duplex record ``r`` (called from the single-strand
    cores ``a`` and ``b``): (col_r(i), ia, ib, col_a(ia), col_b(ib)), None
    where a strand has no base in the column."""
    col_r, aln_r, n_de = columns(r["cons"])
    assert n_de == len(r["d"]) == len(r["e"]) and len(col_r) == len(r["seq"])
    col_a, col_b = columns(a["cons"])[0], columns(b["cons"])[0]
    assert len(col_a) == len(a["seq"]) and len(col_b) == len(b["seq"])
    src = sources(a, b)
    assert len(src[0]) == len(r["cons"])
    out = []
    for c, t in zip(col_r, aln_r):
        ia, ib = src[0][t], src[1][t]
        out.append((c, ia, ib, None if ia is None else col_a[ia], None if ib is None else col_b[ib]))
    return out


def support(a, b, r):
    """(aD, bD, aE, bE, cE) of every base of duplex record ``r``."""
    out = []
    for c, _, _, ca, cb in base_map(a, b, r):
        aD, aE = (a["d"][ca], a["e"][ca]) if ca is not None else (0, 0)
        bD, bE = (b["d"][cb], b["e"][cb]) if cb is not None else (0, 0)
        out.append((aD, bD, aE, bE, r["e"][c]))
    return out


def masks_base(bf, aD, bD, aE, bE, cE):
    m = False
    if bf.min_base_reads is not None:
        t, hi, lo = bf.min_base_reads
        m |= not (aD + bD >= t and max(aD, bD) >= hi and min(aD, bD) >= lo)
    if bf.max_base_error_rate is not None:
        m |= float(aE + bE) > bf.max_base_error_rate * float(aD + bD)
    if bf.require_strand_agreement:
        m |= cE > 0
    return m


def masked_bases(bf, a, b, r):
    """The indices of the bases of duplex record ``r`` the per-base rules mask."""
    return [i for i, s in enumerate(support(a, b, r)) if masks_base(bf, *s)]


def family(subs, P):
    """The six cores of one family from its four subfamilies' raw reads
    (dicts with pos, mapq, cigar, seq, qual), or None when the reference
    raises on it."""
    try:
        pre = []
        for sub in subs:
            ps = []
            for r in sub:
                cig, seq, qual = O.preprocess_read([tuple(x) for x in r["cigar"]], r["seq"], list(r["qual"]),
                                                   P.seqQ_threshold)
                ps.append(dict(r, cigar=cig, seq=seq, qual=qual))
            pre.append(ps)
        ss = [O.consensus_core(sub, P) for sub in pre]
        for s in ss:
            if any(q >= 95 for q in s["qual"]):          # pysam cannot store the aq / bq tag
                return None
        ds = [O.consensus_core([ss[0], ss[1]], P), O.consensus_core([ss[2], ss[3]], P)]
    except O.RefCrash:
        return None
    return dict(ss=ss, ds=ds)


def family_masks(bf, res):
    """[masked base indices of duplex record 0, of duplex record 1]."""
    return [masked_bases(bf, res["ss"][2 * j], res["ss"][2 * j + 1], res["ds"][j]) for j in range(2)]


def mask_record(flt, rec, base_mask):
    """(the record after masking, bases masked): the union of the per-base
    mask and ``--filter_min_base_quality``; every masked base becomes 'N' with
    quality min(q, 2) and is counted once."""
    seq, qual, n = list(rec["seq"]), list(rec["qual"]), 0
    hit = set(base_mask)
    for i, q in enumerate(qual):
        if i in hit or (flt.min_base_quality is not None and q < flt.min_base_quality):
            seq[i], qual[i] = "N", min(q, 2)
            n += 1
    return dict(rec, seq="".join(seq), qual=qual), n


def apply(flt, ds_records, masks):
    """tests.filter_model.apply with the per-base masks: ``masks[f]`` is
    ``family_masks`` of family f.  (the duplex records written, fam_filt)."""
    assert len(ds_records) == 2 * len(masks)
    rules = dataclasses.replace(flt, min_base_quality=None)       # the masking is done here
    kept, words = [], []
    for f, fam in enumerate(masks):
        pair, why, masked = [], 0, 0
        for j in range(2):
            m, n = mask_record(flt, ds_records[2 * f + j], fam[j])
            pair.append(m)
            masked += n
            why |= fm.reasons(rules, m)
        words.append(why | masked << 8)
        if why == 0:
            kept += pair
    return kept, words
