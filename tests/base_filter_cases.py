"""Hand-built families for the per-base filters, with the maps written out
by hand, and the helpers the CPU and GPU tests share: the families as a BAM,
the subfamilies of a packed batch as the model's input, and the model's
masks applied to host result arrays.

A family is four subfamilies (A1, B2, B1, A2) of reads on a 41-base template
at reference position 100; duplex record 0 is called from A1 and B2, which
carry the shape under test, duplex record 1 from two plain 10M subfamilies.
``MAPS[name]`` is duplex record 0's map: per duplex base
(col_r, ia, ib, col_a(ia), col_b(ib)), None where a strand has no base.
"""
import numpy as np

from duplexumiconsensusreads_amd.bam import AlignmentFile, BamHeader
from duplexumiconsensusreads_amd.records import AlignedSegment
from tests import base_filter_model as bm

REF = "ACGTTGCAAGCTTAGGCATCGATCGGATTACAGGCTTAACG"
N_ = None


def read(pos, cigar, qual=None, q=35, last=None):
    """A read at ``pos`` with the template's bases along ``cigar``; inserted
    bases are 'T'.  ``last``: another last base (a dissenting read)."""
    seq, p = "", pos - 100
    for op, n in cigar:
        if op == 0:
            seq += REF[p:p + n]
            p += n
        elif op == 1:
            seq += "T" * n
        elif op == 2:
            p += n
    if last is not None:
        seq = seq[:-1] + last
    return dict(pos=pos, mapq=40, cigar=[tuple(x) for x in cigar], seq=seq, qual=list(qual or [q] * len(seq)))


M10, M12 = [(0, 10)], [(0, 12)]
D2 = [(0, 5), (2, 2), (0, 5)]
D1 = [(0, 5), (2, 1), (0, 5)]
I5 = [(0, 5), (1, 1), (0, 5)]
I6 = [(0, 6), (1, 1), (0, 4)]
ID = [(0, 5), (1, 1), (2, 1), (0, 5)]
DI = [(0, 5), (2, 1), (1, 1), (0, 5)]
PLAIN = [read(100, M10), read(100, M10)]
LOWQ = [5, 5] + [30] * 10


def fam(a1, b2):
    return [a1, b2, PLAIN, PLAIN]


FAMILIES = {
    # two low-quality 5' bases in every A1 read and a last column on which the two reads differ:
    # A1's consensus is NN.........N, so t5 = 2 and t3 = 11 of 12 columns
    "ends": fam([read(100, M12, qual=LOWQ), read(100, M12, qual=LOWQ, last="A")], [read(100, M12)] * 2),
    # the layout ends at pos + len(seq): ten columns, so only three bases follow the deletion
    "5M2D5M": fam([read(100, D2)] * 2, [read(100, D2)] * 3),
    "ins_every_read": fam([read(100, I5)] * 2, [read(100, I5)] * 2),
    "ins_half": fam([read(100, I5)] * 2 + [read(100, M10)] * 2, [read(100, I5), read(100, M10)]),
    # a called insertion next to a deletion is one M over two columns (:797-840), both orders
    "5M1I1D5M": fam([read(100, ID)] * 3 + [read(100, D1)], [read(100, ID)] * 3 + [read(100, D1)]),
    "5M1D1I5M": fam([read(100, DI)] * 3 + [read(100, D1)], [read(100, DI)] * 3 + [read(100, D1)]),
    "a_del_b_not": fam([read(100, D2)] * 2, [read(100, M12)] * 3),
    "pos_a=pos_b+3": fam([read(103, M10)] * 2, [read(100, M10)] * 3),
    # strand a carries a weak insertion that the duplex call rejects: a '+' column, in no d / e list
    "a_weak_ins": fam([read(100, I5, q=21)] * 2 + [read(100, M10)], [read(100, M10)] * 2),
    # insertions one column apart in the two strands, one called and one rejected, both ways round:
    # the duplex CIGARs and lists have the same shape, the source strands differ
    "ins_5_and_6": fam([read(100, I5)] * 3 + [read(100, M10)], [read(100, I6, q=21)] * 2 + [read(100, M10)]),
    "ins_6_and_5": fam([read(100, I5, q=21)] * 2 + [read(100, M10)], [read(100, I6)] * 3 + [read(100, M10)]),
}


def same(cols):
    return [(c, c, c, c, c) for c in cols]


MAPS = {
    # strand a starts at column 2 (pos 102) with its base 0 on its own column 2, and has no base in column 11
    "ends": [(0, N_, 0, N_, 0), (1, N_, 1, N_, 1)] + [(c, c - 2, c, c, c) for c in range(2, 11)] + [(11, N_, 11, N_, 11)],
    # columns 5 and 6 are the deletion; base 5 sits on column 7 in all three records
    "5M2D5M": same(range(5)) + [(7, 5, 5, 7, 7)],
    "ins_every_read": same(range(11)),
    "ins_half": same(range(11)),
    # strands: ACGTTt-CAAG, ten bases under 10M, base 6 on column 7; the duplex of two 10M reads is plain
    "5M1I1D5M": same(range(6)) + [(c, c, c, c + 1, c + 1) for c in range(6, 10)],
    # strands: ACGTT-tCAAG, base 5 on column 6
    "5M1D1I5M": same(range(5)) + [(c, c, c, c + 1, c + 1) for c in range(5, 10)],
    # strand a: ACGTT--AAG (eight bases), strand b twelve
    "a_del_b_not": same(range(5)) + [(5, N_, 5, N_, 5), (6, N_, 6, N_, 6)] + [(c, c - 2, c, c, c) for c in (7, 8, 9)]
                   + [(10, N_, 10, N_, 10), (11, N_, 11, N_, 11)],
    "pos_a=pos_b+3": [(c, N_, c, N_, c) for c in range(3)] + [(c, c - 3, c, c - 3, c) for c in range(3, 10)]
                     + [(c, c - 3, N_, c - 3, N_) for c in (10, 11, 12)],
    # duplex ACGTT+GCAAG: alignment column 5 is '+', so base 5 is on alignment column 6, d-index 5,
    # and comes from base 6 of strand a (ACGTTnGCAAG) and base 5 of strand b
    "a_weak_ins": same(range(5)) + [(c, c + 1, c, c + 1, c) for c in range(5, 10)],
    # duplex ACGTTtG+CAA: base 5 is a's insertion alone; base 6 (column 6) is a's base 6 and b's base 5;
    # column 7 is '+'; bases 7.. are on alignment columns 8.., d-index 7.., from base 7.. of both strands
    "ins_5_and_6": same(range(5)) + [(5, 5, N_, 5, N_), (6, 6, 5, 6, 5)] + same((7, 8, 9)),
    # duplex ACGTT+GtCAA: column 5 is '+'; base 5 (column 6, d-index 5) is a's base 6 and b's base 5;
    # base 6 is b's insertion alone
    "ins_6_and_5": same(range(5)) + [(5, 6, 5, 6, 5), (6, N_, 6, N_, 6)] + same((7, 8, 9)),
}

HEADER = BamHeader("@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:248956422\n", ["chr1"], [248956422])
SUB_FLAG = ((99, "A"), (163, "B"), (83, "B"), (147, "A"))          # A1 B2 B1 A2


def write_families(path, families, shift=1000):
    """``families``: lists of four subfamilies; family f's reads move to reference position + f * shift."""
    with AlignmentFile(path, "wb", header=HEADER) as out:
        for f, subs in enumerate(families):
            for k, ((flag, strand), sub) in enumerate(zip(SUB_FLAG, subs)):
                for j, rd in enumerate(sub):
                    r = AlignedSegment()
                    r.query_name = f"f{f}_{k}_{j}"
                    r.flag = flag
                    r.reference_id = 0
                    r.reference_start = rd["pos"] + f * shift
                    r.mapping_quality = rd["mapq"]
                    r.cigartuples = list(rd["cigar"])
                    r.query_sequence = rd["seq"]
                    r.query_qualities = list(rd["qual"])
                    r.set_tags([("MI", f"{f}/{strand}"), ("RX", "ACGTACGT-TTGGCCAA" if strand == "A" else
                                 "TTGGCCAA-ACGTACGT")])
                    out.write(r)
    return path


def batch_subfamilies(pk, f):
    """The four subfamilies of family ``f`` of a packed batch as the model's reads."""
    subs = []
    for s in range(4 * f, 4 * f + 4):
        sub = []
        for i in range(int(pk.sub_off[s]), int(pk.sub_off[s + 1])):
            o, n = int(pk.seq_off[i]), int(pk.seq_len[i])
            c0, cn = int(pk.cig_off[i]), int(pk.cig_n[i])
            sub.append(dict(pos=int(pk.read_pos[i]), mapq=int(pk.read_mapq[i]),
                            cigar=[(int(v) & 15, int(v) >> 4) for v in pk.cigar[c0:c0 + cn]],
                            seq=pk.bases[o:o + n].tobytes().decode(), qual=pk.quals[o:o + n].tolist()))
        subs.append(sub)
    return subs


def mask_arrays(flt, masks, ds_col_off, ds_len, seq, qual):
    """Apply the model's per-base masks to host duplex arrays in place (the
    host filter that runs next masks the bases below
    ``--filter_min_base_quality``; masking a base twice changes nothing).
    Returns the model's count of masked bases per family
    (``base_filter_model.mask_record``: the union of the per-base masks and
    the quality rule over the qualities as called, each base once); the host
    filter's own count, taken over arrays already masked, is not used."""
    out = np.zeros(len(masks), np.int32)
    for f, fam_masks in enumerate(masks):
        for j, idx in enumerate(fam_masks):
            ro, n = int(ds_col_off[2 * f + j]), int(ds_len[2 * f + j])
            rec = dict(seq=seq[ro:ro + n].tobytes().decode(), qual=qual[ro:ro + n].tolist())
            m, count = bm.mask_record(flt, rec, idx)
            seq[ro:ro + n] = np.frombuffer(m["seq"].encode(), np.uint8)
            qual[ro:ro + n] = m["qual"]
            out[f] += count
    return out


def model_masks(bf, pk, n_fam, P, cache=None, key0=0):
    """``family_masks`` of families [0, n_fam) of a packed batch (None: the
    reference raises on the family).  ``cache``: cores by ``key0 + f``, shared
    between runs over the same input in the same family order."""
    out = []
    for f in range(n_fam):
        if cache is not None and key0 + f in cache:
            res = cache[key0 + f]
        else:
            res = bm.family(batch_subfamilies(pk, f), P)
            if cache is not None:
                cache[key0 + f] = res
        out.append(None if res is None else bm.family_masks(bf, res))
    return out
