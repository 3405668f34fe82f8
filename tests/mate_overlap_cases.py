"""Hand-built families for ``--mate_overlap``, shared by the CPU and the GPU
tests, and the helpers both use.

A family is four subfamilies (A1, B2, B1, A2) of reads on a 60-base template
at reference position 100.  Duplex record 0 (mate 1) is called from A1 and B2,
duplex record 1 (mate 2) from B1 and A2; both subfamilies of a mate hold the
same reads, so the mate is those reads' shape, unless a mate is given as a
tuple (the first strand's reads, the second strand's).  ``CASES[name]`` is
(mate 1's reads, mate 2's reads, what the plain run must give): the ``pos`` and
CIGAR of both duplex records, so that a case cannot silently lose its shape,
and the census of the pair (tests/mate_overlap_model.py ``census``) restricted
to the keys the case is about.
"""
from duplexumiconsensusreads_amd.bam import AlignmentFile
from duplexumiconsensusreads_amd.records import AlignedSegment
from tests.base_filter_cases import HEADER, SUB_FLAG

REF = "ACGTTGCAAGCTTAGGCATCGATCGGATTACAGGCTTAACGTCAGGTCCATAGCTTGACA"
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def read(pos, cigar, sub=(), q=35, lowq=()):
    """A read at ``pos`` with the template's bases along ``cigar`` (inserted
    bases are 'T'); the query indices in ``sub`` carry another base, those in
    ``lowq`` quality 5 (masked to 'N' before the consensus)."""
    seq, p = "", pos - 100
    for op, n in cigar:
        if op == 0:
            seq += REF[p:p + n]
            p += n
        elif op == 1:
            seq += "T" * n
        elif op == 2:
            p += n
    seq = "".join(OTHER[c] if i in sub else c for i, c in enumerate(seq))
    return dict(pos=pos, mapq=40, cigar=[tuple(x) for x in cigar], seq=seq,
                qual=[5 if i in lowq else q for i in range(len(seq))])


def M(n):
    return [(0, n)]


I5 = [(0, 5), (1, 1), (0, 8)]


def case(m1, m2, pos, cigar, **census):
    return (m1, m2, dict(pos=pos, cigar=cigar, census=census))


CASES = {
    "disjoint": case([read(100, M(10))] * 2, [read(120, M(10))] * 2, (100, 120), ("10M", "10M"), overlapping=0),
    "adjacent": case([read(100, M(10))] * 2, [read(110, M(10))] * 2, (100, 110), ("10M", "10M"), overlapping=0),
    "one_base": case([read(100, M(10))] * 2, [read(109, M(10), sub=(0,))] * 2, (100, 109), ("10M", "10M"),
                     overlapping=1, disagree=1, equal_q=1, agree=0),
    # identical spans, a disagreement at the first and at the last base; the same reads on both sides
    # but for the two bases: equal qualities
    "identical": case([read(100, M(12))] * 2, [read(100, M(12), sub=(0, 11))] * 2, (100, 100), ("12M", "12M"),
                      disagree=2, equal_q=2, agree=10),
    # mate 2 inside mate 1, its first and last base dissenting; mate 2 is called from weaker reads
    "inside": case([read(100, M(20))] * 2, [read(105, M(8), sub=(0, 7), q=22)], (100, 105), ("20M", "8M"),
                   disagree=2, mate1_higher=2, agree=6),
    # mate 2 starts left of mate 1 (no golden pair does) and is the stronger one
    "pos1<pos0": case([read(108, M(12), sub=(0, 3), q=22)], [read(100, M(12))] * 2, (108, 100), ("12M", "12M"),
                      disagree=2, mate2_higher=2, agree=2),
    # a deletion in mate 1 across overlap positions 105..107: mate 2's bases there have no partner (the
    # reference's layout ends at pos + len(seq), so two bases follow the deletion); the first base after
    # it dissents
    "deletion": case([read(100, [(0, 5), (2, 3), (0, 8)], sub=(5,))] * 2, [read(100, M(16))] * 2, (100, 100),
                     ("5M3D2M", "16M"), shifted=1, disagree=1, agree=6),
    # an insertion in mate 1 inside the overlap (the duplex CIGAR keeps an I only when one strand lacks it):
    # the bases after it pair one index apart; mate 2 dissents at position 106
    "insertion": case(([read(100, I5)] * 3 + [read(100, M(13))], [read(100, M(13))] * 2),
                      [read(100, M(13), sub=(6,))] * 2, (100, 100), ("5M1I8M", "13M"), shifted=1, disagree=1, agree=12),
    # the same insertion just before the first overlap position, which dissents
    "insertion_first": case(([read(100, I5)] * 3 + [read(100, M(13))], [read(100, M(13))] * 2),
                            [read(105, M(8), sub=(0,))] * 2, (100, 105), ("5M1I8M", "8M"), shifted=1, disagree=1,
                            agree=7),
    # an 'N' on either side, next to a disagreement: the 'N' positions are not compared
    "n_either_side": case([read(100, M(12), lowq=(2,))] * 2, [read(100, M(12), sub=(3,), lowq=(4,))] * 2,
                          (100, 100), ("12M", "12M"), skipped_n=2, disagree=1, agree=9),
    # one weak read per strand, the second strand four bases long: qualities 49 where both strands call
    # (49 + 49 crosses 93) and 21 where one does (42 does not)
    "quality_sums": case(([read(100, M(12), q=21)], [read(100, M(4), q=21)]),
                         ([read(100, M(12), q=21)], [read(100, M(4), q=21)]), (100, 100), ("12M", "12M"),
                         agree=12, agree_sum_le_93=8),
    "sum_crosses_93": case([read(100, M(12))] * 3, [read(100, M(12))] * 3, (100, 100), ("12M", "12M"),
                           agree=12, agree_sum_le_93=0),
}


def families(names=None):
    """The four subfamilies of each named case, in order."""
    out = []
    for name in names or CASES:
        m1, m2, _ = CASES[name]
        out.append([*(m1 if isinstance(m1, tuple) else (m1, m1)), *(m2 if isinstance(m2, tuple) else (m2, m2))])
    return out


def write_families(path, fams, shift=1000):
    """``fams``: lists of four subfamilies; family f's reads move to reference position + f * shift."""
    with AlignmentFile(path, "wb", header=HEADER) as out:
        for f, subs in enumerate(fams):
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


def dissenting_copy(src, dst, every=23):
    """A copy of the BAM ``src`` whose mates disagree (the generator's mates
    read one template, so their consensus reads agree everywhere): the reverse
    reads (flags 83 and 147: mate 2's subfamilies) carry another base on the
    reference positions that are multiples of ``every``, so that mate 2's
    consensus calls it.  In every second family (by the MI's number) the first
    read of each such subfamily (name ..._0) keeps the template's base: a
    dissenting read lowers mate 2's quality there, so that the disagreements
    come with equal and with unequal qualities."""
    with AlignmentFile(src, "rb") as f, AlignmentFile(dst, "wb", header=f.header) as out:
        for r in f:
            keep = int(r.get_tag("MI").split("/")[0]) % 2 == 0 and r.query_name.endswith("_0")
            if r.flag & 16 and not keep:
                seq, qual = list(r.query_sequence), list(r.query_qualities)
                p, i = r.reference_start, 0
                for op, n in r.cigartuples:
                    if op in (0, 7, 8):
                        for t in range(n):
                            if (p + t) % every == 0 and seq[i + t] in OTHER:
                                seq[i + t] = OTHER[seq[i + t]]
                        p += n
                        i += n
                    elif op in (1, 4):
                        i += n
                    elif op in (2, 3):
                        p += n
                r.query_sequence = "".join(seq)
                r.query_qualities = qual
            out.write(r)
    return dst


def summary_lines(totals):
    """What the CLI prints after the reference's summary lines (and the filters')."""
    return ("\n A total of %d reference positions covered by both reads of a pair were compared.\n"
            "\n A total of %d of them held two different bases.\n"
            "\n A total of %d bases were changed where the reads of a pair overlap.\n" % tuple(totals))
