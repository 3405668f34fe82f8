"""The overlapping mates (include/dcr.h ``dcr_set_mate_overlap``,
``--mate_overlap mask|consensus``) restated in plain Python over decoded BAM
records, the dict form ``tests.test_ss_output.records`` returns.

Duplex records come in pairs (paired-end 1, 2) per family, on the same
reference.  The map of a record is the written record's: ``pos``, the CIGAR
string and the length of ``seq``.

    recs, counts = apply("consensus", ds_records)     # counts: (compared, disagree, changed) per family
    census(ds_records)                                 # what kinds of positions the input holds
"""
import re

CIGAR_OP = re.compile(r"(\d+)([MIDNSHP=X])")
MAX_Q = 93


def ref_map(rec):
    """{reference position: base index} of a written record.  M, = and X give
    n bases on n consecutive positions; I and S n bases and no position; D and
    N n positions and no base; H and P neither.  A base index at or past the
    length of seq is not in the map."""
    out, p, i, L = {}, int(rec["pos"]), 0, len(rec["seq"])
    for n, op in CIGAR_OP.findall(rec["cigar"] or ""):
        n = int(n)
        if op in "M=X":
            for t in range(n):
                if i + t < L:
                    out[p + t] = i + t
            p += n
            i += n
        elif op in "IS":
            i += n
        elif op in "DN":
            p += n
    return out


def pairs(r0, r1):
    """[(p, i0, i1)] for every reference position in both maps, in order."""
    m0, m1 = ref_map(r0), ref_map(r1)
    return [(p, m0[p], m1[p]) for p in sorted(m0.keys() & m1.keys())]


def rule(mode, x, qx, y, qy):
    """(x', qx', y', qy') of one compared pair (neither base is 'N')."""
    if x == y:
        if mode == "mask":
            return x, qx, y, qy
        q = min(qx + qy, MAX_Q)
        return x, q, y, q
    if mode == "consensus" and qx != qy:
        return (x, qx - qy, x, qx - qy) if qx > qy else (y, qy - qx, y, qy - qx)
    return "N", min(qx, 2), "N", min(qy, 2)


def apply_pair(mode, r0, r1):
    """(mate 1 after, mate 2 after, (compared, disagree, changed)); every
    result from the values before the step."""
    assert mode in ("mask", "consensus")
    s = [list(r0["seq"]), list(r1["seq"])]
    q = [list(r0["qual"]), list(r1["qual"])]
    compared = disagree = changed = 0
    for _, i0, i1 in pairs(r0, r1):
        x, qx, y, qy = r0["seq"][i0], r0["qual"][i0], r1["seq"][i1], r1["qual"][i1]
        if x == "N" or y == "N":
            continue
        compared += 1
        disagree += x != y
        nx, nqx, ny, nqy = rule(mode, x, qx, y, qy)
        changed += ((nx, nqx) != (x, qx)) + ((ny, nqy) != (y, qy))
        s[0][i0], q[0][i0], s[1][i1], q[1][i1] = nx, nqx, ny, nqy
    return (dict(r0, seq="".join(s[0]), qual=q[0]), dict(r1, seq="".join(s[1]), qual=q[1]),
            (compared, disagree, changed))


def apply(mode, ds_records):
    """(the duplex records after the step, (compared, disagree, changed) per
    family) for the duplex records of whole families, two per family in order."""
    assert len(ds_records) % 2 == 0
    out, counts = [], []
    for f in range(len(ds_records) // 2):
        a, b, c = apply_pair(mode, ds_records[2 * f], ds_records[2 * f + 1])
        out += [a, b]
        counts.append(c)
    return out, counts


def totals(counts, kept=None):
    """The three summary counters over the families written (``kept``: one
    bool per family, None: all)."""
    rows = [c for f, c in enumerate(counts) if kept is None or kept[f]]
    return tuple(sum(c[i] for c in rows) for i in range(3))


def census(ds_records):
    """What the input holds, so that a test can assert it is not vacuous:
    pairs that overlap, pairs with a disagreement, disagreeing positions by
    the order of the qualities, agreeing positions and those whose quality sum
    stays within 93, positions skipped for an 'N', and pairs in which an indel
    or clip moves a base index away from p - pos."""
    c = dict(overlapping=0, with_disagreement=0, disagree=0, equal_q=0, mate1_higher=0, mate2_higher=0, agree=0,
             agree_sum_le_93=0, skipped_n=0, shifted=0)
    for f in range(len(ds_records) // 2):
        r0, r1 = ds_records[2 * f], ds_records[2 * f + 1]
        pr = pairs(r0, r1)
        c["overlapping"] += bool(pr)
        c["shifted"] += any(i0 != p - r0["pos"] or i1 != p - r1["pos"] for p, i0, i1 in pr)
        dis = 0
        for _, i0, i1 in pr:
            x, qx, y, qy = r0["seq"][i0], r0["qual"][i0], r1["seq"][i1], r1["qual"][i1]
            if x == "N" or y == "N":
                c["skipped_n"] += 1
            elif x == y:
                c["agree"] += 1
                c["agree_sum_le_93"] += qx + qy <= MAX_Q
            else:
                dis += 1
                c["equal_q" if qx == qy else "mate1_higher" if qx > qy else "mate2_higher"] += 1
        c["disagree"] += dis
        c["with_disagreement"] += dis > 0
    return c
