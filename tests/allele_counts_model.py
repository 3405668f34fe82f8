"""The allele counts at given sites (include/dcr.h ``dcr_set_allele_sites``,
``--allele_sites`` / ``--allele_counts_output``) restated in plain Python over
decoded BAM records, the dict form ``tests.test_ss_output.records`` returns.

Duplex records come in pairs (paired-end 1, 2) per family, on the same
reference.  Only written records count, so the model takes what a run wrote.
The map of a record is the overlap step's (tests/mate_overlap_model.py
``ref_map``: ``pos``, the CIGAR string, the length of ``seq``) with one
addition: a D run gives the call ``del`` on each of its positions.  The walk
ends at the last operation or once the base index has reached the length of
``seq``.

    table(sites, ds_records, min_q)      # [[A, C, G, T, N, del, discordant, both]] per site
"""
import re

CIGAR_OP = re.compile(r"(\d+)([MIDNSHP=X])")
A, C, G, T, N, DEL, DISCORDANT, BOTH = range(8)
COLS = 8
HEADER = "#chrom\tpos\tA\tC\tG\tT\tN\tdel\tdiscordant\tboth\tdepth\n"


def calls(rec, min_q=0):
    """{reference position: call 0..5} of a written record.  M, = and X give
    n bases on n consecutive positions; D gives n positions calling ``del``; N
    gives n positions without a call; I and S n bases and no position; H and P
    neither.  A base calls A C G T by its letter, anything else N; a base whose
    quality is below ``min_q`` calls N."""
    out, p, i, L = {}, int(rec["pos"]), 0, len(rec["seq"])
    for n, op in CIGAR_OP.findall(rec["cigar"] or ""):
        if i >= L:
            break
        n = int(n)
        if op in "M=X":
            for t in range(n):
                if i + t < L:
                    base = rec["seq"][i + t]
                    out[p + t] = N if rec["qual"][i + t] < min_q else "ACGT".index(base) if base in "ACGT" else N
            p += n
            i += n
        elif op == "D":
            for t in range(n):
                out[p + t] = DEL
            p += n
        elif op in "IS":
            i += n
        elif op == "N":
            p += n
    return out


def molecule(c0, c1):
    """The family's call from its records' calls (None: no call)."""
    if c1 is None or c0 == c1:
        return c0
    if c0 is None or c0 == N:
        return c1
    if c1 == N:
        return c0
    return DISCORDANT


def table(sites, ds_records, min_q=0):
    """``sites``: [(tid, pos)] with pos 0-based, in the output's order;
    ``ds_records``: the written duplex records, two per family in order."""
    assert len(ds_records) % 2 == 0
    index = {s: i for i, s in enumerate(sites)}
    assert len(index) == len(sites)
    out = [[0] * COLS for _ in sites]
    for f in range(len(ds_records) // 2):
        r0, r1 = ds_records[2 * f], ds_records[2 * f + 1]
        assert r0["tid"] == r1["tid"]
        m0, m1 = calls(r0, min_q), calls(r1, min_q)
        for p in m0.keys() | m1.keys():
            i = index.get((r0["tid"], p))
            if i is None:
                continue
            c0, c1 = m0.get(p), m1.get(p)
            out[i][molecule(c0, c1)] += 1
            out[i][BOTH] += c0 is not None and c1 is not None
    return out


def covering(sites, ds_records):
    """Per site, the written families with a call there, by brute force over
    the CIGARs alone (no base is looked at): the identity the seven call
    columns must sum to."""
    out = [0] * len(sites)
    index = {s: i for i, s in enumerate(sites)}
    for f in range(len(ds_records) // 2):
        pair = ds_records[2 * f:2 * f + 2]
        spans = []
        for r in pair:
            p, i, L = int(r["pos"]), 0, len(r["seq"])
            for n, op in CIGAR_OP.findall(r["cigar"] or ""):
                if i >= L:
                    break
                n = int(n)
                if op in "M=X":
                    spans.append((p, p + min(n, L - i)))
                    p, i = p + n, i + n
                elif op == "D":
                    spans.append((p, p + n))
                    p += n
                elif op in "IS":
                    i += n
                elif op == "N":
                    p += n
        for p in {p for a, b in spans for p in range(a, b)}:
            k = index.get((pair[0]["tid"], p))
            if k is not None:
                out[k] += 1
    return out


def tsv(sites, rows, references):
    """The ``--allele_counts_output`` file of a table."""
    return HEADER + "".join("%s\t%d\t%s\t%d\n" % (references[tid], pos + 1, "\t".join(str(v) for v in row),
                                                  sum(row[:7]))
                            for (tid, pos), row in zip(sites, rows))


def summary_line(rows):
    """What the CLI prints after the other summary lines."""
    depth = [sum(r[:7]) for r in rows]
    return ("\n Allele counts at %d sites: %d sites covered, %d molecules counted, %d of them discordant.\n"
            % (len(rows), sum(d > 0 for d in depth), sum(depth), sum(r[DISCORDANT] for r in rows)))
