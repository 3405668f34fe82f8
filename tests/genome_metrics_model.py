"""The errors against a genome (include/dcr.h ``dcr_genome_metrics``,
``--genome`` / ``--genome_metrics_output``) restated in plain Python.

A genome is a list of strings, one per sequence of the input header ("" for
a sequence the FASTA lacks); a base of it is A C G T in either case (codes
0..3) or anything else (4).  Records are taken either as the dicts
``tests.test_ss_output.records`` returns (``tables``: four single-strand
records and two duplex records per family, in order) or as raw result arrays
(``tables_of_arrays``: len and n_cig clamped to the record's region here).

The tables are numpy arrays shaped as the struct's fields, uint64:
n[2][12], sub[2][2][4][4], tri[2][2][4][4][4][4], cyc[2][2][2][512],
qual[2][2][256]; ``words`` lays them out as the block.
"""
import collections
import re

import numpy as np

CIGAR_OP = re.compile(r"(\d+)([MIDNSHP=X])")
OPS = "MIDNSHP=X"
LEVELS = ("single_strand", "duplex")
N_NAMES = ("records", "aligned_bases", "matches", "mismatches", "no_calls", "genome_unknown", "insertions",
           "inserted_bases", "deletions", "deleted_positions")


def new_tables():
    return dict(n=np.zeros((2, 12), np.uint64), sub=np.zeros((2, 2, 4, 4), np.uint64),
                tri=np.zeros((2, 2, 4, 4, 4, 4), np.uint64), cyc=np.zeros((2, 2, 2, 512), np.uint64),
                qual=np.zeros((2, 2, 256), np.uint64))


def words(t):
    return np.concatenate([t[k].reshape(-1) for k in ("n", "sub", "tri", "cyc", "qual")])


def base_code(c):
    """A a 0, C c 1, G g 2, T t 3, anything else 4."""
    return "ACGT".find(c.upper()) if len(c) == 1 and c.upper() in "ACGT" else 4


def code(genome, tid, p):
    """The genome's code at position p of sequence tid; 4 outside either."""
    if not 0 <= tid < len(genome) or not 0 <= p < len(genome[tid]):
        return 4
    return base_code(genome[tid][p])


def count_record(t, lv, j, tid, pos, ops, seq, qual, genome):
    """One record: ``ops`` [(operation letter, n)], ``seq`` a string and
    ``qual`` a list of the same (clamped) length."""
    c = collections.Counter()           # (table, index ...) -> count; added to the arrays at the end
    L = len(seq)
    c["n", lv, 0] += 1
    p, i = pos, 0
    for op, cnt in ops:
        if i >= L:
            break                       # an operation past the last base counts nothing
        here = min(cnt, L - i)
        if op in "M=X":
            for k in range(here):
                g, x = code(genome, tid, p + k), base_code(seq[i + k])
                c["n", lv, 1] += 1
                if g == 4:
                    c["n", lv, 5] += 1
                elif x == 4:
                    c["n", lv, 4] += 1
                else:
                    mis = int(g != x)
                    c["n", lv, 2 + mis] += 1
                    c["sub", lv, j, g, x] += 1
                    g5, g3 = code(genome, tid, p + k - 1), code(genome, tid, p + k + 1)
                    if g5 < 4 and g3 < 4:
                        c["tri", lv, j, g5, g, g3, x] += 1
                    cyc = i + k if j == 0 else L - 1 - (i + k)
                    for what in range(1 + mis):
                        c["cyc", lv, j, what, min(cyc, 511)] += 1
                        c["qual", lv, what, qual[i + k]] += 1
            p += cnt
            i += cnt
        elif op == "I":
            c["n", lv, 6] += 1
            c["n", lv, 7] += here
            i += cnt
        elif op == "S":
            i += cnt
        elif op == "D":
            c["n", lv, 8] += 1
            c["n", lv, 9] += cnt
            p += cnt
        elif op == "N":
            p += cnt
    for (name, *idx), v in c.items():
        t[name][tuple(idx)] += np.uint64(v)
    return t


def tables(ss_records, ds_records, genome, t=None):
    """Over decoded records: four single-strand and two duplex ones per family, in order."""
    t = new_tables() if t is None else t
    assert len(ss_records) == 2 * len(ds_records) and len(ds_records) % 2 == 0
    for lv, recs, per in ((0, ss_records, 4), (1, ds_records, 2)):
        for k, r in enumerate(recs):
            j = (k % per) >> (1 if lv == 0 else 0)
            ops = [(op, int(cnt)) for cnt, op in CIGAR_OP.findall(r["cigar"] or "")]
            count_record(t, lv, j, r["tid"], int(r["pos"]), ops, r["seq"], list(r["qual"]), genome)
    return t


def tables_of_arrays(ss, ds, ss_col_off, ds_col_off, fam_tid, n_fam, genome, fam_fail=None, t=None):
    """Over raw result arrays (attributes pos, len, n_cig, cigar, seq, qual):
    len and n_cig are clamped to the record's region, families with
    fam_fail[f] != 0 are skipped."""
    t = new_tables() if t is None else t
    for f in range(n_fam):
        if fam_fail is not None and fam_fail[f] != 0:
            continue
        for lv, o, off, per in ((0, ss, ss_col_off, 4), (1, ds, ds_col_off, 2)):
            for k in range(per):
                r = per * f + k
                ro, room = int(off[r]), int(off[r + 1]) - int(off[r])
                L, nc = min(max(int(o.len[r]), 0), room), min(max(int(o.n_cig[r]), 0), room)
                ops = [(OPS[int(v) & 15] if int(v) & 15 < len(OPS) else "?", int(v) >> 4) for v in o.cigar[ro:ro + nc]]
                seq = o.seq[ro:ro + L].tobytes().decode("latin-1")
                count_record(t, lv, k >> 1 if lv == 0 else k, int(fam_tid[f]), int(o.pos[r]), ops, seq,
                             o.qual[ro:ro + L].tolist(), genome)
    return t


def totals(t):
    """Per level (aligned bases, mismatches, mismatches per million compared bases)."""
    out = []
    for lv in range(2):
        cmp_, mis = int(t["n"][lv, 2]) + int(t["n"][lv, 3]), int(t["n"][lv, 3])
        out.append((int(t["n"][lv, 1]), mis, mis * 1000000 // cmp_ if cmp_ else 0))
    return out


def summary_line(t):
    """What the CLI prints after the other summary lines."""
    (a0, m0, r0), (a1, m1, r1) = totals(t)
    return ("\n Against the genome: single-strand consensus %d aligned bases, %d mismatches, %d per million; "
            "duplex consensus %d aligned bases, %d mismatches, %d per million.\n" % (a0, m0, r0, a1, m1, r1))


def document(t):
    """The ``--genome_metrics_output`` file as the object its JSON decodes to."""
    doc = {"version": 1, "bins": {"cycle_max": 511}, "codes": "ACGT"}
    for lv, level in enumerate(LEVELS):
        d = {name: int(t["n"][lv, i]) for i, name in enumerate(N_NAMES)}
        d["sub"], d["tri"], d["cycle"] = {}, {}, {}
        for j, read in enumerate(("read1", "read2")):
            d["sub"][read] = t["sub"][lv, j].tolist()
            d["tri"][read] = [[a, b, c, x, int(t["tri"][lv, j, a, b, c, x])]
                              for a in range(4) for b in range(4) for c in range(4) for x in range(4)
                              if t["tri"][lv, j, a, b, c, x]]
            last = max([i for i in range(512) if t["cyc"][lv, j, 0, i]], default=-1)
            d["cycle"][read] = {"compared": t["cyc"][lv, j, 0, :last + 1].tolist(),
                                "mismatches": t["cyc"][lv, j, 1, :last + 1].tolist()}
        last = max([i for i in range(256) if t["qual"][lv, 0, i]], default=-1)
        d["qual"] = {"compared": t["qual"][lv, 0, :last + 1].tolist(),
                     "mismatches": t["qual"][lv, 1, :last + 1].tolist()}
        doc[level] = d
    return doc
