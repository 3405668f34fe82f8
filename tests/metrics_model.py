"""The consensus QC tables (include/dcr.h ``dcr_metrics``, ``--metrics_output``)
restated in plain Python over decoded BAM records, the dict form
``tests.test_ss_output.records`` returns.

Everything comes from the records' own fields and tags: the sub-family size
is ``len(sQ)``, the per-column lists are ``sd`` / ``se`` and ``cd`` / ``ce``,
the strand depths ``aD bD``, the error rates ``aE bE cE`` through
``round(float(tag), 3)`` (the tag is a float32 of a double already rounded to
three decimals, as tests/filter_model.py reads them), and the orientation is
flag bit 0x10.  Single-strand records come four per family (A1 B2 B1 A2),
duplex records two per family.

    doc = document(tables(ds_records, ss_records))      # what the JSON file holds
"""
import json

READS_MAX, DEPTH_MAX, COL_MAX, ERR_OTHER = 255, 63, 511, 1001
SS_NAMES = ("A1", "B2", "B1", "A2")


def tag(rec, name):
    for t in rec["tags"]:
        if t[0] == name:
            return t[2]
    raise KeyError(name)


def int_list(v):
    return [int(x) for x in (json.loads(v) if isinstance(v, str) else v)]


def err_bin(tag_value):
    E = round(float(tag_value), 3)
    return int(round(E * 1000.0)) if 0.0 <= E <= 1.0 else ERR_OTHER        # round(): half to even, as rint


def empty():
    return {"n": [0] * 8, "ss_reads": [[0] * 256 for _ in range(4)], "ds_depth": [[0] * 64 for _ in range(64)],
            "err_c": [0] * 1002, "err_s": [0] * 1002, "ss_qual": [0] * 256, "ds_qual": [0] * 256,
            "col": [[[0] * 512 for _ in range(3)] for _ in range(2)]}


def _columns(t, kind, rec, d_name, e_name):
    d, e = int_list(tag(rec, d_name)), int_list(tag(rec, e_name))
    assert len(d) == len(e)
    n = len(d)
    for c in range(n):
        cp = n - 1 - c if rec["flag"] & 0x10 else c          # counted from the read's sequencing 5' end
        b = min(cp, COL_MAX)
        t["col"][kind][0][b] += 1
        t["col"][kind][1][b] += d[c]
        t["col"][kind][2][b] += e[c]
    return n


def tables(ds_records, ss_records):
    """The tables of whole families: two duplex and four single-strand records each, in order."""
    assert len(ds_records) % 2 == 0 and len(ss_records) == 2 * len(ds_records)
    t = empty()
    t["n"][0] = len(ds_records) // 2
    for i, r in enumerate(ss_records):
        t["n"][1] += len(r["seq"])
        t["ss_reads"][i % 4][min(len(int_list(tag(r, "sQ"))), READS_MAX)] += 1
        for q in r["qual"]:
            t["ss_qual"][q] += 1
        t["n"][4] += _columns(t, 0, r, "sd", "se")
    for r in ds_records:
        t["n"][2] += len(r["seq"])
        t["n"][3] += r["seq"].count("N")
        aD, bD = max(int(tag(r, "aD")), 0), max(int(tag(r, "bD")), 0)
        t["ds_depth"][min(max(aD, bD), DEPTH_MAX)][min(min(aD, bD), DEPTH_MAX)] += 1
        t["err_c"][err_bin(tag(r, "cE"))] += 1
        t["err_s"][max(err_bin(tag(r, "aE")), err_bin(tag(r, "bE")))] += 1
        for q in r["qual"]:
            t["ds_qual"][q] += 1
        t["n"][5] += _columns(t, 1, r, "cd", "ce")
    return t


def flat(t):
    """The tables as the 10,716 words of ``dcr_metrics``, in the struct's order."""
    out = list(t["n"])
    for row in t["ss_reads"]:
        out += row
    for row in t["ds_depth"]:
        out += row
    out += t["err_c"] + t["err_s"] + t["ss_qual"] + t["ds_qual"]
    for kind in t["col"]:
        for row in kind:
            out += row
    assert len(out) == 10716
    return out


def _trim(a):
    while a and a[-1] == 0:
        a = a[:-1]
    return list(a)


def document(t):
    """The ``--metrics_output`` JSON document (version 1) of the tables."""
    doc = {"version": 1, "bins": {"ss_reads_max": READS_MAX, "ds_depth_max": DEPTH_MAX, "column_max": COL_MAX,
                                  "error_rate_other": ERR_OTHER}}
    for i, name in enumerate(("families", "ss_bases", "ds_bases", "ds_no_calls", "ss_columns", "ds_columns")):
        doc[name] = t["n"][i]
    doc["ss_reads"] = {k: _trim(t["ss_reads"][i]) for i, k in enumerate(SS_NAMES)}
    doc["ss_qual"], doc["ds_qual"] = _trim(t["ss_qual"]), _trim(t["ds_qual"])
    doc["ds_depth"] = [[h, lo, t["ds_depth"][h][lo]] for h in range(64) for lo in range(64) if t["ds_depth"][h][lo]]
    for k in ("err_c", "err_s"):
        doc[k] = [[b, v] for b, v in enumerate(t[k]) if v]
    doc["col"] = {}
    for i, kind in enumerate(("ss", "ds")):
        rec = _trim(t["col"][i][0])
        doc["col"][kind] = {"records": rec, "depth": t["col"][i][1][:len(rec)], "errors": t["col"][i][2][:len(rec)]}
    return doc


def file_bytes(doc):
    """Sorted keys, fixed separators, one trailing newline."""
    return (json.dumps(doc, sort_keys=True, separators=(",", ":")) + "\n").encode()
