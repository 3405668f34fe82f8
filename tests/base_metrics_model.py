"""The per-base duplex QC tables (include/dcr.h ``dcr_base_metrics``,
``--base_metrics_output``) restated in plain Python over the per-base filters'
map (tests/base_filter_model.py ``base_map``) and the oracle's cores.

    words = tables(families)           # uint64[BMET_WORDS]; families: base_filter_model.family results
    add_record(m, a, b, r, j)          # duplex core r = record j of its family, called from cores a and b
    view = sparse(words)               # the non-zero entries by name, for literal expectations

Every table is an integer sum, so the words of a run are the sum of the
words of its families in any order.
"""
import numpy as np

from duplexumiconsensusreads_amd import params as P
from tests import base_filter_model as bm

CODE = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "T": 3, "t": 3}
DEPTH_MAX, CYC_MAX, ERR_OTHER = 63, 511, 1001


def add_record(m, a, b, r, j):
    """Count duplex core ``r`` into the tables ``m`` (params.base_metrics_fields views)."""
    n, L = m["n"], len(r["seq"])
    n[0] += 1
    for i, (c, ia, ib, ca, cb) in enumerate(bm.base_map(a, b, r)):
        aD, aE = (a["d"][ca], a["e"][ca]) if ca is not None else (0, 0)
        bD, bE = (b["d"][cb], b["e"][cb]) if cb is not None else (0, 0)
        cE = r["e"][c]
        pa, pb = ia is not None, ib is not None
        cls = 2
        if pa and pb:
            x, y = CODE.get(a["seq"][ia], 4), CODE.get(b["seq"][ib], 4)
            m["pair"][j, x, y] += 1
            cls = 0 if x == y else 1
        s, e = aD + bD, aE + bE
        n[1] += 1
        n[2 if pa and pb else 3 if pa else 4 if pb else 5] += 1
        n[6] += cls == 1
        n[7] += cE > 0
        m["depth"][min(max(aD, bD), DEPTH_MAX), min(min(aD, bD), DEPTH_MAX)] += 1
        m["err"][(1000 * e) // s if s > 0 and e <= s else ERR_OTHER] += 1
        m["qual"][cls, r["qual"][i]] += 1
        cyc = m["cyc"][j, :, min(i if j == 0 else L - 1 - i, CYC_MAX)]
        cyc += np.array([1, r["seq"][i] == "N", cls == 1, cls == 2, s, e], np.uint64)


def add_family(m, res):
    for j in range(2):
        add_record(m, res["ss"][2 * j], res["ss"][2 * j + 1], res["ds"][j], j)


def tables(families):
    """The block of a run over ``families`` (None entries: failing families, not counted)."""
    words = np.zeros(P.BMET_WORDS, np.uint64)
    m = P.base_metrics_fields(words)
    for res in families:
        if res is not None:
            add_family(m, res)
    return words


def sparse(words):
    """The non-zero entries of a block: n as a list, the tables as dicts from index tuples to counts."""
    m = P.base_metrics_fields(words)
    out = {"n": [int(v) for v in m["n"]]}
    for k in ("pair", "depth", "err", "qual", "cyc"):
        out[k] = {tuple(int(x) for x in idx): int(m[k][tuple(idx)]) for idx in np.argwhere(m[k])}
    return out


def masked_by_min_reads(words, t, hi_min, lo_min):
    """The bases ``--filter_min_base_reads t,hi_min,lo_min`` masks, read off ``depth`` (exact below the clamp)."""
    d = P.base_metrics_fields(words)["depth"]
    return sum(int(d[h, lo]) for h in range(DEPTH_MAX + 1) for lo in range(DEPTH_MAX + 1)
               if not (h + lo >= t and h >= hi_min and lo >= lo_min))
