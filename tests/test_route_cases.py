"""The routing-edge case table (tests/route_cases.py) on the CPU: every case's
declared geometry recomputed from the packed batch alone, both sides of every
limit present, and the two oracles (C and the Python restatement) agreeing on
every field at these shapes.  Nothing here says which kernel a record takes."""
from fractions import Fraction

import numpy as np
import pytest

from duplexumiconsensusreads_amd.batch import _end_soft_clips
from oracle import dcr_oracle as po
from oracle import dcr_oracle_c
from tests import route_cases as rc

CASES = rc.cases()
IDS = [c.name for c in CASES]
KIND = {"IndexError": rc.ST_INDEX, "TypeError": rc.ST_TYPE, "ValueError": rc.ST_VALUE,
        "OverflowError": rc.ST_OVERFLOW, "exit": rc.ST_EXIT}


# ---------------------------------------------------------------- geometry
def measure(p, f):
    """The quantities of family f's A1 (and its duplex) from the batch's arrays."""
    so = p.sub_off.astype(np.int64)
    a, b = int(so[4 * f]), int(so[4 * f + 1])
    kept = p.seq_len.astype(np.int64) - _end_soft_clips(p.cigar, p.cig_off, p.cig_n)
    pos = p.read_pos.astype(np.int64)
    m = dict(R=b - a)
    if b == a:
        return m
    m["T"] = int((pos[a:b] + kept[a:b]).max() - pos[a:b].min())
    b2 = int(so[4 * f + 2])
    if b2 > b:
        m["duplex_T"] = int((pos[a:b2] + kept[a:b2]).max() - pos[a:b2].min())
    dp = pos[a:b] - pos[a]
    m["dpos"] = int(dp[np.argmax(np.abs(dp))])
    lo, hi = int(p.seq_off[a:b].min()), int((p.seq_off[a:b] + kept[a:b]).max())
    m["lo15"] = lo & 15
    m["span"] = hi - (lo & ~15)
    m["ncig_max"] = int(p.cig_n[a:b].max())
    m["span4"] = hi - (lo & ~3)                       # the general kernel stages from a dword boundary
    runs, i_runs, failing, len0 = [], [], [], []
    m["single_m"], m["leading_ins"] = True, False
    for g in range(a, b):
        cig = p.cigar[int(p.cig_off[g]):int(p.cig_off[g]) + int(p.cig_n[g])]
        ops, lens = (cig & 15).tolist(), (cig >> 4).tolist()
        if len(ops) != 1:
            runs.append((g - a, len(ops)))
        if ops != [0]:
            m["single_m"] = False
        if 1 in ops:
            i_runs.append((g - a, [n for o, n in zip(ops, lens) if o == 1]))
            m["leading_ins"] |= ops[0] == 1
        bases = p.bases[int(p.seq_off[g]):int(p.seq_off[g]) + int(p.seq_len[g])]
        quals = p.quals[int(p.seq_off[g]):int(p.seq_off[g]) + int(p.seq_len[g])]
        if ops == [4] or (bases == ord("N")).all():
            # no base is kept and no CIGAR op is left: the 3' trim raises (:740), an S run reads back None (:279)
            failing.append(g - a)
        elif (quals < rc.PARAMS.min_base_quality).all() and sum(lens) > len(bases):
            # every base masked and trimmed, one op (of a deleted position) left: status 0, len 0
            len0.append(g - a)
    m["runs"], m["i_runs"] = runs, i_runs
    m["i_run_max"] = max((n for _, ns in i_runs for n in ns), default=0)
    m["i_runs_per_read"] = max((len(ns) for _, ns in i_runs), default=0)
    m["n_failing"], m["n_len0"] = len(failing), len(len0)
    if len(failing) == 1:
        m["failing_read"] = failing[0]
    if len(len0) == 1:
        m["len0_read"] = len0[0]
    # columns of a record whose reads are whole M runs at one position: d, e and the tie of the mean
    if not runs and (dp == 0).all() and (p.seq_len[a:b] == p.seq_len[a]).all():
        L = int(p.seq_len[a])
        rows = np.stack([p.bases[int(p.seq_off[g]):int(p.seq_off[g]) + L] for g in range(a, b)])
        quals = np.stack([p.quals[int(p.seq_off[g]):int(p.seq_off[g]) + L] for g in range(a, b)])
        if (quals == 37).all() and not (rows == ord("N")).any():
            e_over_d = []
            for t in range(L):
                vals, cnt = np.unique(rows[:, t], return_counts=True)
                if len(vals) > 1:
                    e_over_d.append((int(b - a - cnt.max()), b - a))
            x = sum((Fraction(e, d) for e, d in e_over_d), Fraction(0)) * 2000 / L
            m["e_over_d"] = e_over_d
            m["tie"] = x.denominator == 1 and x.numerator % 2 == 1
    return m


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_declared_geometry_alone(case):
    p, where = rc.build_batch([case])
    got = measure(p, where[case.name])
    for k, v in case.declares.items():
        assert k in got, f"{case.name}: no measurement of {k}"
        assert got[k] == v, (case.name, k, got[k], v)


@pytest.mark.parametrize("seed", [1, 2])
def test_declared_geometry_in_the_combined_batches(seed):
    """The same in the two shuffles the GPU tests run: lo & 15 and the span
    depend on the family's place in the batch."""
    sel = rc.shuffled(seed)
    p, where = rc.build_batch(sel)
    assert 90 <= p.n_fam <= 130 and p.n_reads < 60_000
    for case in sel:
        got = measure(p, where[case.name])
        for k, v in case.declares.items():
            assert got[k] == v, (case.name, k, got[k], v)


def _straddles(p, rpw, unit):
    """records whose reads cross a multiple of ``unit`` reads counted from
    their wave's first read (k_recmeta walks [sub_off[rb], sub_off[rend]))"""
    so = p.sub_off.astype(np.int64)
    n_rec, n = len(so) - 1, 0
    for r in range(n_rec):
        g = so[(r // rpw) * rpw]
        if so[r + 1] > so[r] and (so[r] - g) // unit != (so[r + 1] - 1 - g) // unit:
            n += 1
    return n


@pytest.mark.parametrize("name", sorted(rc.RPW_BATCHES))
def test_work_split_batches(name):
    spec = rc.RPW_BATCHES[name]
    p = rc.rpw_batch(name)
    n_rec = 4 * p.n_fam
    assert p.n_fam == spec["n_fam"] and p.n_reads // n_rec == spec["mean"]
    assert rc.recmeta_rpw(p.n_reads, n_rec) == (spec["rpw"], spec["waves"])
    if spec["rpw"] > 1:     # at rpw 1 a block holds 4 records and n_rec is a multiple of 4 (route_cases.UNPINNED)
        assert n_rec % (spec["rpw"] * spec["waves"]) != 0
    assert _straddles(p, spec["rpw"], 64) > 0
    assert _straddles(p, spec["rpw"], 6 * 64) > 0          # kBatch * kWave reads in flight together


# ---------------------------------------------------------------- coverage
def strand_outcomes(p, f):
    """What the duplex pass of family f's first pair is handed, from the C
    oracle's single-strand records: does a strand fail, and does a strand come
    with status 0 and no base."""
    ss, _, _ = dcr_oracle_c.run(p, rc.PARAMS_MIN0)
    st, ln = ss.status[4 * f:4 * f + 2], ss.len[4 * f:4 * f + 2]
    return dict(strand_fails=bool((st != 0).any()), strand_len0=bool(((st == 0) & (ln == 0)).any()))


def limit_values(key):
    _, _, qty, on, past = rc.LIMITS[key]
    if key == "r_safe":                       # from params.py's tables, never a literal
        on = rc.r_safe(rc.PARAMS)
        past = on + 1
    return qty, on, past


def coverage(cases=CASES):
    """limit -> {"on": [case names], "past": [...]}: the side comes from the
    measured quantity (the batch's arrays, or the oracle's single-strand
    records for the two duplex outcomes), never from a label."""
    seen = {k: {"on": [], "past": []} for k in rc.LIMITS}
    for c in cases:
        p, where = rc.build_batch([c])
        got = measure(p, where[c.name])
        if {"duplex_upstream", "duplex_len0"} & set(c.pins):
            got.update(strand_outcomes(p, where[c.name]))
        for k in c.pins:
            qty, on, past = limit_values(k)
            v = got.get(qty)
            for side, want in (("on", on), ("past", past)):
                if v is not None and type(v) is type(want) and v == want:
                    seen[k][side].append(c.name)
    qty, on, past = limit_values("recmeta_rpw")
    for name in rc.RPW_BATCHES:
        p = rc.rpw_batch(name)
        rpw = rc.recmeta_rpw(p.n_reads, 4 * p.n_fam)[0]
        for side, want in (("on", on), ("past", past)):
            if rpw == want:
                seen["recmeta_rpw"][side].append(name)
    return seen


def test_every_limit_has_a_case_on_it_and_one_past_it():
    seen = coverage()
    missing = {k: [s for s in ("on", "past") if not v[s]] for k, v in seen.items() if not (v["on"] and v["past"])}
    assert not missing, missing
    for k, (what, where, qty, on, past) in rc.LIMITS.items():
        assert what and ".hip:" in where and on != past, k
    named = {k for c in CASES for k in c.pins} | {"recmeta_rpw"}
    assert named == set(rc.LIMITS)


@pytest.mark.parametrize("drop,limit,side", [("t_240", "fast_max_t", "on"), ("t_241", "fast_max_t", "past"),
                                             ("deep_r_992", "deep_widen_2", "on"), ("pw_128", "pairwise_128", "on"),
                                             ("duplex_empty_a1_1m1d1m", None, None)])
def test_coverage_notices_a_missing_case(drop, limit, side):
    """without the case on a limit (a neighbour below it left in place) or the
    one past it, the limit lacks that side; a case with a twin leaves none"""
    only = [c for c in CASES if limit in c.pins or (limit is None and "duplex_len0" in c.pins)]
    seen = coverage([c for c in only if c.name != drop])
    if limit is None:
        assert seen["duplex_len0"]["on"] and seen["duplex_len0"]["past"]
    else:
        assert not seen[limit][side] and seen[limit]["past" if side == "on" else "on"]


def test_the_r_safe_pair_follows_the_tables():
    by = {c.name: c for c in CASES}
    assert by["r_safe_plus_1"].declares["R"] == by["r_safe"].declares["R"] + 1 == rc.r_safe(rc.PARAMS) + 1
    assert by["r_safe_plus_1"].declares["R"] <= 63, "above kFastMaxR the pair would not reach the fast kernel"


# ------------------------------------------------- the reference at these shapes
def py_params(params):
    return po.Params(seqQ_threshold=params.min_base_quality, min_reads=params.min_reads, max_reads=params.max_reads,
                     max_base_quality=params.max_base_quality, base_quality_shift=params.base_quality_shift,
                     post=params.error_rate_post_labeling, pre=params.error_rate_pre_labeling,
                     deletion_score=params.deletion_score, no_insertion_score=params.no_insertion_score)


def py_subfamily(p, s, P):
    """The Python restatement over subfamily s: a consensus dict, or the C status."""
    reads = []
    for g in range(int(p.sub_off[s]), int(p.sub_off[s + 1])):
        c0, b0 = int(p.cig_off[g]), int(p.seq_off[g])
        cig = [(int(c & 15), int(c >> 4)) for c in p.cigar[c0:c0 + int(p.cig_n[g])]]
        seq = p.bases[b0:b0 + int(p.seq_len[g])].tobytes().decode()
        qual = p.quals[b0:b0 + int(p.seq_len[g])].tolist()
        try:
            cg, sq, ql = po.preprocess_read(cig, seq, qual, P.seqQ_threshold)
        except po.RefCrash as e:
            return rc.ST_PREP | KIND[e.kind]
        reads.append(dict(pos=int(p.read_pos[g]), mapq=int(p.read_mapq[g]), cigar=cg, seq=sq, qual=ql))
    return py_core(reads, P)


def py_core(reads, P):
    try:
        return po.consensus_core(reads, P)
    except po.RefCrash as e:
        return KIND[e.kind]
    except ValueError:                       # min([]) of an empty subfamily (:458)
        return rc.ST_VALUE


FIELDS = ("pos", "mapq", "cigar", "seq", "qual", "d", "e", "D", "M", "E")


def assert_oracles_agree(p, params, label):
    ss, ds, _ = dcr_oracle_c.run(p, params)
    P = py_params(params)
    py_ss = [py_subfamily(p, s, P) for s in range(4 * p.n_fam)]
    py_ds = []
    for f in range(p.n_fam):
        for x, y in ((4 * f, 4 * f + 1), (4 * f + 2, 4 * f + 3)):
            a, b = py_ss[x], py_ss[y]
            py_ds.append(rc.ST_UPSTREAM if isinstance(a, int) or isinstance(b, int) else py_core([a, b], P))
    for kind, out, col_off, py in (("ss", ss, p.ss_col_off, py_ss), ("ds", ds, p.ds_col_off, py_ds)):
        for i, want in enumerate(py):
            if isinstance(want, int):
                assert int(out.status[i]) == want, (label, kind, i, int(out.status[i]), want)
                continue
            got = out.record(i, col_off)
            assert got["status"] == 0, (label, kind, i, got["status"])
            for k in FIELDS:
                w = [tuple(x) for x in want[k]] if k == "cigar" else want[k]
                assert got[k] == w, (label, kind, i, k)
    return ss, ds


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_both_oracles_agree(case):
    p, where = rc.build_batch([case])
    ss, ds = assert_oracles_agree(p, rc.PARAMS_MIN0 if case.min0 else rc.PARAMS, case.name)
    f = where[case.name]
    st = [int(x) for x in ss.status[4 * f:4 * f + 4]] + [int(x) for x in ds.status[2 * f:2 * f + 2]]
    if not case.fails:
        assert st == [0] * 6, (case.name, st)
    else:
        assert st[0] != 0 or st[1] != 0 or st[4] != 0, (case.name, st)
        assert st[2:4] == [0, 0] and st[5] == 0, (case.name, st)
        if "ss0" in case.expect:
            assert st[0] == case.expect["ss0"], (case.name, st)
        if "ds0" in case.expect:
            assert st[4] == case.expect["ds0"], (case.name, st)


def test_edge_outcomes_the_notes_claim():
    """what keeps two groups of cases on their edge, from the C oracle: the
    underflow column's call is 'A' (every class product is 0: a NaN posterior,
    :603-618), and E of the tie cases is the exact mean rounded half to even
    (the double product lands on the half) while the off-tie case is exact"""
    by = {c.name: c for c in CASES}
    for name in ("underflow_64", "underflow_65"):
        p, where = rc.build_batch([by[name]])
        ss, _, _ = dcr_oracle_c.run(p, rc.PARAMS)
        assert ss.record(4 * where[name], p.ss_col_off)["seq"][10] == "A", name
    want = {"tie_d4_1col_t100": 0.002, "tie_d4_2col_t200": 0.002, "tie_d8_1col_t50": 0.002, "tie_d10_1col_t200": 0.0,
            "tie_off_d4_2col_t100": 0.005}
    assert set(want) == {c.name for c in CASES if "e_tie" in c.pins}
    for name, e in want.items():
        c = by[name]
        p, where = rc.build_batch([c])
        mean = sum(Fraction(x, d) for x, d in c.declares["e_over_d"]) / c.declares["T"] * 1000
        lo = mean.numerator // mean.denominator
        half_even = lo + (1 if mean - lo > Fraction(1, 2) or (mean - lo == Fraction(1, 2) and lo % 2) else 0)
        assert Fraction(half_even, 1000) == Fraction(str(e)), name
        ss, _, _ = dcr_oracle_c.run(p, rc.PARAMS)
        assert float(ss.E[4 * where[name]]) == e, (name, float(ss.E[4 * where[name]]))


@pytest.mark.parametrize("name", sorted(rc.RPW_BATCHES))
def test_both_oracles_agree_on_work_split_batches(name):
    p = rc.rpw_batch(name)
    ss, ds = assert_oracles_agree(p, rc.PARAMS, name)
    assert not ss.status.any() and not ds.status.any()


def test_slot_groups_by_deepest_subfamily():
    """the three inputs of the slot path's hint: deepest subfamily exactly 63, exactly 64, 65 or more"""
    groups = rc.slot_groups()
    assert max(c.max_r for c in groups["r63"]) == 63 and max(c.max_r for c in groups["r64"]) == 64
    assert min(max(c.max_r for c in groups["r65"]), 65) == 65
    assert not any(c.fails for c in groups["r63"] + groups["r64"]) and any(c.fails for c in groups["r65"])
    placed = {c.name for g in groups.values() for c in g}
    assert placed == {c.name for c in CASES if c.ingest}
    assert [c.name for c in CASES if not c.ingest] == ["r_0"]
