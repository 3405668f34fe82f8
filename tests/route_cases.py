"""Hand-made families on both sides of every integer limit that decides which
consensus kernel a record takes (no GPU, no pytest).

A record passes k_recmeta (classification), then the fast kernel (common or
EXACT instantiation) or the general list (k_decide / k_decide_deep,
k_ins_layout, k_consensus_general); the choice depends on limits that follow
from packed bit fields.  ``LIMITS`` names each one with the place it was read
from, the quantity it is about and that quantity's values on the limit and one
step past it; every case names the limits it is for and the quantities it
declares.  tests/test_route_cases.py recomputes those quantities from the
packed batch alone and checks, from what it measured, that every limit has a
case on it and a case one step past it; tests/test_gpu_route_edges.py runs the cases through the
three entry points against the C oracle.  No route is asserted anywhere: the
table proves where the inputs are, the GPU tests that the outputs are right.

Subfamily 0 (A1) of a case's family carries the shape; the duplex cases use
A1 and B2.  The other subfamilies are two plain 150M reads.  Reads share one
template with about 1 % substitutions and qualities drawn from
{37, 37, 37, 25, 12} (12 is below the default mask threshold, so d and e vary
by column); a read's first and last base keep quality 37 and the template's
letter, so that the 3' 'N' trim moves no end.  The generator is seeded by the
case's name.
"""
from __future__ import annotations

import math
import zlib
from fractions import Fraction
from types import SimpleNamespace as NS

import numpy as np

from duplexumiconsensusreads_amd.batch import pack_families
from duplexumiconsensusreads_amd.params import ConsensusParams, build_dcr_params

K = "duplexumiconsensusreads_amd/csrc/dcr_kernels.hip"
C = "duplexumiconsensusreads_amd/csrc/dcr_capi.hip"

# limit -> (the constant or condition, where it was read, the measured quantity
# it is about, that quantity's value ON the limit -- the last one for which the
# record stays on the path the limit guards -- and its value one step PAST it).
# tests/test_route_cases.py measures the quantity of every case that names the
# limit and wants one case at each of the two values; a boolean quantity is a
# predicate over the measured geometry.
LIMITS = {
    "recmeta_empty": ("R == 0", f"{K}:2397", "R", 1, 0),
    "recmeta_wave": ("R > kWave (64): k_prep_big preprocesses the reads", f"{K}:2398", "R", 64, 65),
    "recmeta_failing_read": ("g.flags & 1, fst = the first failing read and its status", f"{K}:2399", "n_failing", 0, 1),
    "recmeta_len0": ("g.flags & 2: a read of status 0 and len <= 0 (TYPE_ERROR)", f"{K}:2400", "n_len0", 0, 1),
    "recmeta_ncig": ("rd.ncig != 1 (flag 4)", f"{K}:2371", "single_m", True, False),
    "recmeta_dpos_hi": ("dpos > 32767 (16-bit dpos)", f"{K}:2372", "dpos", 32767, 32768),
    "recmeta_dpos_lo": ("dpos < -32768 (16-bit dpos)", f"{K}:2371", "dpos", -32768, -32769),
    "fast_max_r": ("R > kFastMaxR (63: 6-bit class counters, 7-bit R of RecMeta::w)", f"{K}:2411", "R", 63, 64),
    "fast_max_t": ("T > kFastMaxT (240: pairwise_small, 8-bit T of RecMeta::w)", f"{K}:2411", "T", 240, 241),
    "fast_stage": ("span > kStageElems (2048 staged bytes)", f"{K}:2411", "span", 2048, 2049),
    "common_stage": ("(span + 3) / 4 > Region<false>::kDw * kWave (1536 staged bytes)", f"{K}:3865", "span", 1536, 1537),
    "general_stage": ("span <= kStageElems in the general kernel's stage (from lo & ~3 there)", f"{K}:1289",
                      "span4", 2048, 2049),
    "deep_reads": ("R >= kDeepReads (64): k_decide_deep", f"{K}:4450", "R", 63, 64),
    "cols_lds": ("T <= kColsLds (256) / decide T > 256", f"{K}:1359", "T", 256, 257),
    "direct_r": ("R <= direct_r (3): exact queue unstaged", f"{K}:3864", "R", 3, 4),
    "narrow_rows": ("R > 15 (4-bit row counts of the narrow rows)", f"{K}:3865", "R", 15, 16),
    "m720": ("R > 16 (720720 = lcm(1..16) rational mean)", f"{K}:3559", "R", 16, 17),
    "r_safe": ("R > r_safe (fast_constants)", f"{K}:3239", "R", "r_safe", "r_safe + 1"),
    "e_tie": ("E = round(sum(e/d) / T, 3) on a half (k_fast_rows hands the record on)", f"{K}:3980", "tie", False, True),
    "pairwise_8": ("pairwise sum: n < 8 sequential", f"{K}:2009", "T", 7, 8),
    "pairwise_tail": ("pairwise sum: n % 8 tail after the eight accumulators", f"{K}:2023", "T", 8, 9),
    "pairwise_128": ("pairwise sum: n <= 128 one block, else two halves", f"{K}:1939", "T", 128, 129),
    "deep_nt1": ("deep T <= 64 (NT = 1)", f"{K}:4570", "T", 64, 65),
    "deep_nt2": ("deep T <= 128 (NT = 2)", f"{K}:4571", "T", 128, 129),
    "deep_nt3": ("deep T <= 192 (NT = 3)", f"{K}:4572", "T", 192, 193),
    "deep_t256": ("deep T <= 256 (NT = 4, refused above)", f"{K}:4565", "T", 256, 257),
    "deep_widen_1": ("packed sums widened every 62 rows, a wave takes R / 8 rows: one widening", f"{K}:1141", "R", 496, 497),
    "deep_widen_2": ("the same, two widenings", f"{K}:1141", "R", 992, 993),
    "deep_max_r": ("R <= 4095 (12-bit d / e of the column word)", f"{K}:4565", "R", 4095, 4096),
    "decide_underflow": ("Z - L_b <= 16 * 700 in the deep decision, records of 64 and 65 reads", f"{K}:1195", "R", 64, 65),
    "ins_run_len": ("L > 127 (7-bit insertion run length)", f"{K}:4218", "i_run_max", 127, 128),
    "ins_runs": ("rd.ncig > 4", f"{K}:4218", "ncig_max", 4, 5),
    "ins_two_runs": ("nIr > 1", f"{K}:4218", "i_runs_per_read", 1, 2),
    "ins_leading": ("need == 0: an insertion run before any M", f"{K}:4208", "leading_ins", False, True),
    "ins_chunk": ("k_ins_layout's 64-read chunks", f"{K}:4163", "R", 64, 65),
    "ins_max_r": ("R <= 4 * kWave (256)", f"{K}:4155", "R", 256, 257),
    "ins_max_t": ("T <= kColsLds (256) in k_ins_layout", f"{K}:4190", "T", 256, 257),
    "duplex_max_t": ("duplex T > kFastMaxT (240)", f"{K}:2411", "duplex_T", 240, 241),
    "duplex_cols_lds": ("duplex T > kColsLds (256)", f"{K}:1359", "duplex_T", 256, 257),
    "duplex_cigar": ("DUPLEX: a strand's cig0 is not one M run", f"{K}:2371", "single_m", True, False),
    "duplex_upstream": ("DUPLEX: g.flags & 1, a strand's record failed (UPSTREAM)", f"{K}:2399", "strand_fails", False, True),
    "duplex_len0": ("DUPLEX: g.flags & 2, a strand's consensus has status 0 and no base (TYPE_ERROR)", f"{K}:2400",
                    "strand_len0", False, True),
    "recmeta_rpw": ("rpw halved while rpw * (n_reads / n_rec) > 1024; 16- or 4-wave blocks", f"{C}:599-605", "rpw", 64, 32),
}

# limits known and left unpinned: (what, why)
UNPINNED = [
    ("base_al + span >= 0xFFFFF000 (dcr_kernels.hip:2412)", "needs a batch of 4 GB of bases"),
    ("k_recmeta at rpw = 1 with a record count that is no multiple of a block's records",
     "a block of rpw = 1 holds 4 records and n_rec = 4 * n_fam: every count is a multiple"),
]

ST_OK, ST_INDEX, ST_TYPE, ST_VALUE, ST_OVERFLOW, ST_EXIT, ST_UPSTREAM, ST_PREP = 0, 1, 2, 3, 4, 5, 6, 0x10
POS0 = 100_000
PARAMS = ConsensusParams(max_reads=10_000)
PARAMS_MIN0 = ConsensusParams(max_reads=10_000, min_reads=0)


def r_safe(params: ConsensusParams) -> int:
    """fast_constants' r_safe (dcr_capi.hip:472-477) over params.py's tables:
    the most reads R with R * c_max <= 700 nats."""
    p = build_dcr_params(params)
    qlo = 123
    while qlo > 0 and p.mismatch[qlo - 1] > 0.0 and p.match[qlo - 1] >= p.mismatch[qlo - 1]:
        qlo -= 1
    cmax = 0.0
    for q in range(123):
        cmax = max(cmax, -math.log(p.mismatch[q]))
        if q >= qlo:
            cmax = max(cmax, -math.log(p.match[q]))
    return int(min(1e6, math.floor(700.0 / cmax))) if cmax > 0.0 else 1000000


def recmeta_rpw(n_reads: int, n_rec: int):
    """launch_strand's records per wave and waves per block (dcr_capi.hip:599-605)."""
    rpw, avg = 64, n_reads // n_rec
    while rpw > 1 and rpw * avg > 1024:
        rpw >>= 1
    return rpw, (16 if rpw == 64 else 4)


class Case:
    """One family (``fam``: [A1, B2, B1, A2] lists of reads).  ``pins``:
    the limits the case is for (its side is measured, never declared).  ``declares``: the quantities the geometry test
    recomputes.  ``lo15``: where the family's first byte must fall modulo 16
    (a pad family in front of it sets that, ``build_batch``).  ``fails``: the
    case holds records that do not complete; ``expect``: the statuses of A1
    ("ss0") and of its duplex ("ds0") where they are known beforehand.  ``min0``: needs
    ConsensusParams(min_reads=0).  ``ingest``: may go through the BAM ingest
    (the empty subfamily cannot: a family with one is filtered there under the
    default min_reads; the failing reads pass the ingest unchanged)."""

    def __init__(self, name, fam, pins, declares, lo15=None, fails=False, min0=False, ingest=True, note="",
                 expect=None):
        self.name, self.fam, self.pins, self.declares = name, fam, pins, declares
        self.expect = expect or {}
        self.lo15, self.fails, self.min0, self.ingest, self.note = lo15, fails, min0, ingest, note
        for k in pins:
            assert k in LIMITS, k

    @property
    def max_r(self):
        return max(len(s) for s in self.fam)

    def __repr__(self):
        return f"Case({self.name})"


class Builder:
    def __init__(self, name, width=800, sub=0.01, quals=(37, 37, 37, 25, 12)):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.tmpl = self._rand(width)
        self.sub, self.quals = sub, quals

    def _rand(self, n):
        return "".join("ACGT"[i] for i in self.rng.integers(0, 4, n))

    def read(self, off, cig, sub=None, pos=None):
        """A read at template offset ``off`` with CIGAR ``cig`` [(op, n)]:
        M copies the template, I and S draw bases, D skips."""
        rng, sub = self.rng, self.sub if sub is None else sub
        out, ref = [], off
        for op, n in cig:
            if op == 0:
                seg = list(self.tmpl[ref:ref + n])
                assert len(seg) == n, "template too short"
                for i in np.nonzero(rng.random(n) < sub)[0]:
                    seg[i] = "ACGT"[("ACGT".index(seg[i]) + 1 + int(rng.integers(0, 3))) % 4]
                out.append("".join(seg))
                ref += n
            elif op in (1, 4):
                out.append(self._rand(n))
            elif op == 2:
                ref += n
        seq = "".join(out)
        q = [int(x) for x in rng.choice(self.quals, len(seq))]
        if seq and cig[-1][0] == 0:
            q[-1], seq = max(self.quals), seq[:-1] + self.tmpl[ref - 1]
        if seq and cig[0][0] == 0:
            q[0], seq = max(self.quals), self.tmpl[off] + seq[1:]
        return NS(reference_start=POS0 + off if pos is None else pos, mapping_quality=40, query_sequence=seq,
                  query_qualities=q, cigartuples=list(cig))

    def plain(self, n=2, L=150, off=0):
        return [self.read(off, [(0, L)]) for _ in range(n)]


def _fam(b, a1, b2=None):
    return [a1, b2 if b2 is not None else b.plain(), b.plain(), b.plain()]


def _plain_r(name, R, pins, L=150, **kw):
    b = Builder(name)
    return Case(name, _fam(b, b.plain(R, L)), pins, dict(R=R, T=L, ncig_max=1), **kw)


def _two_offsets(name, R, T, pins, L=150, sub=None, **kw):
    """R reads of L bases, alternately at offset 0 and T - L"""
    b = Builder(name) if sub is None else Builder(name, sub=sub)
    a1 = [b.read(0 if j % 2 == 0 else T - L, [(0, L)]) for j in range(R)]
    return Case(name, _fam(b, a1), pins, dict(R=R, T=T, ncig_max=1), **kw)


def _cases():
    out = []
    add = out.append
    # ---- k_recmeta classification
    b = Builder("r_0")
    add(Case("r_0", _fam(b, []), ["recmeta_empty", "duplex_upstream"], dict(R=0),
             fails=True, min0=True, ingest=False, note="ss VALUE_ERROR, its duplex UPSTREAM",
             expect=dict(ss0=ST_VALUE, ds0=ST_UPSTREAM)))
    add(_plain_r("r_1", 1, ["recmeta_empty", "duplex_upstream"]))
    for kind, cig_of, seq_of in (("alln", lambda L: [(0, L)], lambda s: "N" * len(s)),
                                 ("srun", lambda L: [(4, L)], lambda s: s)):
        for R, at, tag in ((3, 0, "first"), (3, 2, "last"), (65, 64, "r65_read64"), (65, 0, "r65_first")):
            name = f"fail_{kind}_{tag}"
            b = Builder(name)
            a1 = b.plain(R)
            a1[at].query_sequence = seq_of(a1[at].query_sequence)
            a1[at].cigartuples = cig_of(150)
            add(Case(name, _fam(b, a1), ["recmeta_failing_read"], dict(R=R, failing_read=at, n_failing=1),
                     fails=True, note="PREP | INDEX_ERROR" if kind == "alln" else "PREP | TYPE_ERROR",
                     expect=dict(ss0=ST_PREP | (ST_INDEX if kind == "alln" else ST_TYPE), ds0=ST_UPSTREAM)))
    # a read that preprocessing leaves with status 0 and no base: 75M1D75M with every quality below
    # the mask threshold (all 'N', trimmed from the 3' end; one CIGAR op is left, so nothing raises)
    for R, at, tag in ((3, 0, "first"), (3, 2, "last"), (64, 63, "r64_last"), (65, 64, "r65_read64"), (65, 0, "r65_first")):
        name = f"len0_{tag}"
        b = Builder(name)
        a1 = b.plain(R)
        a1[at] = b.read(0, [(0, 75), (2, 1), (0, 75)])
        a1[at].query_qualities = [12] * 150
        add(Case(name, _fam(b, a1), ["recmeta_len0"], dict(R=R, len0_read=at, n_len0=1, n_failing=0),
                 fails=True, note="the read has status 0 and len 0: the record is a TYPE_ERROR (list(None) at :402)",
                 expect=dict(ss0=ST_TYPE, ds0=ST_UPSTREAM)))
    add(_plain_r("r_3", 3, ["direct_r", "recmeta_failing_read", "recmeta_len0"]))
    add(_plain_r("r_4", 4, ["direct_r"]))
    add(_plain_r("r_15", 15, ["narrow_rows"]))
    add(_plain_r("r_16", 16, ["narrow_rows", "m720"]))
    add(_plain_r("r_17", 17, ["m720"]))
    rs = r_safe(PARAMS)
    add(_plain_r("r_safe", rs, ["r_safe"]))
    add(_plain_r("r_safe_plus_1", rs + 1, ["r_safe"]))
    add(_plain_r("r_63", 63, ["fast_max_r", "deep_reads"]))
    add(_plain_r("r_64", 64, ["fast_max_r", "deep_reads", "recmeta_wave"]))
    add(_plain_r("r_65", 65, ["recmeta_wave", "recmeta_failing_read", "recmeta_len0"]))
    for T, pins in ((239, ["fast_max_t"]), (240, ["fast_max_t"]), (241, ["fast_max_t"]),
                    (255, ["cols_lds"]), (256, ["cols_lds"]), (257, ["cols_lds"])):
        add(_two_offsets(f"t_{T}", 5, T, pins))
    for d, key, first in ((32767, "recmeta_dpos_hi", False), (32768, "recmeta_dpos_hi", False),
                          (-32768, "recmeta_dpos_lo", True), (-32769, "recmeta_dpos_lo", True)):
        name = f"dpos_{'m' if d < 0 else ''}{abs(d)}"
        b = Builder(name, width=34_000)
        near, far = b.read(0, [(0, 100)]), b.read(abs(d), [(0, 100)])
        add(Case(name, _fam(b, [far, near] if first else [near, far]), [key],
                 dict(R=2, T=abs(d) + 100, dpos=d, ncig_max=1)))
    # staged span: R reads of L bases from byte `lo15` of a 16-byte line
    for tag, R, L, key, edge in (("common", 8, 192, "common_stage", 1536), ("general", 8, 256, "general_stage", 2048),
                                 ("fast", 16, 128, "fast_stage", 2048)):
        for lo15 in (0, 1, 15):
            name = f"span_{tag}_{lo15}"
            c = _plain_r(name, R, [key], L=L, lo15=lo15)
            c.declares.update(span=edge + lo15, lo15=lo15)
            add(c)
    b = Builder("ncig_del")
    a1 = b.plain(5)
    a1[2] = b.read(0, [(0, 75), (2, 1), (0, 75)])
    add(Case("ncig_del", _fam(b, a1), ["recmeta_ncig"], dict(R=5, T=150, ncig_max=3, runs=[(2, 3)])))
    add(_plain_r("r_5", 5, ["recmeta_ncig", "duplex_cigar", "duplex_len0"]))
    # ---- rational ties of the mean: uniform quality 37, one read differs on `cols` columns
    for name, d, cols, T, tie in (("tie_d4_1col_t100", 4, 1, 100, True), ("tie_d4_2col_t200", 4, 2, 200, True),
                                  ("tie_d8_1col_t50", 8, 1, 50, True), ("tie_d10_1col_t200", 10, 1, 200, True),
                                  ("tie_off_d4_2col_t100", 4, 2, 100, False)):
        b = Builder(name, sub=0.0, quals=(37,))
        a1 = b.plain(d, T)
        s = list(a1[1].query_sequence)
        for k in range(cols):
            col = T // 3 + 7 * k
            s[col] = "ACGT"[("ACGT".index(s[col]) + 1) % 4]
        a1[1].query_sequence = "".join(s)
        x = Fraction(cols, d) * 2000 / T
        assert (x.denominator == 1 and x.numerator % 2 == 1) == tie
        add(Case(name, _fam(b, a1), ["e_tie"],
                 dict(R=d, T=T, ncig_max=1, tie=tie, e_over_d=[(1, d)] * cols),
                 note="sum(e/d) * 2000 / T = %s" % x))
    for T, pins in ((1, ["pairwise_8"]), (7, ["pairwise_8"]), (8, ["pairwise_8", "pairwise_tail"]),
                    (9, ["pairwise_tail"]), (127, ["pairwise_128"]), (128, ["pairwise_128"]),
                    (129, ["pairwise_128"])):
        b = Builder(f"pw_{T}", sub=0.10)
        add(Case(f"pw_{T}", _fam(b, b.plain(5, T)), pins, dict(R=5, T=T, ncig_max=1)))
    # ---- k_decide / k_decide_deep
    for R in (64, 65):
        name = f"deep_mdm_{R}"
        b = Builder(name)
        a1 = [b.read(0, [(0, 75), (2, 1), (0, 75)]) if j % 9 == 4 else b.read(0, [(0, 151)]) for j in range(R)]
        add(Case(name, _fam(b, a1), ["recmeta_wave", "deep_reads"],
                 dict(R=R, T=151, ncig_max=3, runs=[(j, 3) for j in range(4, R, 9)])))
    for T, pins in ((64, ["deep_nt1"]), (65, ["deep_nt1"]), (128, ["deep_nt2"]), (129, ["deep_nt2"]),
                    (192, ["deep_nt3"]), (193, ["deep_nt3"]), (256, ["deep_t256"]),
                    (257, ["deep_t256"])):
        add(_two_offsets(f"deep_t_{T}", 100, T, pins, L=min(150, T - 4)))
    for R in (495, 496, 497, 991, 992, 993):
        add(_two_offsets(f"deep_r_{R}", R, 64, ["deep_widen_1" if R < 900 else "deep_widen_2"], L=60))
    for R in (4095, 4096):
        add(_two_offsets(f"deep_r_{R}", R, 60, ["deep_max_r"], L=50))
    for R in (64, 65):
        # test_gpu_underflow_columns' column: one 'G' beside sequenced 'N' at maxQ
        name = f"underflow_{R}"
        b = Builder(name, sub=0.0, quals=(60,))
        a1 = b.plain(R, 40)
        for j, r in enumerate(a1):
            s = r.query_sequence
            r.query_sequence = s[:10] + ("G" if j == 0 else "N") + s[11:]
        add(Case(name, _fam(b, a1), ["decide_underflow"], dict(R=R, T=40, ncig_max=1),
                 note="every class product underflows: NaN posterior, the call is 'A'"))
    # ---- k_ins_layout eligibility: a plain subfamily and one read with the insertion
    def ins(name, cig, pins, R=5, off2=None, **decl):
        b = Builder(name)
        a1 = b.plain(R - 1) if off2 is None else [b.read(0 if j % 2 == 0 else off2, [(0, 150)]) for j in range(R - 1)]
        at = min(2, R - 1)
        a1.insert(at, b.read(0, cig))
        i_runs = [n for op, n in cig if op == 1]
        add(Case(name, _fam(b, a1), pins, dict(R=R, ncig_max=len(cig), runs=[(at, len(cig))], i_runs=[(at, i_runs)], **decl)))
    ins("ins_len_127", [(0, 60), (1, 127), (0, 60)], ["ins_run_len"], T=247)
    ins("ins_len_128", [(0, 60), (1, 128), (0, 60)], ["ins_run_len"], T=248)
    ins("ins_runs_4", [(1, 2), (0, 30), (2, 1), (0, 118)], ["ins_runs"], T=150)
    ins("ins_runs_5", [(0, 30), (1, 2), (0, 30), (2, 1), (0, 87)], ["ins_runs"], T=150)
    ins("ins_one_run", [(0, 40), (1, 2), (0, 108)], ["ins_two_runs", "ins_leading"], T=150)
    ins("ins_two_runs", [(0, 40), (1, 2), (0, 50), (1, 3), (0, 55)], ["ins_two_runs"], T=150)
    ins("ins_leading", [(1, 2), (0, 148)], ["ins_leading"], T=150)
    ins("ins_r_64", [(0, 70), (1, 2), (0, 78)], ["ins_chunk"], R=64, T=150)
    ins("ins_r_65", [(0, 70), (1, 2), (0, 78)], ["ins_chunk"], R=65, T=150)
    ins("ins_r_256", [(0, 70), (1, 2), (0, 78)], ["ins_max_r"], R=256, T=150)
    ins("ins_r_257", [(0, 70), (1, 2), (0, 78)], ["ins_max_r"], R=257, T=150)
    ins("ins_t_256", [(0, 70), (1, 2), (0, 78)], ["ins_max_t"], R=6, off2=106, T=256)
    ins("ins_t_257", [(0, 70), (1, 2), (0, 78)], ["ins_max_t"], R=6, off2=107, T=257)
    # ---- duplex pass: the two reads are the single-strand records of A1 and B2
    for off, pins in ((90, ["duplex_max_t"]), (91, ["duplex_max_t"]), (106, ["duplex_cols_lds"]),
                      (107, ["duplex_cols_lds"])):
        name = f"duplex_t_{150 + off}"
        b = Builder(name)
        add(Case(name, _fam(b, b.plain(3), b.plain(3, off=off)), pins, dict(R=3, T=150, duplex_T=150 + off, ncig_max=1)))
    b = Builder("duplex_indel")
    add(Case("duplex_indel", _fam(b, [b.read(0, [(0, 75), (2, 1), (0, 75)]) for _ in range(3)], b.plain(3)),
             ["duplex_cigar"], dict(R=3, T=150, duplex_T=150, ncig_max=3, runs=[(j, 3) for j in range(3)])))
    b = Builder("duplex_b2_all_n")
    b2 = b.plain(3)
    for r in b2:
        r.query_sequence = "N" * 150
    add(Case("duplex_b2_all_n", _fam(b, b.plain(3), b2), ["duplex_upstream"], dict(R=3, T=150, ncig_max=1),
             fails=True, note="every read of B2 is 'N' at every base: each fails its 3' trim (PREP | INDEX_ERROR in "
                              "both oracles), so the duplex is UPSTREAM, not the empty-consensus case below"))
    # one strand's consensus empty: two reads that disagree on both bases of M D M give 'N' '-' 'N',
    # the 'N' trims leave the CIGAR 1D and no base; the record is stored with status 0 and len 0,
    # and the duplex step fails when it reads it back (oracle/dcr_oracle.py consensus_core)
    for name, n, seqs, strand in (("duplex_empty_a1_1m1d1m", 1, ("AC", "CA"), 0), ("duplex_empty_b2_2m2d2m", 2, ("ACGT", "CATG"), 1)):
        b = Builder(name, sub=0.0, quals=(37,))
        sub = [b.read(0, [(0, n), (2, n), (0, n)]) for _ in seqs]
        for r, sq in zip(sub, seqs):
            r.query_sequence = sq
        add(Case(name, _fam(b, sub, None) if strand == 0 else _fam(b, b.plain(3), sub), ["duplex_len0"],
                 dict(R=2 if strand == 0 else 3), fails=True, expect=dict(ss0=ST_OK, ds0=ST_TYPE),
                 note="a strand's consensus has status 0 and len 0: the duplex is a TYPE_ERROR"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CACHE = {}


def cases():
    """The table (built once)."""
    if "cases" not in _CACHE:
        _CACHE["cases"] = _cases()
    return _CACHE["cases"]


def _pad_family(nbytes):
    """Four one-read subfamilies holding ``nbytes`` bases in all (nbytes >= 4)."""
    b = Builder("pad%d" % nbytes, sub=0.0, quals=(37,))
    lens = [nbytes // 4] * 3 + [nbytes - 3 * (nbytes // 4)]
    return [b.plain(1, L) for L in lens]


def families(sel):
    """The cases ``sel`` in that order as families.  A case with ``lo15`` gets
    a pad family in front of it, sized so that the case's first byte falls on
    lo15 modulo 16.  Returns (families, {case name: family index})."""
    fams, where, nbytes = [], {}, 0
    for c in sel:
        if c.lo15 is not None:
            pad = 600 + (c.lo15 - nbytes - 600) % 16
            fams.append(_pad_family(pad))
            nbytes += pad
            assert nbytes % 16 == c.lo15
        where[c.name] = len(fams)
        fams.append(c.fam)
        nbytes += sum(len(r.query_sequence) for s in c.fam for r in s)
    return fams, where


def build_batch(sel):
    """``families(sel)`` packed: (PackedBatch, {case name: family index})."""
    fams, where = families(sel)
    return pack_families(fams), where


# the combined batches: seed of the shuffle -> with the case that needs min_reads = 0
COMBINED = {1: False, 2: True}


def shuffled(seed):
    """Every case in a fixed shuffle; COMBINED[seed] tells whether the empty
    subfamily is among them (the batch then runs under PARAMS_MIN0)."""
    sel = [c for c in cases() if COMBINED[seed] or not c.min0]
    order = np.random.default_rng(seed).permutation(len(sel))
    return [sel[i] for i in order]


def combined_params(seed):
    return PARAMS_MIN0 if COMBINED[seed] else PARAMS


def slot_groups():
    """The cases that pass the ingest, split by their deepest subfamily for the
    slot path's hint: exactly 63 reads, exactly 64, and 65 or more.  Cases of
    fewer than 63 reads go into the 63 and the 64 group both; the failing ones
    go last into the third, so that its record stream before the first
    failing family holds every other family."""
    ok = [c for c in cases() if c.ingest]
    small = [c for c in ok if c.max_r < 63 and not c.fails]
    g63 = [c for c in ok if c.max_r == 63 and not c.fails] + small
    g64 = small[::-1] + [c for c in ok if c.max_r == 64 and not c.fails]
    g65 = [c for c in ok if c.max_r >= 65 and not c.fails] + [c for c in ok if c.fails]
    return {"r63": g63, "r64": g64, "r65": g65}


# ---- whole batches for k_recmeta's work split: (name, families, mean reads per record, read length)
RPW_BATCHES = {
    "rpw_64": dict(n_fam=300, mean=16, rpw=64, waves=16, L=30),
    "rpw_32": dict(n_fam=40, mean=17, rpw=32, waves=4, L=30),
    "rpw_16": dict(n_fam=5, mean=33, rpw=16, waves=4, L=30),
    "rpw_1": dict(n_fam=1, mean=1100, rpw=1, waves=4, L=30),
}


def rpw_batch(name):
    """Records of varied sizes with ``n_reads // n_rec == mean``.  Sizes are
    drawn around the mean (so records straddle the 64-read chunks and the
    384-read groups of their wave) and the last is set to fix the total;
    rpw_1 is one family of four subfamilies of 1,100 reads."""
    if name in _CACHE:
        return _CACHE[name]
    spec = RPW_BATCHES[name]
    b = Builder(name, width=64)
    n_rec, mean = 4 * spec["n_fam"], spec["mean"]
    if name == "rpw_1":
        sizes = [mean] * 4
    else:
        sizes = [int(x) for x in b.rng.integers(max(1, mean - 12), mean + 13, n_rec)]
        sizes[-1] = 1
        sizes[-1] = n_rec * mean + n_rec // 2 - sum(sizes) + 1
        assert sizes[-1] >= 1
    fams = [[[b.read(int(b.rng.integers(0, 8)), [(0, spec["L"])]) for _ in range(sizes[4 * f + k])] for k in range(4)]
            for f in range(spec["n_fam"])]
    _CACHE[name] = pack_families(fams)
    return _CACHE[name]
