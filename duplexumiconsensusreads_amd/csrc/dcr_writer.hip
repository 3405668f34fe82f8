// dcr_writer.hip — the record writer on the GPU: the two duplex BAM records
// of every family of a batch formatted straight from the kernel outputs in
// HBM, the failure scan, and the BGZF compression of the record stream
// (dcr_deflate.h), so that only compressed blocks cross PCIe.  On request
// (dcr_submit_write_ss) also the four single-strand records of every family,
// as a second record stream compressed by the same kernels; and with a filter
// set (dcr_set_filter) k_filter first, which masks weak duplex bases and marks
// the families neither stream writes.  With the per-base tags on
// (dcr_set_base_tags) kernels of their own format both streams, the default
// ones staying as they are.  With the per-base QC tables on
// (dcr_set_base_metrics) k_base_metrics counts over the same maps.
// With a genome set (dcr_set_genome) k_genome_metrics counts the records as
// called against it, at the end of this file.
//
// Reference (/root/reference/DuplexUMIConsensusReads.py): record fields
// make_consensus_read :1352-1384, names / flags :892-968, duplex tags
// add_tags :1076-1120, mate fields fix_paired_end_fields :1390-1419.  The
// byte layout is exactly the host formatter's (csrc/dcr_format.cpp), which
// tests/test_cli_e2e.py pins to the Python record codec.
#include <hip/hip_runtime.h>

#include "dcr_deflate.h"
#include "dcr_internal.h"
#include "dcr_writer.h"

namespace dcrw {

constexpr int kW = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & (kW - 1); }

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < kW; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, kW);
        if (l >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kW);
    return v;
}

__device__ __forceinline__ uint32_t ndigits(uint32_t v) {
    return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : 10;
}
__device__ __forceinline__ uint32_t int_tag_bytes(int64_t v) {
    if (v < 0) return v >= -128 ? 4 : v >= -32768 ? 5 : 7;
    return v <= 255 ? 4 : v <= 65535 ? 5 : 7;
}

__device__ __forceinline__ int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

__device__ __forceinline__ uint8_t nt_code(uint8_t c) {
    // "=ACMGRSVTWYHKDBN" (either case), unknown letters 15
    switch (c | 0x20) {
        case 'a': return 1; case 'c': return 2; case 'm': return 3; case 'g': return 4; case 'r': return 5;
        case 's': return 6; case 'v': return 7; case 't': return 8; case 'w': return 9; case 'y': return 10;
        case 'h': return 11; case 'k': return 12; case 'd': return 13; case 'b': return 14; case 'n': return 15;
        default: return c == '=' ? 0 : 15;
    }
}

__device__ __forceinline__ uint32_t dstrlen(const char *s) {
    uint32_t n = 0;
    while (s[n]) ++n;
    return n;
}

// text bytes of a "[1, 2, 3]" list (digits and separators only)
__device__ uint32_t list_body(const uint16_t *v, int32_t n) {
    uint32_t t = 0;
    for (int32_t i = lane_id(); i < n; i += kW) t += ndigits(v[i]);
    t = wave_sum(t);
    return t + (n > 0 ? 2u * (uint32_t)(n - 1) : 0u);
}

struct Rec {
    int32_t k, f, j, a, b;
    int32_t L, nc, tid, pos, opos, tlen, mapq;
    int64_t ro, ao, bo;
    const char *code, *rx;
    uint32_t lc, lr;
    int32_t a0, a1, b0, b1;
};

__device__ void rec_setup(const FmtArgs &A, int32_t k, Rec &r) {
    r.k = k;
    r.f = k >> 1;
    r.j = k & 1;
    r.a = 4 * r.f + 2 * r.j;
    r.b = r.a + 1;
    r.L = A.ds.len[k];
    r.nc = A.ds.n_cig[k];
    r.tid = A.fam_tid[r.f];
    r.pos = A.ds.pos[k];
    r.opos = A.ds.pos[2 * r.f + 1 - r.j];
    const int32_t t = A.ds.pos[2 * r.f + 1] + A.ds.len[2 * r.f + 1] - A.ds.pos[2 * r.f];
    r.tlen = r.j == 0 ? t : -t;
    r.mapq = A.ds.mapq[k];
    r.ro = A.ds_col_off[k];
    r.ao = A.ss_col_off[r.a];
    r.bo = A.ss_col_off[r.b];
    r.code = A.names + A.fam_code[r.f];
    r.rx = A.names + A.fam_rx[2 * r.f + r.j];
    r.lc = dstrlen(r.code);
    r.lr = dstrlen(r.rx);
    r.a0 = A.sub_off[r.a];
    r.a1 = A.sub_off[r.a + 1];
    r.b0 = A.sub_off[r.b];
    r.b1 = A.sub_off[r.b + 1];
}

__device__ uint32_t rec_size(const FmtArgs &A, const Rec &r) {
    const dcr_out &ss = A.ss, &ds = A.ds;
    uint32_t n = 36 + 16 + r.lc + 12 + 1 + 4u * (uint32_t)r.nc + (uint32_t)((r.L + 1) >> 1) + (uint32_t)r.L;
    n += 3 + r.lc + 1 + 3 + r.lr + 1;                                  // MI, RX
    n += 8 + (uint32_t)(r.a1 - r.a0) + 8 + (uint32_t)(r.b1 - r.b0) + 8 + 2;   // aQ bQ cQ
    const uint16_t *dl[3] = {ss.d + r.ao, ss.d + r.bo, ds.d + r.ro};
    const uint16_t *el[3] = {ss.e + r.ao, ss.e + r.bo, ds.e + r.ro};
    const int32_t nn[3] = {ss.n_de[r.a], ss.n_de[r.b], ds.n_de[r.k]};
    for (int i = 0; i < 3; ++i) n += 6 + list_body(dl[i], nn[i]);
    for (int i = 0; i < 3; ++i) n += 6 + list_body(el[i], nn[i]);
    n += int_tag_bytes(ss.D[r.a]) + int_tag_bytes(ss.D[r.b]) + int_tag_bytes(ds.D[r.k]);
    n += int_tag_bytes(ss.M[r.a]) + int_tag_bytes(ss.M[r.b]) + int_tag_bytes(ds.M[r.k]);
    n += 3 * 7;
    n += 2 * (4 + (uint32_t)ss.len[r.a]) + 2 * (4 + (uint32_t)ss.len[r.b]);   // ac bc aq bq
    return n;
}

// byte writer: scalar pieces by lane 0, arrays by the whole wave
struct Out {
    uint8_t *o;
    uint32_t p;
    __device__ void b1(uint32_t v) {
        if (lane_id() == 0) o[p] = (uint8_t)v;
        p += 1;
    }
    __device__ void u16(uint32_t v) {
        if (lane_id() == 0) { o[p] = (uint8_t)v; o[p + 1] = (uint8_t)(v >> 8); }
        p += 2;
    }
    __device__ void u32(uint32_t v) {
        if (lane_id() == 0)
            for (int i = 0; i < 4; ++i) o[p + i] = (uint8_t)(v >> (8 * i));
        p += 4;
    }
    __device__ void str(const char *s, uint32_t n) {
        for (uint32_t i = lane_id(); i < n; i += kW) o[p + i] = (uint8_t)s[i];
        p += n;
    }
    __device__ void bytes(const uint8_t *s, uint32_t n) {
        for (uint32_t i = lane_id(); i < n; i += kW) o[p + i] = s[i];
        p += n;
    }
    __device__ void tag(char a, char b, char t) { b1((uint8_t)a); b1((uint8_t)b); b1((uint8_t)t); }
    __device__ void int_tag(char a, char b, int64_t v) {
        b1((uint8_t)a);
        b1((uint8_t)b);
        if (v < 0) {
            if (v >= -128) { b1('c'); b1((uint8_t)(int8_t)v); }
            else if (v >= -32768) { b1('s'); u16((uint16_t)(int16_t)v); }
            else { b1('i'); u32((uint32_t)(int32_t)v); }
        } else if (v <= 255) { b1('C'); b1((uint32_t)v); }
        else if (v <= 65535) { b1('S'); u16((uint32_t)v); }
        else { b1('I'); u32((uint32_t)v); }
    }
    __device__ void float_tag(char a, char b, double v) {
        b1((uint8_t)a);
        b1((uint8_t)b);
        b1('f');
        const float f = (float)v;
        u32(__float_as_uint(f));
    }
    __device__ void list(char a, char b, const uint16_t *v, int32_t n) {
        tag(a, b, 'Z');
        b1('[');
        for (int32_t c0 = 0; c0 < n; c0 += kW) {
            const int32_t i = c0 + lane_id();
            uint32_t x = 0, len = 0;
            if (i < n) {
                x = v[i];
                len = ndigits(x) + (i > 0 ? 2u : 0u);
            }
            const uint32_t incl = wave_incl_scan(len);
            const uint32_t tot = __shfl(incl, kW - 1, kW);
            if (i < n) {
                uint8_t *q = o + p + (incl - len);
                if (i > 0) { q[0] = ','; q[1] = ' '; q += 2; }
                const uint32_t nd = ndigits(x);
                for (int d = (int)nd - 1; d >= 0; --d) { q[d] = (uint8_t)('0' + x % 10); x /= 10; }
            }
            p += tot;
        }
        b1(']');
        b1(0);
    }
};

__device__ void rec_write(const FmtArgs &A, const Rec &r, uint8_t *o, uint32_t total) {
    const dcr_out &ss = A.ss, &ds = A.ds;
    Out w{o, 0};
    w.u32(total - 4);
    w.u32((uint32_t)r.tid);
    w.u32((uint32_t)r.pos);
    w.b1(16 + r.lc + 12 + 1);
    w.b1((uint32_t)(r.mapq & 0xff));
    const uint32_t *cg = ds.cigar + r.ro;
    int64_t rl = 0;
    if (lane_id() == 0)
        for (int32_t i = 0; i < r.nc; ++i) {
            const uint32_t op = cg[i] & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[i] >> 4;
        }
    w.u16(r.pos >= 0 ? (uint32_t)reg2bin(r.pos, r.pos + (rl > 0 ? rl : 1)) : 4680u);
    w.u16((uint32_t)r.nc);
    w.u16(r.j == 0 ? 99u : 147u);
    w.u32((uint32_t)r.L);
    w.u32((uint32_t)r.tid);
    w.u32((uint32_t)r.opos);
    w.u32((uint32_t)r.tlen);
    w.str("consensus_family", 16);
    w.str(r.code, r.lc);
    w.str(r.j == 0 ? "_paired-end1" : "_paired-end2", 12);
    w.b1(0);
    for (int32_t i = lane_id(); i < r.nc; i += kW) {
        const uint32_t v = cg[i];
        for (int b = 0; b < 4; ++b) o[w.p + 4 * i + b] = (uint8_t)(v >> (8 * b));
    }
    w.p += 4u * (uint32_t)r.nc;
    const uint8_t *sq = ds.seq + r.ro;
    const int32_t nb = (r.L + 1) >> 1;
    for (int32_t i = lane_id(); i < nb; i += kW) {
        const uint8_t hi = nt_code(sq[2 * i]);
        const uint8_t lo = (2 * i + 1 < r.L) ? nt_code(sq[2 * i + 1]) : 0;
        o[w.p + i] = (uint8_t)((hi << 4) | lo);
    }
    w.p += (uint32_t)nb;
    w.bytes(ds.qual + r.ro, (uint32_t)r.L);
    w.tag('M', 'I', 'Z');
    w.str(r.code, r.lc);
    w.b1(0);
    w.tag('R', 'X', 'Z');
    w.str(r.rx, r.lr);
    w.b1(0);
    w.tag('a', 'Q', 'B'); w.b1('C'); w.u32((uint32_t)(r.a1 - r.a0)); w.bytes(A.read_mapq + r.a0, (uint32_t)(r.a1 - r.a0));
    w.tag('b', 'Q', 'B'); w.b1('C'); w.u32((uint32_t)(r.b1 - r.b0)); w.bytes(A.read_mapq + r.b0, (uint32_t)(r.b1 - r.b0));
    w.tag('c', 'Q', 'B'); w.b1('C'); w.u32(2); w.b1((uint32_t)ss.mapq[r.a] & 0xff); w.b1((uint32_t)ss.mapq[r.b] & 0xff);
    w.list('a', 'd', ss.d + r.ao, ss.n_de[r.a]);
    w.list('b', 'd', ss.d + r.bo, ss.n_de[r.b]);
    w.list('c', 'd', ds.d + r.ro, ds.n_de[r.k]);
    w.int_tag('a', 'D', ss.D[r.a]); w.int_tag('b', 'D', ss.D[r.b]); w.int_tag('c', 'D', ds.D[r.k]);
    w.int_tag('a', 'M', ss.M[r.a]); w.int_tag('b', 'M', ss.M[r.b]); w.int_tag('c', 'M', ds.M[r.k]);
    w.list('a', 'e', ss.e + r.ao, ss.n_de[r.a]);
    w.list('b', 'e', ss.e + r.bo, ss.n_de[r.b]);
    w.list('c', 'e', ds.e + r.ro, ds.n_de[r.k]);
    w.float_tag('a', 'E', ss.E[r.a]); w.float_tag('b', 'E', ss.E[r.b]); w.float_tag('c', 'E', ds.E[r.k]);
    w.tag('a', 'c', 'Z'); w.bytes(ss.seq + r.ao, (uint32_t)ss.len[r.a]); w.b1(0);
    w.tag('b', 'c', 'Z'); w.bytes(ss.seq + r.bo, (uint32_t)ss.len[r.b]); w.b1(0);
    w.tag('a', 'q', 'Z');
    for (int32_t i = lane_id(); i < ss.len[r.a]; i += kW) o[w.p + i] = (uint8_t)(ss.qual[r.ao + i] + 33);
    w.p += (uint32_t)ss.len[r.a];
    w.b1(0);
    w.tag('b', 'q', 'Z');
    for (int32_t i = lane_id(); i < ss.len[r.b]; i += kW) o[w.p + i] = (uint8_t)(ss.qual[r.bo + i] + 33);
    w.p += (uint32_t)ss.len[r.b];
    w.b1(0);
}

// ---- the consensus filters (dcr_set_filter; include/dcr.h states the rules).
// One wave per family, both duplex records.  The lanes stride the record's
// seq / qual region a dword (four bases) at a time: regions start on
// 16-column boundaries and are whole multiples of 16 columns, so the last
// partial word stays inside the record's own region; its bytes at or past
// len are neither counted nor changed.  Bases below min_base_quality are
// masked in place, then 'N' bases, the quality sum and the masked bases are
// wave-reduced and lane 0 tests the rules on the record's scalars.
__global__ __launch_bounds__(256) void k_filter(FilterArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    const dcr_filter &T = A.flt;
    // quality bytes are below 256: a larger threshold masks every base
    const uint32_t minq = (T.active & DCR_FILT_MASK_BASES) ? (uint32_t)(T.min_base_quality < 256 ? T.min_base_quality : 256) : 0u;
    for (int64_t f = wave; f < A.n_fam; f += nw) {
        if (A.fam_fail[f] != 0) {
            if (lane_id() == 0) A.fam_filt[f] = 0;
            continue;
        }
        uint32_t why = 0, masked = 0;
        for (int j = 0; j < 2; ++j) {
            const int64_t k = 2 * f + j, a = 4 * f + 2 * j, b = a + 1;
            const int64_t ro = A.ds_col_off[k], room = A.ds_col_off[k + 1] - ro;
            int64_t L = A.ds.len[k];
            L = L < 0 ? 0 : L > room ? room : L;
            uint32_t *sq = reinterpret_cast<uint32_t *>(A.ds.seq + ro);
            uint32_t *ql = reinterpret_cast<uint32_t *>(A.ds.qual + ro);
            uint32_t n_n = 0, q_sum = 0, n_m = 0;
            for (int64_t w = lane_id(); 4 * w < L; w += kW) {
                const uint32_t s0 = sq[w], q0 = ql[w];
                const int nb = L - 4 * w < 4 ? (int)(L - 4 * w) : 4;
                uint32_t s1 = s0, q1 = q0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i >= nb) break;
                    uint32_t sb = (s0 >> (8 * i)) & 0xffu, qb = (q0 >> (8 * i)) & 0xffu;
                    if (qb < minq) {
                        sb = 'N';
                        qb = qb < 2 ? qb : 2;
                        s1 = (s1 & ~(0xffu << (8 * i))) | (sb << (8 * i));
                        q1 = (q1 & ~(0xffu << (8 * i))) | (qb << (8 * i));
                        ++n_m;
                    }
                    n_n += sb == 'N';
                    q_sum += qb;
                }
                if (s1 != s0) sq[w] = s1;
                if (q1 != q0) ql[w] = q1;
            }
            n_n = wave_sum(n_n);
            q_sum = wave_sum(q_sum);
            masked += wave_sum(n_m);
            const int32_t aD = A.ss.D[a], bD = A.ss.D[b];
            if (T.active & DCR_FILT_MIN_READS) {
                const int32_t hi = aD > bD ? aD : bD, lo = aD > bD ? bD : aD;
                if (!((int64_t)aD + bD >= T.min_reads[0] && hi >= T.min_reads[1] && lo >= T.min_reads[2]))
                    why |= DCR_FILT_MIN_READS;
            }
            if (T.active & DCR_FILT_ERROR_RATE)
                if (!(A.ds.E[k] <= T.max_error_rate[0] && A.ss.E[a] <= T.max_error_rate[1] &&
                      A.ss.E[b] <= T.max_error_rate[1]))
                    why |= DCR_FILT_ERROR_RATE;
            if ((T.active & DCR_FILT_NO_CALL) && (double)n_n > T.max_no_call_fraction * (double)L)
                why |= DCR_FILT_NO_CALL;
            if ((T.active & DCR_FILT_MEAN_QUAL) && (double)q_sum < T.min_mean_base_quality * (double)L)
                why |= DCR_FILT_MEAN_QUAL;
        }
        // k_base_filter's count leaves out every base whose quality it left below minq (those were
        // counted above), so the sum counts each masked base once
        if (A.base_masked) masked += (uint32_t)A.base_masked[f];
        if (lane_id() == 0) A.fam_filt[f] = (int32_t)(why | (masked << 8));
    }
}

// ---- the per-base filters (dcr_set_base_filter; include/dcr.h states the
// rules and the two levels of the map).  One wave per family, both duplex
// records, the lanes striding seq / qual a dword at a time as k_filter does;
// runs before k_filter, which then counts 'N' and sums qualities over the
// bases masked here and adds this kernel's count into fam_filt.
//
// A lane finds the columns of its own bases; no LDS.  Records without
// insertion columns (the fast list's single M runs, and whatever else has no
// stored map) follow from pos and CIGAR: t5 = pos - min(read pos), an M run
// is bases on consecutive columns, a D run skips columns.  When the duplex
// record and both strands are one M run each this is lane arithmetic
// (col_r(i) = t5_r + i, ia = min_pos_r + col_r(i) - pos_a, col_a(ia) = t5_a +
// ia); otherwise each lane walks the few runs of the two strands' CIGARs the
// way reconstruct_alignment (:430-547) lays them out, and reads the stored
// maps (dcr::BaseMap) of the records that have them.  Every index is
// clamped to the record's region before it is used.
struct BfRec {
    const uint32_t *cig;    // consensus CIGAR
    const uint32_t *col;    // stored d-index per base (mapped), else unused
    const uint16_t *d, *e;
    int64_t len, nde, ncig; // clamped to [0, the region]
    int64_t pos, t5;
    bool mapped, simple;    // a stored map; one M run of len bases and no stored map
};

constexpr int64_t kBfInf = (int64_t)1 << 40;

__device__ __forceinline__ int64_t bf_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : v > hi ? hi : v; }

__device__ __forceinline__ void bf_rec(const dcr_out &o, const int64_t *col_off, int64_t r, const uint32_t *col,
                                       bool mapped, BfRec &R) {
    const int64_t ro = col_off[r], room = col_off[r + 1] - ro;
    R.cig = o.cigar + ro;
    R.col = col + ro;
    R.d = o.d + ro;
    R.e = o.e + ro;
    R.len = bf_clamp(o.len[r], room);
    R.nde = bf_clamp(o.n_de[r], room);
    R.ncig = bf_clamp(o.n_cig[r], room);
    R.pos = o.pos[r];
    R.t5 = 0;
    R.mapped = mapped;
    R.simple = !mapped && R.ncig == 1 && R.len > 0 && R.cig[0] == ((uint32_t)R.len << 4);
}

// the d-index of base i of a record (Level 1), -1 when it has none
__device__ int64_t bf_own_col(const BfRec &R, int64_t i) {
    if (i < 0 || i >= R.len) return -1;
    if (R.mapped) return (int64_t)R.col[i];
    if (R.simple) return R.t5 + i;
    int64_t is = 0, dc = R.t5;
    for (int64_t k = 0; k < R.ncig; ++k) {
        const int64_t n = R.cig[k] >> 4;
        if ((R.cig[k] & 15u) == 2u) {
            dc += n;
        } else {
            if (i < is + n) return dc + (i - is);
            is += n;
            dc += n;
        }
    }
    return -1;
}

// a strand's place in its CIGAR during the two-read layout
struct BfCur {
    int64_t k, rem, is;
    int op;                 // 0 base-consuming, 1 I, 2 D (:361-377: everything but I and D lays a base)
};
__device__ __forceinline__ void bf_load(const BfRec &R, BfCur &c) {
    while (c.k < R.ncig && (R.cig[c.k] >> 4) == 0) ++c.k;     // expand_cigartuples drops empty runs
    if (c.k < R.ncig) {
        const uint32_t v = R.cig[c.k];
        c.rem = v >> 4;
        c.op = (v & 15u) == 1u ? 1 : (v & 15u) == 2u ? 2 : 0;
    } else {
        c.rem = kBfInf;     // past the last run: the reference reads M (:408-427)
        c.op = 0;
    }
}

// Level 2: the base indices ia / ib (-1: none) that the two strands put into
// alignment column t of their duplex record, by runs instead of by columns
__device__ void bf_sources(const BfRec &A, const BfRec &B, int64_t minpos, int64_t t, int64_t &ia, int64_t &ib) {
    const BfRec *R[2] = {&A, &B};
    BfCur c[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    bf_load(A, c[0]);
    bf_load(B, c[1]);
    int64_t out[2] = {-1, -1};
    int64_t col = 0, p = minpos;
    while (col <= t) {
        int64_t n = kBfInf, src[2] = {-1, -1};
        int kind[2] = {0, 0};                      // 0 nothing, 1 bases, 2 deletion, 3 inserted bases
        if (c[0].op == 1 || c[1].op == 1) {        // insertion columns (:476-503): '+' for the other strand
            for (int s = 0; s < 2; ++s)
                if (c[s].op == 1) {
                    kind[s] = 3;
                    src[s] = c[s].is;
                    n = c[s].rem < n ? c[s].rem : n;
                }
        } else {
            for (int s = 0; s < 2; ++s) {
                int64_t seg = kBfInf;
                if (p < R[s]->pos) {
                    seg = R[s]->pos - p;           // 'N' padding before the read (:506)
                } else if (c[s].is < R[s]->len && c[s].k < R[s]->ncig) {
                    if (c[s].op == 2) {
                        kind[s] = 2;
                        seg = c[s].rem;
                    } else {
                        kind[s] = 1;
                        src[s] = c[s].is;
                        const int64_t left = R[s]->len - c[s].is;
                        seg = c[s].rem < left ? c[s].rem : left;
                    }
                }                                  // else 'N' padding after the read (:540)
                n = seg < n ? seg : n;
            }
        }
        if (t < col + n) {
            for (int s = 0; s < 2; ++s)
                if ((kind[s] & 1) && src[s] + (t - col) < R[s]->len) out[s] = src[s] + (t - col);
            break;
        }
        for (int s = 0; s < 2; ++s)
            if (kind[s]) {
                c[s].rem -= n;
                if (kind[s] != 2) c[s].is += n;
                if (c[s].rem == 0) {
                    ++c[s].k;
                    bf_load(*R[s], c[s]);
                }
            }
        col += n;
        p += n;
    }
    ia = out[0];
    ib = out[1];
}

__global__ __launch_bounds__(256) void k_base_filter(BaseFilterArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    const dcr_base_filter &T = A.flt;
    const uint32_t skip = (uint32_t)(A.skip_below < 0 ? 0 : A.skip_below);
    for (int64_t f = wave; f < A.n_fam; f += nw) {
        if (A.fam_fail[f] != 0) {
            if (lane_id() == 0) A.masked[f] = 0;
            continue;
        }
        uint32_t masked = 0;
        for (int j = 0; j < 2; ++j) {
            const int64_t k = 2 * f + j, a = 4 * f + 2 * j;
            BfRec S[2], R;
            for (int s = 0; s < 2; ++s) {
                bf_rec(A.ss, A.ss_col_off, a + s, A.ss_col, A.flag[a + s] != 0, S[s]);
                if (!S[s].mapped) {                // min_pos of the strand's own layout: its reads' smallest start
                    const int32_t r0 = A.sub_off[a + s], r1 = A.sub_off[a + s + 1];
                    int32_t mp = 0x7fffffff;
                    for (int32_t r = r0 + lane_id(); r < r1; r += kW) mp = A.read_pos[r] < mp ? A.read_pos[r] : mp;
#pragma unroll
                    for (int dd = 32; dd >= 1; dd >>= 1) {
                        const int32_t o = __shfl_xor(mp, dd, kW);
                        mp = o < mp ? o : mp;
                    }
                    S[s].t5 = r1 > r0 ? S[s].pos - (int64_t)mp : 0;
                }
            }
            bf_rec(A.ds, A.ds_col_off, k, A.ds_col, A.flag[4 * (int64_t)A.n_fam + k] != 0, R);
            const int64_t ro = A.ds_col_off[k];
            const int64_t minpos = S[0].pos < S[1].pos ? S[0].pos : S[1].pos;
            R.t5 = R.pos - minpos;
            const uint32_t *aln = A.ds_aln + ro;
            const bool lane_math = R.simple && S[0].simple && S[1].simple;
            const int64_t L = R.len;
            uint32_t *sq = reinterpret_cast<uint32_t *>(A.ds.seq + ro);
            uint32_t *ql = reinterpret_cast<uint32_t *>(A.ds.qual + ro);
            uint32_t n_m = 0;
            for (int64_t w = lane_id(); 4 * w < L; w += kW) {
                const uint32_t s0 = sq[w], q0 = ql[w];
                const int nb = L - 4 * w < 4 ? (int)(L - 4 * w) : 4;
                uint32_t s1 = s0, q1 = q0;
                for (int i = 0; i < nb; ++i) {
                    const uint32_t qb = (q0 >> (8 * i)) & 0xffu;
                    if (qb < skip) continue;
                    const int64_t bi = 4 * w + i;
                    int64_t c, ca, cb;             // d-indices in r, a, b (-1: none)
                    if (lane_math) {
                        c = R.t5 + bi;
                        const int64_t p = minpos + c;
                        ca = bf_own_col(S[0], p - S[0].pos);
                        cb = bf_own_col(S[1], p - S[1].pos);
                    } else {
                        int64_t t, ia, ib;
                        if (R.mapped) {
                            c = (int64_t)R.col[bi];
                            t = (int64_t)aln[bi];
                        } else {
                            c = t = bf_own_col(R, bi);        // no '+' column: the d-index is the alignment column
                        }
                        bf_sources(S[0], S[1], minpos, t, ia, ib);
                        ca = bf_own_col(S[0], ia);
                        cb = bf_own_col(S[1], ib);
                    }
                    const bool va = ca >= 0 && ca < S[0].nde, vb = cb >= 0 && cb < S[1].nde;
                    const int32_t aD = va ? S[0].d[ca] : 0, aE = va ? S[0].e[ca] : 0;
                    const int32_t bD = vb ? S[1].d[cb] : 0, bE = vb ? S[1].e[cb] : 0;
                    const int32_t cE = (c >= 0 && c < R.nde) ? R.e[c] : 0;
                    bool m = false;
                    if (T.active & DCR_BF_MIN_READS) {
                        const int32_t hi = aD > bD ? aD : bD, lo = aD > bD ? bD : aD;
                        m |= !(aD + bD >= T.min_reads[0] && hi >= T.min_reads[1] && lo >= T.min_reads[2]);
                    }
                    if (T.active & DCR_BF_ERROR_RATE) m |= (double)(aE + bE) > T.max_error_rate * (double)(aD + bD);
                    if (T.active & DCR_BF_AGREEMENT) m |= cE > 0;
                    if (m) {
                        const uint32_t q2 = qb < 2 ? qb : 2;
                        s1 = (s1 & ~(0xffu << (8 * i))) | ((uint32_t)'N' << (8 * i));
                        q1 = (q1 & ~(0xffu << (8 * i))) | (q2 << (8 * i));
                        // k_filter masks and counts whatever it then finds below its bound, this base
                        // at its new quality included: count here only what it will not count again
                        n_m += q2 >= skip ? 1u : 0u;
                    }
                }
                if (s1 != s0) sq[w] = s1;
                if (q1 != q0) ql[w] = q1;
            }
            masked += wave_sum(n_m);
        }
        if (lane_id() == 0) A.masked[f] = (int32_t)masked;
    }
}

// ---- the consensus QC tables (dcr_set_metrics; include/dcr.h states them).
// A workgroup of 16 waves, one wave per family at a time: first the four
// single-strand records of its families, then the two duplex ones.
// Nothing per base or per column goes to HBM one by one: a same-address
// device atomic costs about 30 ns serialised and a batch holds ten million
// columns in a few hundred bins.  Three levels instead:
//   lanes   a lane takes 16 quality bytes (one dwordx4) and adds once per
//           run of equal bytes; it takes 8 columns of d / e (one dwordx4) and
//           keeps bins 8*lane .. 8*lane + 7 of the column tables in registers
//           (column c' < 512 of every record belongs to the same lane);
//   wave    the lanes whose 16 bytes all equal the first lane's quality (the
//           hot bin) are added by one lane with one LDS add;
//   LDS     the workgroup's copy of the whole dcr_metrics, 64-bit for the
//           per-base tables and 32-bit for the per-record ones; at the end
//           one global 64-bit add per non-zero bin per workgroup.
// No counter wraps: the 32-bit register bins take at most 4 records * 65535
// per family and are emptied into 64-bit LDS bins every kMetFlush families
// (4 * 4096 * 65535 < 2^32); columns and record counts past bin 511, which
// have no such bound, are summed in 64-bit lane variables; the 32-bit LDS
// bins are per-record tables, each taking at most 2 per family of a batch
// whose n_fam is an int32; everything else in LDS and HBM is 64-bit.
// Loads: regions start on 16-column boundaries and are whole multiples of 16
// columns, so a 16-byte load of qual / seq (16 columns) or of d / e (8
// columns) that begins inside [0, n) on its own alignment stays inside the
// region.  Reverse records are read from their end, 16 bytes at a 2-byte
// alignment, so that column c' = n - 1 - c lands on the same lane as a
// forward record's; a lane with fewer than 8 columns left reads them singly.
// The single-strand seq is not touched.
constexpr int kMetFlush = 4096;
constexpr int kMetRecBase = (int)(offsetof(dcr_metrics, ss_reads) / 8);    // the per-record tables: 32-bit in LDS
constexpr int kMetBigBase = (int)(offsetof(dcr_metrics, ss_qual) / 8);     // per base / per column: 64-bit in LDS
constexpr int kMetWords = (int)(sizeof(dcr_metrics) / 8);
constexpr int kMetDepth = (int)(offsetof(dcr_metrics, ds_depth) / 8) - kMetRecBase;
constexpr int kMetErrC = (int)(offsetof(dcr_metrics, err_c) / 8) - kMetRecBase;
constexpr int kMetErrS = (int)(offsetof(dcr_metrics, err_s) / 8) - kMetRecBase;
constexpr int kMetCol = (int)(offsetof(dcr_metrics, col) / 8) - kMetBigBase;
static_assert(sizeof(dcr_metrics) % 8 == 0 && offsetof(dcr_metrics, n) == 0 && kMetRecBase == 8 &&
                  offsetof(dcr_metrics, ds_qual) / 8 - kMetBigBase == DCR_MET_QUAL_BINS && DCR_MET_COL_BINS == 8 * kW,
              "k_metrics' LDS layout follows dcr_metrics");

struct MetShared {
    unsigned long long n[8];
    unsigned long long big[kMetWords - kMetBigBase];    // ss_qual, ds_qual, col
    uint32_t rec[kMetBigBase - kMetRecBase];            // ss_reads, ds_depth, err_c, err_s
};

// a lane's share of one kind's column tables: bins 8 * lane + t, and what falls past bin 511
struct MetCols {
    uint32_t cnt[8], d[8], e[8];
    unsigned long long tail_n, tail_d, tail_e;
};

__device__ __forceinline__ int met_err_bin(double E) {
    return (E >= 0.0 && E <= 1.0) ? (int)__builtin_rint(E * 1000.0) : DCR_MET_ERR_BINS - 1;
}

__device__ __forceinline__ int64_t met_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the quality bytes [0, L) of a region into the 256-bin histogram h (LDS)
__device__ void met_qual(const uint8_t *q, uint32_t L, unsigned long long *h) {
    for (uint32_t w = lane_id(); w < (L + 15) / 16; w += kW) {
        const uint4 v = *reinterpret_cast<const uint4 *>(q + 16 * w);
        const int nb = L - 16 * w < 16 ? (int)(L - 16 * w) : 16;
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
        uint32_t cur = x[0] & 0xffu, run = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t b = (x[i >> 2] >> (8 * (i & 3))) & 0xffu;
            if (i < nb) {
                if (b != cur) {
                    atomicAdd(&h[cur], (unsigned long long)run);
                    cur = b;
                    run = 0;
                }
                ++run;
            }
        }
        // the lanes still in the loop whose 16 bytes are all the first such lane's quality: one add
        const uint32_t q0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
        const bool hot = cur == q0 && run == 16;
        const unsigned long long m = __ballot(hot);
        if (!hot)
            atomicAdd(&h[cur], (unsigned long long)run);
        else if (lane_id() == (int)__builtin_ctzll(m))
            atomicAdd(&h[q0], 16ull * (unsigned long long)__builtin_popcountll(m));
    }
}

// this lane's count of 'N' among the bytes [0, L) of a region (at most L / 64 + 16: 32 bits hold it)
__device__ uint32_t met_count_n(const uint8_t *s, uint32_t L) {
    uint32_t n = 0;
    for (uint32_t w = lane_id(); w < (L + 15) / 16; w += kW) {
        const uint4 v = *reinterpret_cast<const uint4 *>(s + 16 * w);
        const int nb = L - 16 * w < 16 ? (int)(L - 16 * w) : 16;
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) n += (i < nb && ((x[i >> 2] >> (8 * (i & 3))) & 0xffu) == 'N') ? 1u : 0u;
    }
    return n;
}

// v[t] = p[c'] for this lane's columns c' = c0 + t, t < nv (0 past them), of a
// record of n columns; REV: c' counts from the record's end
template <bool REV>
__device__ __forceinline__ void met_load8(const uint16_t *p, uint32_t n, uint32_t c0, int nv, uint32_t v[8]) {
    if (!REV) {
        const uint4 r = *reinterpret_cast<const uint4 *>(p + c0);
        const uint32_t x[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = t < nv ? (x[t >> 1] >> (16 * (t & 1))) & 0xffffu : 0u;
    } else if (nv >= 8) {
        uint4 r;
        __builtin_memcpy(&r, p + (n - 8 - c0), 16);
        const uint32_t x[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = (x[(7 - t) >> 1] >> (16 * ((7 - t) & 1))) & 0xffffu;
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = t < nv ? (uint32_t)p[n - 1 - c0 - t] : 0u;
    }
}

template <bool REV>
__device__ void met_cols(const uint16_t *d, const uint16_t *e, uint32_t n, MetCols &a) {
    const uint32_t l8 = 8 * lane_id();
#pragma unroll
    for (int t = 0; t < 8; ++t) a.cnt[t] += l8 + t < n ? 1u : 0u;
    if (n > DCR_MET_COL_BINS) a.tail_n += (unsigned long long)(n - DCR_MET_COL_BINS);
    for (uint32_t base = 0; base < n; base += DCR_MET_COL_BINS) {      // n < 2^31: no wrap
        const uint32_t c0 = base + l8;
        if (c0 >= n) break;
        const int nv = n - c0 < 8 ? (int)(n - c0) : 8;
        uint32_t vd[8], ve[8];
        met_load8<REV>(d, n, c0, nv, vd);
        met_load8<REV>(e, n, c0, nv, ve);
        if (base == 0) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                a.d[t] += vd[t];
                a.e[t] += ve[t];
            }
        } else {
            uint32_t sd = 0, se = 0;            // 8 * 65535 each
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                sd += vd[t];
                se += ve[t];
            }
            a.tail_d += sd;
            a.tail_e += se;
        }
    }
}

// a wave's register bins of one kind into the workgroup's tables, and cleared
__device__ void met_flush(MetCols &a, unsigned long long *col) {
    const int l8 = 8 * lane_id();
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (a.cnt[t]) atomicAdd(&col[0 * DCR_MET_COL_BINS + l8 + t], (unsigned long long)a.cnt[t]);
        if (a.d[t]) atomicAdd(&col[1 * DCR_MET_COL_BINS + l8 + t], (unsigned long long)a.d[t]);
        if (a.e[t]) atomicAdd(&col[2 * DCR_MET_COL_BINS + l8 + t], (unsigned long long)a.e[t]);
        a.cnt[t] = a.d[t] = a.e[t] = 0;
    }
    // tail_n is the same in every lane (the record's n), the sums are each lane's own
    if (a.tail_n && lane_id() == 0) atomicAdd(&col[0 * DCR_MET_COL_BINS + DCR_MET_COL_BINS - 1], a.tail_n);
    if (a.tail_d) atomicAdd(&col[1 * DCR_MET_COL_BINS + DCR_MET_COL_BINS - 1], a.tail_d);
    if (a.tail_e) atomicAdd(&col[2 * DCR_MET_COL_BINS + DCR_MET_COL_BINS - 1], a.tail_e);
    a.tail_n = a.tail_d = a.tail_e = 0;
}

// One kind's records (DS: the two duplex ones, else the four single-strand
// ones) of this wave's families.  Two passes over the families, one kind
// each, keep one MetCols in registers at a time.
template <bool DS>
__device__ void met_pass(const MetricsArgs &A, MetShared &S, int wave, int nw) {
    constexpr int R = DS ? 2 : 4;
    const dcr_out &o = DS ? A.ds : A.ss;
    const int64_t *col_off = DS ? A.ds_col_off : A.ss_col_off;
    unsigned long long *qual = S.big + (DS ? DCR_MET_QUAL_BINS : 0);
    unsigned long long *col = S.big + kMetCol + (DS ? 3 * DCR_MET_COL_BINS : 0);
    MetCols c{};
    unsigned long long n_len = 0, n_de = 0, n_n = 0;
    uint32_t fams = 0, since = 0;
    for (int64_t f = wave; f < A.n_fam; f += nw) {
        if (A.fam_fail[f] != 0) continue;
        ++fams;
#pragma nounroll
        for (int i = 0; i < R; ++i) {
            const int64_t r = R * f + i;
            const int64_t ro = col_off[r], room = col_off[r + 1] - ro;
            // len and n_de are int32: the clamped values fit 31 bits
            const uint32_t L = (uint32_t)met_clamp(o.len[r], room), N = (uint32_t)met_clamp(o.n_de[r], room);
            n_len += L;
            n_de += N;
            if (lane_id() == 0) {
                if (!DS) {
                    const int64_t nr = met_clamp((int64_t)A.sub_off[r + 1] - A.sub_off[r], DCR_MET_READS_BINS - 1);
                    atomicAdd(&S.rec[i * DCR_MET_READS_BINS + nr], 1u);
                } else {
                    const int64_t a = 4 * f + 2 * i, b = a + 1;
                    const int aD = (int)met_clamp(A.ss.D[a], DCR_MET_DEPTH_BINS - 1);
                    const int bD = (int)met_clamp(A.ss.D[b], DCR_MET_DEPTH_BINS - 1);
                    const int hi = aD > bD ? aD : bD, lo = aD > bD ? bD : aD;
                    atomicAdd(&S.rec[kMetDepth + hi * DCR_MET_DEPTH_BINS + lo], 1u);
                    atomicAdd(&S.rec[kMetErrC + met_err_bin(A.ds.E[r])], 1u);
                    const int ea = met_err_bin(A.ss.E[a]), eb = met_err_bin(A.ss.E[b]);
                    atomicAdd(&S.rec[kMetErrS + (ea > eb ? ea : eb)], 1u);
                }
            }
            met_qual(o.qual + ro, L, qual);
            if (DS) n_n += met_count_n(o.seq + ro, L);
            if (DS ? i == 0 : i < 2)
                met_cols<false>(o.d + ro, o.e + ro, N, c);
            else
                met_cols<true>(o.d + ro, o.e + ro, N, c);
        }
        if (++since == kMetFlush) {
            met_flush(c, col);
            since = 0;
        }
    }
    met_flush(c, col);
    if (n_n) atomicAdd(&S.n[3], n_n);                         // each lane's own count
    if (lane_id() == 0 && fams) {                             // the same in every lane
        if (DS) atomicAdd(&S.n[0], (unsigned long long)fams);
        atomicAdd(&S.n[DS ? 2 : 1], n_len);
        atomicAdd(&S.n[DS ? 5 : 4], n_de);
    }
}

__global__ __launch_bounds__(kMetThreads) void k_metrics(MetricsArgs A) {
    __shared__ MetShared S;
    for (int i = threadIdx.x; i < (int)(sizeof(MetShared) / 4); i += kMetThreads) reinterpret_cast<uint32_t *>(&S)[i] = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kMetThreads + threadIdx.x) / kW));
    const int nw = (int)(gridDim.x * (kMetThreads / kW));
    met_pass<false>(A, S, wave, nw);
    met_pass<true>(A, S, wave, nw);
    __syncthreads();
    // the workgroup's tables into the slot's: one 64-bit add per non-zero bin
    unsigned long long *out = reinterpret_cast<unsigned long long *>(A.out);
    for (int i = threadIdx.x; i < kMetWords; i += kMetThreads) {
        const unsigned long long v =
            i < kMetRecBase ? S.n[i] : i < kMetBigBase ? S.rec[i - kMetRecBase] : S.big[i - kMetBigBase];
        if (v) atomicAdd(&out[i], v);
    }
}

// one wave per duplex record; records of failing or dropped families get size 0
__global__ __launch_bounds__(256) void k_fmt_size(FmtArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t k = wave; k < 2LL * A.n_fam; k += nw) {
        uint32_t n = 0;
        if (A.fam_fail[k >> 1] == 0 && !(A.fam_filt && (A.fam_filt[k >> 1] & 0xff))) {
            Rec r;
            rec_setup(A, (int32_t)k, r);
            n = rec_size(A, r);
        }
        if (lane_id() == 0) A.rec_size[k] = n;
    }
}

__global__ __launch_bounds__(256) void k_fmt_write(FmtArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t k = wave; k < 2LL * A.n_fam; k += nw) {
        const int64_t o = A.rec_off[k], n = A.rec_off[k + 1] - o;
        if (n == 0) continue;
        Rec r;
        rec_setup(A, (int32_t)k, r);
        rec_write(A, r, A.stream + o, (uint32_t)n);
    }
}

// ---- the single-strand records (dcr_submit_write_ss): record s = 4f + k is
// what make_consensus_read(method="single_strand") returns for subfamily k
// (A1 B2 B1 A2) of family f (:1352-1384): read0's flag, no mate fields, tags
// MI RX sQ sd sD sM se sE (add_tags :1054-1073).  The layout is
// dcr_format.cpp's format_record_ss.
struct RecSs {
    int32_t s, L, nc, tid, pos, mapq, r0, r1, nde;
    int64_t ro;
    const char *code, *mi, *rx;
    uint32_t lc, lmi, lrx;
};

__device__ void rec_setup_ss(const FmtSsArgs &A, int32_t s, RecSs &r) {
    const int32_t f = s >> 2;
    r.s = s;
    r.L = A.ss.len[s];
    r.nc = A.ss.n_cig[s];
    r.tid = A.fam_tid[f];
    r.pos = A.ss.pos[s];
    r.mapq = A.ss.mapq[s];
    r.nde = A.ss.n_de[s];
    r.ro = A.ss_col_off[s];
    r.r0 = A.sub_off[s];
    r.r1 = A.sub_off[s + 1];
    r.code = A.names + A.fam_code[f];
    r.mi = A.names + A.sub_mi[s];
    r.rx = A.names + A.sub_rx[s];
    r.lc = dstrlen(r.code);
    r.lmi = dstrlen(r.mi);
    r.lrx = dstrlen(r.rx);
}

__device__ uint32_t rec_size_ss(const FmtSsArgs &A, const RecSs &r) {
    const dcr_out &ss = A.ss;
    uint32_t n = 36 + 16 + r.lc + 3 + 1 + 4u * (uint32_t)r.nc + (uint32_t)((r.L + 1) >> 1) + (uint32_t)r.L;
    n += 3 + r.lmi + 1 + 3 + r.lrx + 1;                      // MI, RX
    n += 8 + (uint32_t)(r.r1 - r.r0);                        // sQ
    n += 6 + list_body(ss.d + r.ro, r.nde) + 6 + list_body(ss.e + r.ro, r.nde);
    n += int_tag_bytes(ss.D[r.s]) + int_tag_bytes(ss.M[r.s]) + 7;
    return n;
}

__device__ void rec_write_ss(const FmtSsArgs &A, const RecSs &r, uint8_t *o, uint32_t total) {
    const dcr_out &ss = A.ss;
    Out w{o, 0};
    w.u32(total - 4);
    w.u32((uint32_t)r.tid);
    w.u32((uint32_t)r.pos);
    w.b1(16 + r.lc + 3 + 1);
    w.b1((uint32_t)(r.mapq & 0xff));
    const uint32_t *cg = ss.cigar + r.ro;
    int64_t rl = 0;
    if (lane_id() == 0)
        for (int32_t i = 0; i < r.nc; ++i) {
            const uint32_t op = cg[i] & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[i] >> 4;
        }
    w.u16(r.pos >= 0 ? (uint32_t)reg2bin(r.pos, r.pos + (rl > 0 ? rl : 1)) : 4680u);
    w.u16((uint32_t)r.nc);
    w.u16(A.sub_flag[r.s]);
    w.u32((uint32_t)r.L);
    w.u32(0xffffffffu);
    w.u32(0xffffffffu);
    w.u32(0);
    w.str("consensus_family", 16);
    w.str(r.code, r.lc);
    const int k = r.s & 3;
    w.str(k == 0 ? "_A1" : k == 1 ? "_B2" : k == 2 ? "_B1" : "_A2", 3);
    w.b1(0);
    for (int32_t i = lane_id(); i < r.nc; i += kW) {
        const uint32_t v = cg[i];
        for (int b = 0; b < 4; ++b) o[w.p + 4 * i + b] = (uint8_t)(v >> (8 * b));
    }
    w.p += 4u * (uint32_t)r.nc;
    const uint8_t *sq = ss.seq + r.ro;
    const int32_t nb = (r.L + 1) >> 1;
    for (int32_t i = lane_id(); i < nb; i += kW) {
        const uint8_t hi = nt_code(sq[2 * i]);
        const uint8_t lo = (2 * i + 1 < r.L) ? nt_code(sq[2 * i + 1]) : 0;
        o[w.p + i] = (uint8_t)((hi << 4) | lo);
    }
    w.p += (uint32_t)nb;
    w.bytes(ss.qual + r.ro, (uint32_t)r.L);
    w.tag('M', 'I', 'Z');
    w.str(r.mi, r.lmi);
    w.b1(0);
    w.tag('R', 'X', 'Z');
    w.str(r.rx, r.lrx);
    w.b1(0);
    w.tag('s', 'Q', 'B'); w.b1('C'); w.u32((uint32_t)(r.r1 - r.r0)); w.bytes(A.read_mapq + r.r0, (uint32_t)(r.r1 - r.r0));
    w.list('s', 'd', ss.d + r.ro, r.nde);
    w.int_tag('s', 'D', ss.D[r.s]);
    w.int_tag('s', 'M', ss.M[r.s]);
    w.list('s', 'e', ss.e + r.ro, r.nde);
    w.float_tag('s', 'E', ss.E[r.s]);
}

// one wave per single-strand record; records of failing families get size 0
__global__ __launch_bounds__(256) void k_fmt_size_ss(FmtSsArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t s = wave; s < 4LL * A.n_fam; s += nw) {
        uint32_t n = 0;
        if (A.fam_fail[s >> 2] == 0 && !(A.fam_filt && (A.fam_filt[s >> 2] & 0xff))) {
            RecSs r;
            rec_setup_ss(A, (int32_t)s, r);
            n = rec_size_ss(A, r);
        }
        if (lane_id() == 0) A.rec_size[s] = n;
    }
}

__global__ __launch_bounds__(256) void k_fmt_write_ss(FmtSsArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t s = wave; s < 4LL * A.n_fam; s += nw) {
        const int64_t o = A.rec_off[s], n = A.rec_off[s + 1] - o;
        if (n == 0) continue;
        RecSs r;
        rec_setup_ss(A, (int32_t)s, r);
        rec_write_ss(A, r, A.stream + o, (uint32_t)n);
    }
}

// ---- the per-base tags (dcr_set_base_tags; include/dcr.h states them).  The
// six depth / error tags become B:s arrays and the four strand strings Z
// strings of the record's own length, one value per base of SEQ, so the sizes
// follow from len alone and the size kernels read no map.  The write kernels
// are one wave per record like k_fmt_write[_ss]: the head through cQ / sQ is
// rec_head[_ss]; then every lane finds the columns and source bases of its own
// base once, as k_base_filter does (bf_rec, bf_own_col, bf_sources, the single
// M run shortcut, the stored maps of the records that have them), and stores
// its element of every tag, whose offsets inside the record are known up
// front.  Records start at any byte offset: the 16-bit elements go out as two
// byte stores.  No LDS.  Every index is clamped to its region (bf_rec), and a
// base at or past the clamped length gets the absent-strand values.
constexpr uint32_t kTagArr = 8;     // tag, 'B', 's', count
constexpr uint32_t kTagStr = 4;     // tag, 'Z', NUL

__device__ __forceinline__ uint32_t tags_size(int32_t L) {
    return 6 * (kTagArr + 2u * (uint32_t)L) + 4 * (kTagStr + (uint32_t)L);
}

__device__ uint32_t rec_size_tags(const FmtArgs &A, const Rec &r) {
    const dcr_out &ss = A.ss, &ds = A.ds;
    uint32_t n = 36 + 16 + r.lc + 12 + 1 + 4u * (uint32_t)r.nc + (uint32_t)((r.L + 1) >> 1) + (uint32_t)r.L;
    n += 3 + r.lc + 1 + 3 + r.lr + 1;                                  // MI, RX
    n += 8 + (uint32_t)(r.a1 - r.a0) + 8 + (uint32_t)(r.b1 - r.b0) + 8 + 2;   // aQ bQ cQ
    n += int_tag_bytes(ss.D[r.a]) + int_tag_bytes(ss.D[r.b]) + int_tag_bytes(ds.D[r.k]);
    n += int_tag_bytes(ss.M[r.a]) + int_tag_bytes(ss.M[r.b]) + int_tag_bytes(ds.M[r.k]);
    n += 3 * 7;
    return n + tags_size(r.L);
}

// t5 of a record without a stored map: pos - the smallest start of its reads (k_base_filter's wave minimum)
__device__ int64_t tag_t5(const int32_t *sub_off, const int32_t *read_pos, int64_t s, int64_t pos) {
    const int32_t r0 = sub_off[s], r1 = sub_off[s + 1];
    int32_t mp = 0x7fffffff;
    for (int32_t r = r0 + lane_id(); r < r1; r += kW) mp = read_pos[r] < mp ? read_pos[r] : mp;
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        const int32_t o = __shfl_xor(mp, dd, kW);
        mp = o < mp ? o : mp;
    }
    return r1 > r0 ? pos - (int64_t)mp : 0;
}

// the head of a B:s array of n elements / of a Z string of n characters (and its NUL): returns where
// the elements start and leaves the writer after the tag
__device__ __forceinline__ uint32_t tag_arr(Out &w, char a, char b, uint32_t n) {
    w.tag(a, b, 'B');
    w.b1('s');
    w.u32(n);
    const uint32_t at = w.p;
    w.p += 2 * n;
    return at;
}
__device__ __forceinline__ uint32_t tag_str(Out &w, char a, char b, uint32_t n) {
    w.tag(a, b, 'Z');
    const uint32_t at = w.p;
    w.p += n;
    w.b1(0);
    return at;
}
__device__ __forceinline__ void put_s(uint8_t *o, uint32_t at, int64_t i, uint32_t v) {
    v = v > 32767u ? 32767u : v;
    o[at + 2 * i] = (uint8_t)v;
    o[at + 2 * i + 1] = (uint8_t)(v >> 8);
}

// The records up to and including cQ / sQ, as rec_write / rec_write_ss write
// them.  Copies, not shared code: the default kernels compile to the parent's
// instructions only while their own functions stay as they are.
__device__ void rec_head(const FmtArgs &A, const Rec &r, Out &w, uint32_t total) {
    const dcr_out &ss = A.ss, &ds = A.ds;
    uint8_t *o = w.o;
    w.u32(total - 4);
    w.u32((uint32_t)r.tid);
    w.u32((uint32_t)r.pos);
    w.b1(16 + r.lc + 12 + 1);
    w.b1((uint32_t)(r.mapq & 0xff));
    const uint32_t *cg = ds.cigar + r.ro;
    int64_t rl = 0;
    if (lane_id() == 0)
        for (int32_t i = 0; i < r.nc; ++i) {
            const uint32_t op = cg[i] & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[i] >> 4;
        }
    w.u16(r.pos >= 0 ? (uint32_t)reg2bin(r.pos, r.pos + (rl > 0 ? rl : 1)) : 4680u);
    w.u16((uint32_t)r.nc);
    w.u16(r.j == 0 ? 99u : 147u);
    w.u32((uint32_t)r.L);
    w.u32((uint32_t)r.tid);
    w.u32((uint32_t)r.opos);
    w.u32((uint32_t)r.tlen);
    w.str("consensus_family", 16);
    w.str(r.code, r.lc);
    w.str(r.j == 0 ? "_paired-end1" : "_paired-end2", 12);
    w.b1(0);
    for (int32_t i = lane_id(); i < r.nc; i += kW) {
        const uint32_t v = cg[i];
        for (int b = 0; b < 4; ++b) o[w.p + 4 * i + b] = (uint8_t)(v >> (8 * b));
    }
    w.p += 4u * (uint32_t)r.nc;
    const uint8_t *sq = ds.seq + r.ro;
    const int32_t nb = (r.L + 1) >> 1;
    for (int32_t i = lane_id(); i < nb; i += kW) {
        const uint8_t hi = nt_code(sq[2 * i]);
        const uint8_t lo = (2 * i + 1 < r.L) ? nt_code(sq[2 * i + 1]) : 0;
        o[w.p + i] = (uint8_t)((hi << 4) | lo);
    }
    w.p += (uint32_t)nb;
    w.bytes(ds.qual + r.ro, (uint32_t)r.L);
    w.tag('M', 'I', 'Z');
    w.str(r.code, r.lc);
    w.b1(0);
    w.tag('R', 'X', 'Z');
    w.str(r.rx, r.lr);
    w.b1(0);
    w.tag('a', 'Q', 'B'); w.b1('C'); w.u32((uint32_t)(r.a1 - r.a0)); w.bytes(A.read_mapq + r.a0, (uint32_t)(r.a1 - r.a0));
    w.tag('b', 'Q', 'B'); w.b1('C'); w.u32((uint32_t)(r.b1 - r.b0)); w.bytes(A.read_mapq + r.b0, (uint32_t)(r.b1 - r.b0));
    w.tag('c', 'Q', 'B'); w.b1('C'); w.u32(2); w.b1((uint32_t)ss.mapq[r.a] & 0xff); w.b1((uint32_t)ss.mapq[r.b] & 0xff);
}

__device__ void rec_head_ss(const FmtSsArgs &A, const RecSs &r, Out &w, uint32_t total) {
    const dcr_out &ss = A.ss;
    uint8_t *o = w.o;
    w.u32(total - 4);
    w.u32((uint32_t)r.tid);
    w.u32((uint32_t)r.pos);
    w.b1(16 + r.lc + 3 + 1);
    w.b1((uint32_t)(r.mapq & 0xff));
    const uint32_t *cg = ss.cigar + r.ro;
    int64_t rl = 0;
    if (lane_id() == 0)
        for (int32_t i = 0; i < r.nc; ++i) {
            const uint32_t op = cg[i] & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[i] >> 4;
        }
    w.u16(r.pos >= 0 ? (uint32_t)reg2bin(r.pos, r.pos + (rl > 0 ? rl : 1)) : 4680u);
    w.u16((uint32_t)r.nc);
    w.u16(A.sub_flag[r.s]);
    w.u32((uint32_t)r.L);
    w.u32(0xffffffffu);
    w.u32(0xffffffffu);
    w.u32(0);
    w.str("consensus_family", 16);
    w.str(r.code, r.lc);
    const int k = r.s & 3;
    w.str(k == 0 ? "_A1" : k == 1 ? "_B2" : k == 2 ? "_B1" : "_A2", 3);
    w.b1(0);
    for (int32_t i = lane_id(); i < r.nc; i += kW) {
        const uint32_t v = cg[i];
        for (int b = 0; b < 4; ++b) o[w.p + 4 * i + b] = (uint8_t)(v >> (8 * b));
    }
    w.p += 4u * (uint32_t)r.nc;
    const uint8_t *sq = ss.seq + r.ro;
    const int32_t nb = (r.L + 1) >> 1;
    for (int32_t i = lane_id(); i < nb; i += kW) {
        const uint8_t hi = nt_code(sq[2 * i]);
        const uint8_t lo = (2 * i + 1 < r.L) ? nt_code(sq[2 * i + 1]) : 0;
        o[w.p + i] = (uint8_t)((hi << 4) | lo);
    }
    w.p += (uint32_t)nb;
    w.bytes(ss.qual + r.ro, (uint32_t)r.L);
    w.tag('M', 'I', 'Z');
    w.str(r.mi, r.lmi);
    w.b1(0);
    w.tag('R', 'X', 'Z');
    w.str(r.rx, r.lrx);
    w.b1(0);
    w.tag('s', 'Q', 'B'); w.b1('C'); w.u32((uint32_t)(r.r1 - r.r0)); w.bytes(A.read_mapq + r.r0, (uint32_t)(r.r1 - r.r0));
}

__device__ void rec_write_tags(const FmtTagArgs &T, const Rec &r, uint8_t *o, uint32_t total) {
    const FmtArgs &A = T.f;
    const dcr_out &ss = A.ss, &ds = A.ds;
    Out w{o, 0};
    rec_head(A, r, w, total);
    const uint32_t L = (uint32_t)r.L;
    const uint32_t ad = tag_arr(w, 'a', 'd', L), bd = tag_arr(w, 'b', 'd', L), cd = tag_arr(w, 'c', 'd', L);
    w.int_tag('a', 'D', ss.D[r.a]); w.int_tag('b', 'D', ss.D[r.b]); w.int_tag('c', 'D', ds.D[r.k]);
    w.int_tag('a', 'M', ss.M[r.a]); w.int_tag('b', 'M', ss.M[r.b]); w.int_tag('c', 'M', ds.M[r.k]);
    const uint32_t ae = tag_arr(w, 'a', 'e', L), be = tag_arr(w, 'b', 'e', L), ce = tag_arr(w, 'c', 'e', L);
    w.float_tag('a', 'E', ss.E[r.a]); w.float_tag('b', 'E', ss.E[r.b]); w.float_tag('c', 'E', ds.E[r.k]);
    const uint32_t ac = tag_str(w, 'a', 'c', L), bc = tag_str(w, 'b', 'c', L);
    const uint32_t aq = tag_str(w, 'a', 'q', L), bq = tag_str(w, 'b', 'q', L);
    // the maps of the three records, as k_base_filter sets them up
    BfRec S[2], R;
    for (int s = 0; s < 2; ++s) {
        bf_rec(ss, A.ss_col_off, r.a + s, T.ss_col, T.flag[r.a + s] != 0, S[s]);
        if (!S[s].mapped) S[s].t5 = tag_t5(A.sub_off, T.read_pos, r.a + s, S[s].pos);
    }
    bf_rec(ds, A.ds_col_off, r.k, T.ds_col, T.flag[4 * (int64_t)A.n_fam + r.k] != 0, R);
    const int64_t minpos = S[0].pos < S[1].pos ? S[0].pos : S[1].pos;
    R.t5 = R.pos - minpos;
    const uint32_t *aln = T.ds_aln + r.ro;
    const bool lane_math = R.simple && S[0].simple && S[1].simple;
    const uint8_t *sq[2] = {ss.seq + r.ao, ss.seq + r.bo}, *ql[2] = {ss.qual + r.ao, ss.qual + r.bo};
    const uint32_t at_d[2] = {ad, bd}, at_e[2] = {ae, be}, at_c[2] = {ac, bc}, at_q[2] = {aq, bq};
    for (int64_t i = lane_id(); i < (int64_t)L; i += kW) {
        int64_t c = -1, ix[2] = {-1, -1};       // the duplex d-index, the strands' base indices (-1: none)
        if (i < R.len) {
            if (lane_math) {
                c = R.t5 + i;
                for (int s = 0; s < 2; ++s) {
                    const int64_t b = minpos + c - S[s].pos;
                    ix[s] = b >= 0 && b < S[s].len ? b : -1;
                }
            } else {
                int64_t t;
                if (R.mapped) {
                    c = (int64_t)R.col[i];
                    t = (int64_t)aln[i];
                } else {
                    c = t = bf_own_col(R, i);   // no '+' column: the d-index is the alignment column
                }
                bf_sources(S[0], S[1], minpos, t, ix[0], ix[1]);
            }
        }
        for (int s = 0; s < 2; ++s) {
            const int64_t cs = bf_own_col(S[s], ix[s]);
            const bool v = cs >= 0 && cs < S[s].nde;
            put_s(o, at_d[s], i, v ? S[s].d[cs] : 0u);
            put_s(o, at_e[s], i, v ? S[s].e[cs] : 0u);
            o[at_c[s] + i] = ix[s] >= 0 ? sq[s][ix[s]] : (uint8_t)'N';
            o[at_q[s] + i] = ix[s] >= 0 ? (uint8_t)(ql[s][ix[s]] + 33) : (uint8_t)'!';
        }
        const bool vc = c >= 0 && c < R.nde;
        put_s(o, cd, i, vc ? R.d[c] : 0u);
        put_s(o, ce, i, vc ? R.e[c] : 0u);
    }
}

// one wave per duplex record, as k_fmt_size
__global__ __launch_bounds__(256) void k_fmt_size_tags(FmtArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t k = wave; k < 2LL * A.n_fam; k += nw) {
        uint32_t n = 0;
        if (A.fam_fail[k >> 1] == 0 && !(A.fam_filt && (A.fam_filt[k >> 1] & 0xff))) {
            Rec r;
            rec_setup(A, (int32_t)k, r);
            n = rec_size_tags(A, r);
        }
        if (lane_id() == 0) A.rec_size[k] = n;
    }
}

__global__ __launch_bounds__(256) void k_fmt_write_tags(FmtTagArgs T) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t k = wave; k < 2LL * T.f.n_fam; k += nw) {
        const int64_t o = T.f.rec_off[k], n = T.f.rec_off[k + 1] - o;
        if (n == 0) continue;
        Rec r;
        rec_setup(T.f, (int32_t)k, r);
        rec_write_tags(T, r, T.f.stream + o, (uint32_t)n);
    }
}

// the single-strand records: sd / se per base from the record's own columns (Level 1)
__device__ uint32_t rec_size_ss_tags(const FmtSsArgs &A, const RecSs &r) {
    const dcr_out &ss = A.ss;
    uint32_t n = 36 + 16 + r.lc + 3 + 1 + 4u * (uint32_t)r.nc + (uint32_t)((r.L + 1) >> 1) + (uint32_t)r.L;
    n += 3 + r.lmi + 1 + 3 + r.lrx + 1;                      // MI, RX
    n += 8 + (uint32_t)(r.r1 - r.r0);                        // sQ
    n += 2 * (kTagArr + 2u * (uint32_t)r.L);                 // sd, se
    n += int_tag_bytes(ss.D[r.s]) + int_tag_bytes(ss.M[r.s]) + 7;
    return n;
}

__device__ void rec_write_ss_tags(const FmtSsTagArgs &T, const RecSs &r, uint8_t *o, uint32_t total) {
    const FmtSsArgs &A = T.f;
    const dcr_out &ss = A.ss;
    Out w{o, 0};
    rec_head_ss(A, r, w, total);
    const uint32_t L = (uint32_t)r.L;
    const uint32_t sd = tag_arr(w, 's', 'd', L);
    w.int_tag('s', 'D', ss.D[r.s]);
    w.int_tag('s', 'M', ss.M[r.s]);
    const uint32_t se = tag_arr(w, 's', 'e', L);
    w.float_tag('s', 'E', ss.E[r.s]);
    BfRec S;
    bf_rec(ss, A.ss_col_off, r.s, T.ss_col, T.flag[r.s] != 0, S);
    if (!S.mapped) S.t5 = tag_t5(A.sub_off, T.read_pos, r.s, S.pos);
    for (int64_t i = lane_id(); i < (int64_t)L; i += kW) {
        const int64_t c = bf_own_col(S, i);
        const bool v = c >= 0 && c < S.nde;
        put_s(o, sd, i, v ? S.d[c] : 0u);
        put_s(o, se, i, v ? S.e[c] : 0u);
    }
}

__global__ __launch_bounds__(256) void k_fmt_size_ss_tags(FmtSsArgs A) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t s = wave; s < 4LL * A.n_fam; s += nw) {
        uint32_t n = 0;
        if (A.fam_fail[s >> 2] == 0 && !(A.fam_filt && (A.fam_filt[s >> 2] & 0xff))) {
            RecSs r;
            rec_setup_ss(A, (int32_t)s, r);
            n = rec_size_ss_tags(A, r);
        }
        if (lane_id() == 0) A.rec_size[s] = n;
    }
}

__global__ __launch_bounds__(256) void k_fmt_write_ss_tags(FmtSsTagArgs T) {
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kW;
    const int64_t nw = (int64_t)gridDim.x * blockDim.x / kW;
    for (int64_t s = wave; s < 4LL * T.f.n_fam; s += nw) {
        const int64_t o = T.f.rec_off[s], n = T.f.rec_off[s + 1] - o;
        if (n == 0) continue;
        RecSs r;
        rec_setup_ss(T.f, (int32_t)s, r);
        rec_write_ss_tags(T, r, T.f.stream + o, (uint32_t)n);
    }
}

// ---- the per-base duplex QC tables (dcr_set_base_metrics; include/dcr.h
// states them).  One wave per duplex record, 64 bases at a time; every lane
// finds the columns and source bases of its own base exactly as
// rec_write_tags does (bf_rec, tag_t5, the single M run shortcut, the stored
// maps of the records that have them, else bf_own_col + bf_sources) and then
// counts instead of storing.  Nothing per base goes to HBM (a same-address
// device atomic costs about 30 ns serialised; a batch has millions of bases in
// a few hundred bins).  Three levels, in the shape of k_metrics:
//   wave    the loop over a record is uniform (every lane stays in it, the
//           ones past the end inactive), so the scalars n[] are popcounts of
//           ballots kept in scalar registers, and for pair, depth, err and
//           qual the lanes that share the first active lane's bin (the hot
//           bin: most bases agree at one quality, one depth pair and err[0])
//           are added by one lane with one LDS add (bm_count); the other
//           lanes add their own.  The cycle bins of 64 consecutive bases are
//           64 different addresses; a whole step past bin 511 is summed over
//           the wave and added once;
//   LDS     the workgroup's copy of dcr_base_metrics: 32-bit for the count
//           tables, 64-bit for n[] and the two sums of cyc (what 4, 5);
//   HBM     at the end one global 64-bit add per non-zero bin per workgroup.
// No counter wraps: every 32-bit LDS bin takes at most 1 per base, and a
// launch covers families [f0, f1) whose duplex regions hold fewer than 2^32
// columns (len is clamped to the region; the host splits a larger batch into
// several launches, which is the bounded flush); the sums are 64-bit, a
// step's wave sum of s or e is at most 64 * 2 * 65535; n[] is 64-bit.
// Every index is clamped to its region (bf_rec).
constexpr int kBmWords = (int)(sizeof(dcr_base_metrics) / 8);
constexpr int kBmPair = (int)(offsetof(dcr_base_metrics, pair) / 8);
constexpr int kBmDepth = (int)(offsetof(dcr_base_metrics, depth) / 8) - kBmPair;
constexpr int kBmErr = (int)(offsetof(dcr_base_metrics, err) / 8) - kBmPair;
constexpr int kBmQual = (int)(offsetof(dcr_base_metrics, qual) / 8) - kBmPair;
constexpr int kBmCyc = (int)(offsetof(dcr_base_metrics, cyc) / 8);
static_assert(sizeof(dcr_base_metrics) % 8 == 0 && offsetof(dcr_base_metrics, n) == 0 && kBmPair == 8 &&
                  kBmWords == kBmCyc + 2 * 6 * DCR_BMET_CYC_BINS,
              "k_base_metrics' LDS layout follows dcr_base_metrics");

struct BmShared {
    unsigned long long n[8];
    unsigned long long sum[2][2][DCR_BMET_CYC_BINS];    // cyc what 4, 5
    uint32_t cnt[kBmCyc - kBmPair];                     // pair, depth, err, qual
    uint32_t cyc[2][4][DCR_BMET_CYC_BINS];              // cyc what 0 .. 3
};

__device__ __forceinline__ int bm_code(uint8_t c) {
    switch (c | 0x20) {
        case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': return 3;
        default: return 4;
    }
}

// +1 into h[bin] for the lanes with act (every lane of the wave calls): the lanes that share the
// first such lane's bin are added by one lane
__device__ __forceinline__ void bm_count(uint32_t *h, int bin, bool act) {
    const unsigned long long ma = __ballot(act);
    if (ma == 0) return;
    const int b0 = __shfl(bin, (int)__builtin_ctzll(ma), kW);
    const bool hot = act && bin == b0;
    const unsigned long long mh = __ballot(hot);
    if (hot) {
        if (lane_id() == (int)__builtin_ctzll(mh)) atomicAdd(&h[b0], (uint32_t)__builtin_popcountll(mh));
    } else if (act) {
        atomicAdd(&h[bin], 1u);
    }
}

__device__ __forceinline__ unsigned long long bm_pop(bool p) {
    return (unsigned long long)__builtin_popcountll(__ballot(p));
}

// duplex record k: n[] is the wave's own (the same in every lane)
__device__ void bm_record(const BaseMetricsArgs &A, BmShared &Sh, int64_t k, unsigned long long (&n)[8]) {
    const dcr_out &ss = A.ss, &ds = A.ds;
    const int j = (int)(k & 1);
    const int64_t a = 4 * (k >> 1) + 2 * j;
    // the maps of the three records, as rec_write_tags sets them up
    BfRec S[2], R;
    for (int s = 0; s < 2; ++s) {
        bf_rec(ss, A.ss_col_off, a + s, A.ss_col, A.flag[a + s] != 0, S[s]);
        if (!S[s].mapped) S[s].t5 = tag_t5(A.sub_off, A.read_pos, a + s, S[s].pos);
    }
    bf_rec(ds, A.ds_col_off, k, A.ds_col, A.flag[4 * (int64_t)A.n_fam + k] != 0, R);
    const int64_t minpos = S[0].pos < S[1].pos ? S[0].pos : S[1].pos;
    R.t5 = R.pos - minpos;
    const int64_t ro = A.ds_col_off[k];
    const uint32_t *aln = A.ds_aln + ro;
    const bool lane_math = R.simple && S[0].simple && S[1].simple;
    const uint8_t *sq[2] = {ss.seq + A.ss_col_off[a], ss.seq + A.ss_col_off[a + 1]};
    const uint8_t *dsq = ds.seq + ro, *dql = ds.qual + ro;
    const int L = __builtin_amdgcn_readfirstlane((int)R.len);      // len is an int32: the clamped value fits
    n[0] += 1;
    n[1] += (unsigned long long)L;
    for (int i0 = 0; i0 < L; i0 += kW) {
        const int64_t i = (int64_t)i0 + lane_id();
        const bool act = i < (int64_t)L;
        int64_t c = -1, ix[2] = {-1, -1};       // the duplex d-index, the strands' base indices (-1: none)
        if (act) {
            if (lane_math) {
                c = R.t5 + i;
                for (int s = 0; s < 2; ++s) {
                    const int64_t b = minpos + c - S[s].pos;
                    ix[s] = b >= 0 && b < S[s].len ? b : -1;
                }
            } else {
                int64_t t;
                if (R.mapped) {
                    c = (int64_t)R.col[i];
                    t = (int64_t)aln[i];
                } else {
                    c = t = bf_own_col(R, i);   // no '+' column: the d-index is the alignment column
                }
                bf_sources(S[0], S[1], minpos, t, ix[0], ix[1]);
            }
        }
        uint32_t D[2], E[2];
        int code[2];
        for (int s = 0; s < 2; ++s) {
            const int64_t cs = bf_own_col(S[s], ix[s]);
            const bool v = cs >= 0 && cs < S[s].nde;
            D[s] = v ? S[s].d[cs] : 0u;
            E[s] = v ? S[s].e[cs] : 0u;
            code[s] = ix[s] >= 0 ? bm_code(sq[s][ix[s]]) : 4;
        }
        const uint32_t cE = (c >= 0 && c < R.nde) ? R.e[c] : 0u;
        const bool pa = ix[0] >= 0, pb = ix[1] >= 0, both = pa && pb;
        const int cls = both ? (code[0] == code[1] ? 0 : 1) : 2;
        const uint32_t sd = D[0] + D[1], se = E[0] + E[1];
        const uint32_t q = act ? dql[i] : 0u;
        const bool isn = act && dsq[i] == (uint8_t)'N';
        n[2] += bm_pop(act && both);
        n[3] += bm_pop(act && pa && !pb);
        n[4] += bm_pop(act && !pa && pb);
        n[5] += bm_pop(act && !pa && !pb);
        n[6] += bm_pop(act && cls == 1);
        n[7] += bm_pop(act && cE > 0);
        const uint32_t hi = D[0] > D[1] ? D[0] : D[1], lo = D[0] > D[1] ? D[1] : D[0];
        const int dbin = (int)(hi < 63u ? hi : 63u) * DCR_BMET_DEPTH_BINS + (int)(lo < 63u ? lo : 63u);
        // s <= 2 * 65535: 1000 * e fits 32 bits whenever e <= s
        const int ebin = (sd > 0 && se <= sd) ? (se == 0 ? 0 : (int)(1000u * se / sd)) : DCR_BMET_ERR_BINS - 1;
        bm_count(Sh.cnt, j * 25 + code[0] * 5 + code[1], act && both);      // pair comes first
        bm_count(Sh.cnt + kBmDepth, dbin, act);
        bm_count(Sh.cnt + kBmErr, ebin, act);
        bm_count(Sh.cnt + kBmQual, cls * DCR_BMET_QUAL_BINS + (int)q, act);
        // the cycle: i' from the sequencing 5' end
        const int last = i0 + kW - 1 < L - 1 ? i0 + kW - 1 : L - 1;
        const int ip_min = j == 0 ? i0 : L - 1 - last;          // the smallest i' of this step's bases
        if (ip_min >= DCR_BMET_CYC_BINS - 1) {
            const uint32_t c0 = (uint32_t)bm_pop(act), c1 = (uint32_t)bm_pop(isn);
            const uint32_t c2 = (uint32_t)bm_pop(act && cls == 1), c3 = (uint32_t)bm_pop(act && cls == 2);
            const uint32_t ws = wave_sum(act ? sd : 0u), we = wave_sum(act ? se : 0u);
            if (lane_id() == 0) {
                const int b = DCR_BMET_CYC_BINS - 1;
                atomicAdd(&Sh.cyc[j][0][b], c0);
                if (c1) atomicAdd(&Sh.cyc[j][1][b], c1);
                if (c2) atomicAdd(&Sh.cyc[j][2][b], c2);
                if (c3) atomicAdd(&Sh.cyc[j][3][b], c3);
                if (ws) atomicAdd(&Sh.sum[j][0][b], (unsigned long long)ws);
                if (we) atomicAdd(&Sh.sum[j][1][b], (unsigned long long)we);
            }
        } else if (act) {
            const int ip = j == 0 ? (int)i : L - 1 - (int)i;
            const int b = ip < DCR_BMET_CYC_BINS - 1 ? ip : DCR_BMET_CYC_BINS - 1;
            atomicAdd(&Sh.cyc[j][0][b], 1u);
            if (isn) atomicAdd(&Sh.cyc[j][1][b], 1u);
            if (cls == 1) atomicAdd(&Sh.cyc[j][2][b], 1u);
            if (cls == 2) atomicAdd(&Sh.cyc[j][3][b], 1u);
            if (sd) atomicAdd(&Sh.sum[j][0][b], (unsigned long long)sd);
            if (se) atomicAdd(&Sh.sum[j][1][b], (unsigned long long)se);
        }
    }
}

__global__ __launch_bounds__(kBmThreads) void k_base_metrics(BaseMetricsArgs A) {
    __shared__ BmShared S;
    for (int i = threadIdx.x; i < (int)(sizeof(BmShared) / 4); i += kBmThreads) reinterpret_cast<uint32_t *>(&S)[i] = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kBmThreads + threadIdx.x) / kW));
    const int nw = (int)(gridDim.x * (kBmThreads / kW));
    unsigned long long n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t k = 2 * (int64_t)A.f0 + wave; k < 2 * (int64_t)A.f1; k += nw) {
        if (A.fam_fail[k >> 1] != 0) continue;
        bm_record(A, S, k, n);
    }
    if (lane_id() == 0)
        for (int t = 0; t < 8; ++t)
            if (n[t]) atomicAdd(&S.n[t], n[t]);
    __syncthreads();
    // the workgroup's tables into the slot's: one 64-bit add per non-zero bin
    unsigned long long *out = reinterpret_cast<unsigned long long *>(A.out);
    for (int w = threadIdx.x; w < kBmWords; w += kBmThreads) {
        unsigned long long v;
        if (w < kBmPair) {
            v = S.n[w];
        } else if (w < kBmCyc) {
            v = S.cnt[w - kBmPair];
        } else {
            const int t = w - kBmCyc, jj = t / (6 * DCR_BMET_CYC_BINS), what = t / DCR_BMET_CYC_BINS % 6;
            const int b = t % DCR_BMET_CYC_BINS;
            v = what < 4 ? (unsigned long long)S.cyc[jj][what][b] : S.sum[jj][what - 4][b];
        }
        if (v) atomicAdd(&out[w], v);
    }
}

// the reference's outcome per family, in its execution order (dcr_fmt_scan)
__global__ __launch_bounds__(256) void k_famfail(FmtArgs A) {
    const int32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= A.n_fam) return;
    int32_t kind = 0, which = -1;
    // preprocessing of every read comes first (:1272-1283): the first
    // subfamily holding a failing read (DCR_ST_PREP | its status)
    for (int k = 0; k < 4 && !kind; ++k) {
        const int st = A.ss.status[4 * f + k];
        if (st & DCR_ST_PREP) { kind = st & 15; which = 8 + k; }
    }
    auto st_fail = [](int st) { return st != 0 && st != DCR_ST_UPSTREAM; };
    for (int k = 0; k < 4 && !kind; ++k) {
        const int st = A.ss.status[4 * f + k];
        if (st_fail(st)) { kind = st; which = k; }
    }
    for (int j = 0; j < 2 && !kind; ++j) {
        const int st = A.ds.status[2 * f + j];
        if (st_fail(st)) { kind = st; which = 4 + j; break; }
        for (int s = 4 * f + 2 * j; s < 4 * f + 2 * j + 2 && !kind; ++s) {
            const int64_t o = A.ss_col_off[s];
            for (int32_t i = 0; i < A.ss.len[s]; ++i)
                if (A.ss.qual[o + i] >= 95) { kind = 7; which = 4 + j; break; }   // pysam force_bytes(ascii)
        }
    }
    A.fam_fail[f] = kind ? (kind | (which << 8)) : 0;
    A.ds_len_out[2 * f] = A.ds.len[2 * f];
    A.ds_len_out[2 * f + 1] = A.ds.len[2 * f + 1];
}

// dfl::p4_scan across the workgroup: wave scans of the lanes' bit counts,
// xor of their CRC registers; zeroes the words two lanes share (not of a
// block that will be stored: every lane has the total after the barrier)
__device__ __forceinline__ void p4_scan_wg(dfl::Shared &s, uint32_t n, int lane, uint32_t *slot) {
    const uint32_t b = s.lane_bits[lane];
    const uint32_t inc = wave_incl_scan(b);
    uint32_t cx = s.lane_crc[lane];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cx ^= __shfl_xor(cx, d, kW);
    const int w = lane >> 6;
    if ((lane & (kW - 1)) == kW - 1) s.wave_sum[w] = inc;
    if ((lane & (kW - 1)) == 0) s.wave_crc[w] = cx;
    __syncthreads();
    uint32_t base = 3 * 8 * 6 + s.hdr_bits, end = base;
    for (int k = 0; k < w; ++k) base += s.wave_sum[k];
    for (int k = 0; k < dfl::kT / kW; ++k) end += s.wave_sum[k];
    const uint32_t off = base + inc - b;
    s.lane_off[lane] = off;
    if (lane && (off & 31) && !dfl::will_store(s, n, end)) {
        slot[off >> 5] = 0;
        if ((off >> 5) < sizeof(s.stage) / 4) s.stage[off >> 5] = 0;
    }
    if (lane == dfl::kT - 1) {
        dfl::decide(s, n, off + b);
        uint32_t c = dfl::multmodp(dfl::x8nmodp(n), 0xffffffffu);
        for (int k = 0; k < dfl::kT / kW; ++k) c ^= s.wave_crc[k];
        s.crc = ~c;
    }
}

// dfl::p3c_header on wave 0 (lanes 0..63): the same greedy run-length
// code of the code lengths, built in parallel.  Runs start where a length
// differs from the one before it (ballots over five chunks of 64 positions);
// each run's lane counts its symbols, an exclusive scan in run order gives
// its offset in rle[], and it writes them; the symbol counts go in by LDS
// atomics.  Lane 0 then finishes as the serial code does (p3c_header_post).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void p3c_header_wave(dfl::Shared &s, int lane) {
    const uint32_t last_lit = s.last_lit, last_dist = s.last_dist;
    const int nlit = last_lit + 1 > 257 ? (int)last_lit + 1 : 257;
    const int ndist = (int)last_dist + 1;
    const int N = nlit + ndist;                       // <= 316: five chunks
    auto L = [&](int i) -> uint32_t { return i < nlit ? s.lit_len[i] : s.dist_len[i - nlit]; };
    uint32_t *clf = s.t0_clf;
    if (lane < 19) clf[lane] = 0;
    if (lane == 0) {
        dfl::first_codes_from_counts(s.num_lit, s.next_code[0]);
        dfl::first_codes_from_counts(s.num_dist, s.next_code[1]);
        s.hlit = (uint32_t)(nlit - 257);
        s.hdist = (uint32_t)(ndist - 1);
    }
    constexpr int kC = 5;
    uint32_t v[kC];
    uint64_t st[kC];                                  // run starts per chunk (uniform)
#pragma unroll
    for (int c = 0; c < kC; ++c) {
        const int i = 64 * c + lane;
        v[c] = i < N ? L(i) : 0xffu;
        const uint32_t pv = (i > 0 && i <= N) ? L(i - 1) : 0xfeu;
        st[c] = __ballot(i < N && v[c] != pv);
    }
    wave_lds_sync();                                  // clf zeroed before the atomics
    uint32_t base = 0;
#pragma unroll
    for (int c = 0; c < kC; ++c) {
        const int i = 64 * c + lane;
        const bool start = (st[c] >> lane) & 1u;
        // the next run start after i: in this chunk above the lane, else in a later chunk, else N
        int nxt = N;
        const uint64_t above = lane == 63 ? 0ull : st[c] & (~0ull << (lane + 1));
        if (above) nxt = 64 * c + (int)__builtin_ctzll(above);
        else {
#pragma unroll
            for (int d = kC - 1; d > c; --d)
                if (st[d]) nxt = 64 * d + (int)__builtin_ctzll(st[d]);
        }
        int run = nxt - i;
        uint32_t ns = 0, n18 = 0, n17 = 0, n16 = 0, nv = 0;
        const uint32_t val = v[c];
        if (start) {
            int r = run;
            if (val == 0) {
                while (r >= 11) { r -= r < 138 ? r : 138; ++n18; }
                if (r >= 3) { ++n17; r = 0; }
                nv = (uint32_t)r;
                ns = n18 + n17 + nv;
            } else {
                --r;
                nv = 1;
                while (r >= 3) { r -= r < 6 ? r : 6; ++n16; }
                nv += (uint32_t)r;
                ns = 1 + n16 + (uint32_t)r;
            }
        }
        const uint32_t inc = wave_incl_scan(ns);
        uint32_t off = base + inc - ns;
        base += __shfl(inc, 63, kW);
        if (start) {
            int r = run;
            if (val == 0) {
                while (r >= 11) { const int t = r < 138 ? r : 138; s.rle[off++] = (uint16_t)(18 | ((t - 11) << 8)); r -= t; }
                if (r >= 3) { s.rle[off++] = (uint16_t)(17 | ((r - 3) << 8)); r = 0; }
                while (r-- > 0) s.rle[off++] = 0;
            } else {
                s.rle[off++] = (uint16_t)val;
                --r;
                while (r >= 3) { const int t = r < 6 ? r : 6; s.rle[off++] = (uint16_t)(16 | ((t - 3) << 8)); r -= t; }
                while (r-- > 0) s.rle[off++] = (uint16_t)val;
            }
            if (n18) atomicAdd(&clf[18], n18);
            if (n17) atomicAdd(&clf[17], n17);
            if (n16) atomicAdd(&clf[16], n16);
            if (nv) atomicAdd(&clf[val], nv);
        }
    }
    wave_lds_sync();
    if (lane == 0) {
        s.n_rle = base;
        dfl::p3c_header_post(s);
    }
}

// one workgroup (256 lanes) per BGZF block of the record stream
__global__ __launch_bounds__(dfl::kT) void k_deflate(DflArgs D) {
    extern __shared__ __align__(16) uint8_t smem[];
    dfl::Shared &s = *reinterpret_cast<dfl::Shared *>(smem);
    const int lane = threadIdx.x;
    const int64_t total = *D.stream_bytes;
    const int64_t nb = (total + dfl::kMaxIn - 1) / dfl::kMaxIn;
    const bool st = D.stamps != nullptr;
    uint32_t *tok = D.tok + (size_t)blockIdx.x * dfl::kTokWords;
    // phase stamps (dcr_deflate_probe): accumulated in LDS by lane 0, not
    // in per-lane registers
    __shared__ uint64_t t[12];
    uint64_t t0 = 0;
    if (st && lane < 12) t[lane] = 0;
    // slice-by-8 CRC32 tables, once per workgroup: t[0] the byte table,
    // t[k][i] = t[k-1][i] >> 8 ^ t[0][t[k-1][i] & 255]
    for (int i = lane; i < 256; i += dfl::kT) s.crc_t[0][i] = dfl::crc_byte((uint32_t)i);
    __syncthreads();
    for (int k = 1; k < 8; ++k) {
        for (int i = lane; i < 256; i += dfl::kT) {
            const uint32_t v = s.crc_t[k - 1][i];
            s.crc_t[k][i] = (v >> 8) ^ s.crc_t[0][v & 255];
        }
        __syncthreads();
    }
    auto stamp = [&](int k) {
        if (st && lane == 0) {
            const uint64_t now = __builtin_amdgcn_s_memtime();
            t[k] += now - t0;
            t0 = now;
        }
    };
    // blocks claimed one at a time when a counter is given: in the pipeline
    // the grid's workgroups start as inflate workgroups leave their CUs, and
    // a fixed stride left the late starters' blocks as the launch's tail
    __shared__ int64_t s_claim;
    auto claim = [&](int64_t fixed) -> int64_t {
        if (!D.claim) return fixed;
        __syncthreads();                 // every lane has read the previous claim
        if (lane == 0) s_claim = (int64_t)atomicAdd(D.claim, 1ull);
        __syncthreads();
        return s_claim;
    };
    for (int64_t b = claim(blockIdx.x); b < nb; b = claim(b + gridDim.x)) {
        if (st && lane == 0) t0 = __builtin_amdgcn_s_memtime();
        const int64_t off = b * (int64_t)dfl::kMaxIn;
        const uint32_t n = (uint32_t)((total - off) < (int64_t)dfl::kMaxIn ? (total - off) : dfl::kMaxIn);
        uint32_t *slot = reinterpret_cast<uint32_t *>(D.slots + b * (int64_t)dfl::kSlot);
        // stage the block as dwords (block starts are dword-aligned; the
        // record stream's allocation is padded), zero bytes past n
        {
            // 16 bytes per lane per load, four loads in flight (block starts
            // are 16-byte aligned: 0xff00 = 16 * 4080)
            static_assert(dfl::kMaxIn % 16 == 0 && sizeof(s.in) % 16 == 0, "16-byte staging");
            const uint4 *src = reinterpret_cast<const uint4 *>(D.stream + off);
            uint4 *dst = reinterpret_cast<uint4 *>(s.in);
            const uint32_t nq = (n + 15) / 16, pq = (uint32_t)sizeof(s.in) / 16;
            auto mask = [&](uint32_t w, uint32_t byte0) -> uint32_t {     // bytes of w at or past n zeroed
                return byte0 + 4 <= n ? w : byte0 >= n ? 0u : w & ((1u << (8 * (n - byte0))) - 1);
            };
            for (uint32_t i0 = lane; i0 < pq; i0 += 4 * dfl::kT) {
                uint4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t i = i0 + (uint32_t)k * dfl::kT;
                    v[k] = (i < nq) ? src[i] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t i = i0 + (uint32_t)k * dfl::kT;
                    if (i >= pq) continue;
                    uint4 w = v[k];
                    if (16 * i + 16 > n) {
                        w.x = mask(w.x, 16 * i);
                        w.y = mask(w.y, 16 * i + 4);
                        w.z = mask(w.z, 16 * i + 8);
                        w.w = mask(w.w, 16 * i + 12);
                    }
                    dst[i] = w;
                }
            }
        }
        dfl::p0_clear(s, lane);
        __syncthreads();
        stamp(0);
        dfl::p1_hash(s, n, lane);
        __syncthreads();
        stamp(1);
        dfl::p2_count(s, n, lane, tok);
        __syncthreads();
        stamp(2);
        dfl::p3a_keys(s, lane);
        __syncthreads();
        dfl::p3b_rank(s, lane);
        __syncthreads();
        stamp(3);
        dfl::p3c_trees(s, lane);
        // waves 2 and 3 are idle while lanes 0 and 64 build the two codes:
        // the sub-block CRCs (two per lane) go there
        static_assert(dfl::kT == 256, "the sub-block CRCs on waves 2 and 3 assume four waves");
        if (lane >= 128) {
            s.lane_crc[lane - 128] = dfl::sub_crc(s, n, lane - 128);
            s.lane_crc[lane] = dfl::sub_crc(s, n, lane);
        }
        __syncthreads();
        stamp(4);
        dfl::p3c_assign(s, lane);
        __syncthreads();
        stamp(10);
        if (lane < kW) p3c_header_wave(s, lane);
        else dfl::p3d_codes_litdist(s, lane - kW, dfl::kT - kW);   // waves 1-3, idle during the header
        __syncthreads();
        stamp(11);
        if (lane < 19) s.cl_code[lane] = dfl::code_of(s.cl_len, lane, s.next_code[2]);
        __syncthreads();
        stamp(5);
        dfl::p4_bits(s, n, lane, tok);
        __syncthreads();
        stamp(6);
        p4_scan_wg(s, n, lane, slot);
        __syncthreads();
        stamp(7);
        dfl::p5_emit(s, n, lane, tok, slot);
        __syncthreads();
        dfl::p6_copy(s, lane, slot);
        stamp(8);
        if (lane == 0) D.sizes[b] = dfl::p6_frame(s, n, slot);
        __syncthreads();
        stamp(9);
    }
    if (st && lane == 0)
        for (int k = 0; k < 12; ++k) atomicAdd(&D.stamps[k], (unsigned long long)t[k]);
}

// compressed blocks into one contiguous buffer (offsets from an exclusive scan)
__global__ __launch_bounds__(256) void k_compact(CompactArgs C) {
    const int64_t total = *C.stream_bytes;
    const int64_t nb = (total + dfl::kMaxIn - 1) / dfl::kMaxIn;
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint32_t n = (uint32_t)C.sizes[b];
        const int64_t o = C.offs[b];
        const uint8_t *src = C.slots + b * (int64_t)dfl::kSlot;
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) C.out[o + i] = src[i];
        if (b == nb - 1 && threadIdx.x == 0) {
            C.totals[0] = o + n;        // compressed bytes
            C.totals[1] = total;        // formatted bytes
            C.totals[2] = nb;           // blocks
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && nb == 0) {
        C.totals[0] = 0;
        C.totals[1] = 0;
        C.totals[2] = 0;
    }
}


// ---- exclusive prefix sums of int64 (record sizes -> record offsets, block
// sizes -> block offsets).  Tiles of 2,048 values per 256-lane workgroup: each
// lane sums its 8 consecutive values, the workgroup scans the lane sums (wave
// shuffles, then the four wave totals through LDS) and writes the tile's
// exclusive prefixes; tile totals go to `part`.  More than one tile: one
// workgroup scans the tile totals, and every tile after the first adds its
// prefix.  Plain launches, no inter-workgroup waiting.
constexpr int kScanT = 256, kScanPer = 8, kScanTile = kScanT * kScanPer;

__device__ __forceinline__ int64_t wg_excl_scan(int64_t v, int64_t &total, int64_t *wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int64_t before = 0;
    for (int k = 0; k < w; ++k) before += wsum[k];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return before + x - v;
}

__global__ __launch_bounds__(kScanT) void k_scan_tiles(const int64_t *in, int64_t *out, int64_t *part, int n) {
    __shared__ int64_t wsum[4];
    const int64_t t0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanPer;
    int64_t v[kScanPer], s = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        v[k] = t0 + k < n ? in[t0 + k] : 0;
        s += v[k];
    }
    int64_t total;
    int64_t run = wg_excl_scan(s, total, wsum);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (t0 + k < n) out[t0 + k] = run;
        run += v[k];
    }
    if (part && threadIdx.x == 0) part[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the tile totals in place
__global__ __launch_bounds__(kScanT) void k_scan_part(int64_t *part, int nt) {
    __shared__ int64_t wsum[4];
    int64_t carry = 0;
    for (int base = 0; base < nt; base += kScanT) {
        const int i = base + (int)threadIdx.x;
        const int64_t v = i < nt ? part[i] : 0;
        int64_t total;
        const int64_t e = wg_excl_scan(v, total, wsum);
        if (i < nt) part[i] = carry + e;
        carry += total;
    }
}

__global__ __launch_bounds__(kScanT) void k_scan_add(int64_t *out, const int64_t *part, int n) {
    const int64_t add = part[blockIdx.x + 1];
    const int64_t t0 = (int64_t)(blockIdx.x + 1) * kScanTile;
    for (int k = (int)threadIdx.x; k < kScanTile; k += kScanT)
        if (t0 + k < n) out[t0 + k] += add;
}

size_t scan_tmp_bytes(int n) { return 8 * (size_t)((n + kScanTile - 1) / kScanTile + 1); }

hipError_t scan_excl_i64(const int64_t *in, int64_t *out, int n, int64_t *tmp, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int nt = (n + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(k_scan_tiles, dim3((unsigned)nt), dim3(kScanT), 0, s, in, out, nt > 1 ? tmp : nullptr, n);
    if (nt > 1) {
        hipLaunchKernelGGL(k_scan_part, dim3(1), dim3(kScanT), 0, s, tmp, nt);
        hipLaunchKernelGGL(k_scan_add, dim3((unsigned)(nt - 1)), dim3(kScanT), 0, s, out, (const int64_t *)tmp, n);
    }
    return hipGetLastError();
}

// ---- the overlapping mates (dcr_set_mate_overlap; include/dcr.h states the
// map and the rules).  One wave per family in 256-lane blocks, as k_filter;
// runs after the QC tables and before the filters.  The map is the written
// record's (pos, CIGAR, len), not the stored column maps.
//
// A lane owns pairs, not bases: it takes reference positions of an
// intersection of an M run of mate 1 with an M run of mate 2, finds the two
// base indices by subtraction, loads both bases and qualities as bytes and
// stores what changed as bytes.  A base has one reference position and a
// position one base per mate, so a pair (i0, i1) belongs to exactly one lane
// and no lane reads a byte another lane writes: no barrier, no second pass,
// no LDS.  (The two records' windows are misaligned against each other by
// (pos1 - pos0) mod 4, so dword accesses would need a funnel shift on one
// side and a read-modify-write on words two lanes share; a family's overlap
// is a few hundred bytes.)
//
// When both CIGARs are one M run the intersection is lane arithmetic.
// Otherwise the wave walks the two CIGARs run by run (every lane the same
// walk: the wave index comes from readfirstlane, so its branches are
// wave-uniform), always advancing the run that ends first, and the lanes
// stride each intersection: the work follows the number of runs, never the
// length of a D or N run.  len, n_cig and, through them, every base index are
// clamped to the record's region (as bf_rec does); positions are 64-bit.
struct MoRec {
    const uint32_t *cig;
    uint8_t *seq, *qual;
    int64_t len, ncig, pos;
};
// a place in a CIGAR (next operation k, its reference position rp and base
// index bi) and the M run found last: n bases from base b0 at position r0
struct MoCur {
    int64_t k, rp, bi;
    int64_t r0, b0, n;      // n == 0: no run left
};

__device__ __forceinline__ void mo_rec(const dcr_out &o, const int64_t *col_off, int64_t r, MoRec &R) {
    const int64_t ro = col_off[r], room = col_off[r + 1] - ro;
    R.cig = o.cigar + ro;
    R.seq = o.seq + ro;
    R.qual = o.qual + ro;
    R.len = bf_clamp(o.len[r], room);
    R.ncig = bf_clamp(o.n_cig[r], room);
    R.pos = o.pos[r];
}

// the next M / = / X run that still holds a base of the map
__device__ __forceinline__ void mo_next(const MoRec &R, MoCur &c) {
    c.n = 0;
    while (c.k < R.ncig && c.bi < R.len) {
        const uint32_t v = R.cig[c.k++];
        const int64_t n = v >> 4;
        const uint32_t op = v & 15u;
        if (op == 0u || op == 7u || op == 8u) {
            const int64_t left = R.len - c.bi;
            c.r0 = c.rp;
            c.b0 = c.bi;
            c.n = n < left ? n : left;
            c.rp += n;
            c.bi += n;
            if (c.n > 0) return;
        } else if (op == 1u || op == 4u) {
            c.bi += n;
        } else if (op == 2u || op == 3u) {
            c.rp += n;
        }                   // H, P and the unused codes: neither
    }
}

// n positions from base i0 of mate 1 and base i1 of mate 2, strided by the lanes
__device__ __forceinline__ void mo_segment(const MoRec &R0, const MoRec &R1, int64_t i0, int64_t i1, int64_t n, int mode,
                                           uint32_t &cmp, uint32_t &dis, uint32_t &chg) {
    for (int64_t t = lane_id(); t < n; t += kW) {
        const int64_t a = i0 + t, b = i1 + t;
        const uint32_t x = R0.seq[a], qx = R0.qual[a], y = R1.seq[b], qy = R1.qual[b];
        if (x == 'N' || y == 'N') continue;
        ++cmp;
        uint32_t nx = x, nqx = qx, ny = y, nqy = qy;
        if (x == y) {
            if (mode == DCR_OVL_CONSENSUS) nqx = nqy = qx + qy < 93u ? qx + qy : 93u;
        } else {
            ++dis;
            if (mode == DCR_OVL_CONSENSUS && qx != qy) {
                nx = ny = qx > qy ? x : y;
                nqx = nqy = qx > qy ? qx - qy : qy - qx;
            } else {
                nx = ny = 'N';
                nqx = qx < 2u ? qx : 2u;
                nqy = qy < 2u ? qy : 2u;
            }
        }
        if (nx != x) R0.seq[a] = (uint8_t)nx;
        if (nqx != qx) R0.qual[a] = (uint8_t)nqx;
        if (ny != y) R1.seq[b] = (uint8_t)ny;
        if (nqy != qy) R1.qual[b] = (uint8_t)nqy;
        chg += (nx != x || nqx != qx ? 1u : 0u) + (ny != y || nqy != qy ? 1u : 0u);
    }
}

__device__ __forceinline__ bool mo_is_m(uint32_t v) { return (v & 15u) == 0u || (v & 15u) == 7u || (v & 15u) == 8u; }

__global__ __launch_bounds__(256) void k_mate_overlap(MateOverlapArgs A) {
    const int64_t wpb = blockDim.x / kW;
    const int64_t wave = (int64_t)blockIdx.x * wpb + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kW));
    const int64_t nw = (int64_t)gridDim.x * wpb;
    for (int64_t f = wave; f < A.n_fam; f += nw) {
        uint32_t cmp = 0, dis = 0, chg = 0;
        if (A.fam_fail[f] == 0) {
            MoRec R0, R1;
            mo_rec(A.ds, A.ds_col_off, 2 * f, R0);
            mo_rec(A.ds, A.ds_col_off, 2 * f + 1, R1);
            if (R0.ncig == 1 && R1.ncig == 1 && mo_is_m(R0.cig[0]) && mo_is_m(R1.cig[0])) {
                const int64_t m0 = R0.cig[0] >> 4, m1 = R1.cig[0] >> 4;
                const int64_t n0 = m0 < R0.len ? m0 : R0.len, n1 = m1 < R1.len ? m1 : R1.len;
                const int64_t lo = R0.pos > R1.pos ? R0.pos : R1.pos;
                const int64_t hi = R0.pos + n0 < R1.pos + n1 ? R0.pos + n0 : R1.pos + n1;
                mo_segment(R0, R1, lo - R0.pos, lo - R1.pos, hi - lo, A.mode, cmp, dis, chg);
            } else {
                MoCur c0{0, R0.pos, 0, 0, 0, 0}, c1{0, R1.pos, 0, 0, 0, 0};
                mo_next(R0, c0);
                mo_next(R1, c1);
                while (c0.n > 0 && c1.n > 0) {
                    const int64_t e0 = c0.r0 + c0.n, e1 = c1.r0 + c1.n;
                    const int64_t lo = c0.r0 > c1.r0 ? c0.r0 : c1.r0, hi = e0 < e1 ? e0 : e1;
                    mo_segment(R0, R1, c0.b0 + (lo - c0.r0), c1.b0 + (lo - c1.r0), hi - lo, A.mode, cmp, dis, chg);
                    if (e0 <= e1)
                        mo_next(R0, c0);
                    else
                        mo_next(R1, c1);
                }
            }
            cmp = wave_sum(cmp);
            dis = wave_sum(dis);
            chg = wave_sum(chg);
        }
        if (lane_id() == 0) {
            A.fam_ovl[3 * f] = (int32_t)cmp;
            A.fam_ovl[3 * f + 1] = (int32_t)dis;
            A.fam_ovl[3 * f + 2] = (int32_t)chg;
        }
    }
}

// ---- the allele counts at given sites (dcr_set_allele_sites; include/dcr.h
// states the map, the calls and the table).  One wave per family in 256-lane
// blocks, k_filter's grid; runs after the filters and before k_fmt_size, reads
// the duplex records as they will be written and writes nothing but the
// context's table.
//
// The work follows the sites hit, never the bases or the length of a run: the
// wave first looks the family's whole span [min pos, max end) up in the sorted
// keys (two lower bounds, wave-uniform: the wave index comes from
// readfirstlane, so the keys' loads and every branch on them are the whole
// wave's); a family that touches no site ends there.  Then it walks mate 1's
// CIGAR run by run; for each M / = / X / D run two lower bounds inside the
// range found give the sites of the run, and the lanes stride them.  A lane
// has its own record's call by subtraction (base index = the run's first base
// + p - the run's first position) and the other record's from a walk of that
// record's CIGAR (ac_call_at; a duplex CIGAR is a few operations).  Mate 2's
// runs follow in the same way and count only where mate 1 has no call.  A
// (family, site) pair belongs to exactly one lane, so the table is the only
// shared state: one 64-bit atomic add on the call's column, one on `both`
// where both records call.  No LDS, no barrier.
constexpr int64_t kAcPosEnd = (int64_t)1 << 31;     // a site's pos lies below it

// first index in [lo, hi) whose key is not below `key`
__device__ __forceinline__ int64_t ac_lower(const int64_t *keys, int64_t lo, int64_t hi, int64_t key) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t ac_clip(int64_t p) { return p < 0 ? 0 : p > kAcPosEnd ? kAcPosEnd : p; }

// the call of base i of a record (i inside the map)
__device__ __forceinline__ int ac_base(const MoRec &R, int64_t i, uint32_t min_q) {
    const uint32_t b = R.seq[i];
    if ((uint32_t)R.qual[i] < min_q) return 4;
    return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
}

// the call of a record at reference position p, -1 for none
__device__ __forceinline__ int ac_call_at(const MoRec &R, int64_t p, uint32_t min_q) {
    int64_t rp = R.pos, bi = 0;
    for (int64_t k = 0; k < R.ncig && bi < R.len && rp <= p; ++k) {
        const uint32_t v = R.cig[k];
        const int64_t n = v >> 4;
        const uint32_t op = v & 15u;
        if (op == 0u || op == 7u || op == 8u) {
            if (p < rp + n) return bi + (p - rp) < R.len ? ac_base(R, bi + (p - rp), min_q) : -1;
            rp += n;
            bi += n;
        } else if (op == 2u) {
            if (p < rp + n) return 5;
            rp += n;
        } else if (op == 1u || op == 4u) {
            bi += n;
        } else if (op == 3u) {
            rp += n;
        }                   // H, P and the unused codes: neither
    }
    return -1;
}

// the reference position after the last operation of the map (no less than the map's end)
__device__ __forceinline__ int64_t ac_end(const MoRec &R) {
    int64_t rp = R.pos, bi = 0;
    for (int64_t k = 0; k < R.ncig && bi < R.len; ++k) {
        const uint32_t v = R.cig[k];
        const int64_t n = v >> 4;
        const uint32_t op = v & 15u;
        if (op == 0u || op == 7u || op == 8u) {
            rp += n;
            bi += n;
        } else if (op == 1u || op == 4u) {
            bi += n;
        } else if (op == 2u || op == 3u) {
            rp += n;
        }
    }
    return rp;
}

__device__ __forceinline__ int ac_molecule(int c0, int c1) {
    if (c1 < 0 || c0 == c1) return c0;
    if (c0 < 0) return c1;
    if (c0 == 4) return c1;
    if (c1 == 4) return c0;
    return 6;
}

// the runs of record R with a call, the sites [s_lo, s_hi) of the family's span strided by the
// lanes; O is the family's other record.  second: R is mate 2, whose sites count only where
// mate 1 (O) has no call.
__device__ __forceinline__ void ac_runs(const AlleleArgs &A, const MoRec &R, const MoRec &O, bool second, int64_t base,
                                        int64_t s_lo, int64_t s_hi) {
    int64_t rp = R.pos, bi = 0;
    for (int64_t k = 0; k < R.ncig && bi < R.len && s_lo < s_hi; ++k) {
        const uint32_t v = R.cig[k];
        const int64_t n = v >> 4;
        const uint32_t op = v & 15u;
        const bool m = op == 0u || op == 7u || op == 8u;
        if (m || op == 2u) {
            const int64_t left = R.len - bi;
            const int64_t ne = m && n > left ? left : n;
            const int64_t a = ac_lower(A.keys, s_lo, s_hi, base + ac_clip(rp));
            const int64_t b = ac_lower(A.keys, a, s_hi, base + ac_clip(rp + ne));
            for (int64_t s = a + lane_id(); s < b; s += kW) {
                const int64_t p = A.keys[s] - base;
                const int own = m ? ac_base(R, bi + (p - rp), (uint32_t)A.min_q) : 5;
                const int oth = ac_call_at(O, p, (uint32_t)A.min_q);
                unsigned long long *row = A.table + s * DCR_ALLELE_COLS;
                if (second) {
                    if (oth < 0) atomicAdd(row + own, 1ull);
                } else {
                    atomicAdd(row + ac_molecule(own, oth), 1ull);
                    if (oth >= 0) atomicAdd(row + 7, 1ull);
                }
            }
            s_lo = b;           // the runs' positions ascend
            rp += n;
            if (m) bi += n;
        } else if (op == 1u || op == 4u) {
            bi += n;
        } else if (op == 3u) {
            rp += n;
        }
    }
}

__global__ __launch_bounds__(256) void k_allele_counts(AlleleArgs A) {
    const int64_t wpb = blockDim.x / kW;
    const int64_t wave = (int64_t)blockIdx.x * wpb + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kW));
    const int64_t nw = (int64_t)gridDim.x * wpb;
    for (int64_t f = wave; f < A.n_fam; f += nw) {
        if (A.fam_fail[f] != 0 || (A.fam_filt && (A.fam_filt[f] & 0xff))) continue;
        const int64_t tid = A.fam_tid[f];
        if (tid < 0) continue;
        MoRec R0, R1;
        mo_rec(A.ds, A.ds_col_off, 2 * f, R0);
        mo_rec(A.ds, A.ds_col_off, 2 * f + 1, R1);
        const int64_t e0 = ac_end(R0), e1 = ac_end(R1);
        const int64_t lo = ac_clip(R0.pos < R1.pos ? R0.pos : R1.pos), hi = ac_clip(e0 > e1 ? e0 : e1);
        if (lo >= hi) continue;
        const int64_t base = tid << 32;
        const int64_t s_lo = ac_lower(A.keys, 0, A.n_keys, base + lo);
        const int64_t s_hi = ac_lower(A.keys, s_lo, A.n_keys, base + hi);
        if (s_lo == s_hi) continue;         // the common case of a sparse panel: one search, no walk
        ac_runs(A, R0, R1, false, base, s_lo, s_hi);
        ac_runs(A, R1, R0, true, base, s_lo, s_hi);
    }
}

// ---- the errors against a genome (dcr_set_genome; include/dcr.h states the
// map, the codes and the tables).  One launch per level (A.lv: the four
// single-strand records of a family, then its two duplex records), the same
// kernel: one level's tables are 3,104 32-bit bins and twelve 64-bit words,
// 12,512 bytes of LDS, so a workgroup does not wait for the LDS that both
// levels together (25 KB) or k_base_metrics' 56 KB would.  Runs in
// k_base_metrics' place: after the failure scan, before k_mate_overlap and the
// filters rewrite the duplex seq / qual.  Reads only; writes the slot's block.
//
// The reduction is k_base_metrics': a wave per record, 64 bases of an M run a
// step in a wave-uniform loop (the wave index comes from readfirstlane, so the
// CIGAR walk and its branches are the whole wave's), n[] as popcounts of
// ballots, the hot bin of sub and qual merged (bm_count), one LDS add per lane
// for the cycle (64 consecutive bases are 64 bins) and tri, a whole step past
// bin 511 summed over the wave; then one global 64-bit add per non-zero bin per
// workgroup.  A base's position is the run's first position plus the lane: the
// genome bytes of a step are 64 consecutive bytes (and their two neighbours).
// No 32-bit bin wraps: a base adds at most 1 to a bin and a launch covers
// records [r0, r1) whose regions hold fewer than 2^32 columns (the host splits
// a larger batch).  Every index is clamped to its region (mo_rec, gm_at).
#define GM_FN __device__ __forceinline__
GM_FN int gm_lane() { return lane_id(); }
GM_FN unsigned long long gm_pop(bool p) { return bm_pop(p); }
GM_FN unsigned long long gm_once(unsigned long long v) { return v; }
GM_FN void gm_count(uint32_t *h, int bin, bool act) { bm_count(h, bin, act); }
GM_FN void gm_wave_add(uint32_t *p, bool pred) {
    const uint32_t c = (uint32_t)bm_pop(pred);
    if (c && lane_id() == 0) atomicAdd(p, c);
}
GM_FN void gm_add(uint32_t *p) { atomicAdd(p, 1u); }
GM_FN int gm_code(uint8_t c) { return bm_code(c); }
#include "dcr_genome_body.h"

constexpr int kGmWords = 12 + kGmBins;      // one level's words in the block
static_assert(sizeof(dcr_genome_metrics) == 8 * 2 * (size_t)kGmWords &&
                  offsetof(dcr_genome_metrics, sub) == 8 * 24 &&
                  offsetof(dcr_genome_metrics, tri) == 8 * (24 + 2 * (kGmTri - kGmSub)) &&
                  offsetof(dcr_genome_metrics, cyc) == 8 * (24 + 2 * (kGmCyc - kGmSub)) &&
                  offsetof(dcr_genome_metrics, qual) == 8 * (24 + 2 * (kGmQual - kGmSub)),
              "k_genome_metrics' LDS layout follows dcr_genome_metrics");

struct GmShared {
    unsigned long long n[12];
    uint32_t cnt[kGmBins];
};

__global__ __launch_bounds__(kGmThreads) void k_genome_metrics(GenomeMetricsArgs A) {
    __shared__ GmShared S;
    for (int i = threadIdx.x; i < (int)(sizeof(GmShared) / 4); i += kGmThreads) reinterpret_cast<uint32_t *>(&S)[i] = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kGmThreads + threadIdx.x) / kW));
    const int nw = (int)(gridDim.x * (kGmThreads / kW));
    const int per = A.lv == 0 ? 2 : 1;          // log2 of a family's records on this level
    unsigned long long n[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = A.r0 + wave; r < A.r1; r += nw) {
        const int64_t f = r >> per;
        if (A.fam_fail[f] != 0) continue;
        MoRec M;
        mo_rec(A.o, A.col_off, r, M);
        const GmRec R{M.cig, M.seq, M.qual, M.len, M.ncig, M.pos};
        const int64_t tid = A.fam_tid[f];
        const uint8_t *g = A.codes;
        int64_t glen = 0;
        if (tid >= 0 && tid < (int64_t)A.n_ref) {
            const int64_t o = A.ref_off[tid];
            glen = A.ref_off[tid + 1] - o;
            g += o;
        }
        gm_record(R, (int)((r >> (per - 1)) & 1), g, glen, n, S.cnt);
    }
    if (lane_id() == 0)
        for (int t = 0; t < 12; ++t)
            if (n[t]) atomicAdd(&S.n[t], n[t]);
    __syncthreads();
    // the workgroup's tables into the slot's: one 64-bit add per non-zero bin.  Word w of the level
    // lies in its table of the block after the tables' parts of the levels before it
    unsigned long long *out = reinterpret_cast<unsigned long long *>(A.out);
    for (int w = threadIdx.x; w < kGmWords; w += kGmThreads) {
        unsigned long long v;
        int at;
        if (w < 12) {
            v = S.n[w];
            at = A.lv * 12 + w;
        } else {
            const int b = w - 12;
            v = S.cnt[b];
            const int t0 = b < kGmTri ? kGmSub : b < kGmCyc ? kGmTri : b < kGmQual ? kGmCyc : kGmQual;
            const int t1 = b < kGmTri ? kGmTri : b < kGmCyc ? kGmCyc : b < kGmQual ? kGmQual : kGmBins;
            at = 24 + 2 * t0 + A.lv * (t1 - t0) + (b - t0);
        }
        if (v) atomicAdd(&out[at], v);
    }
}
#undef GM_FN

}  // namespace dcrw
