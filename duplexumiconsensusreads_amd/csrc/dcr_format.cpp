// dcr_format.cpp — native writer side (include/dcr_io.h): the duplex
// consensus records of a batch, built from kernel outputs with the
// reference's exact field and tag layout, and a BGZF writer that deflates
// blocks on a worker pool (libdeflate).
//
// Reference (/root/reference/DuplexUMIConsensusReads.py):
//   record fields        make_consensus_read :1352-1384
//   name / flag          get_consensus_id :892-933, get_consensus_flag :936-968
//   duplex tags          add_tags(method="double_strand") :1076-1120
//   mate fields          fix_paired_end_fields :1390-1419
//   pysam typing         smallest integer type, 'f' float32, 'Z' text, 'B' arrays;
//                        sd/se text is str() of a list of numpy-1.x ints: "[1, 2]"
#include <cctype>
#include <cmath>
#include <fcntl.h>
#include <unistd.h>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dcr.h"
#include "../../include/dcr_io.h"
#include "dcr_host.h"

using namespace dcrh;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &m) {
    g_err = m;
    return code;
}

constexpr size_t kBlockData = 0xff00;
const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                          0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};

struct TLComp {
    libdeflate_compressor *c[13] = {};
    ~TLComp() {
        for (auto *p : c)
            if (p) libdeflate_free_compressor(p);
    }
    libdeflate_compressor *get(int level) {
        if (!c[level]) c[level] = libdeflate_alloc_compressor(level);
        return c[level];
    }
};
thread_local TLComp tl_comp;

// ASCII -> 4-bit BAM code ("=ACMGRSVTWYHKDBN", either case; unknown 15)
struct NtTable {
    uint8_t code[256];
    NtTable() {
        std::memset(code, 15, sizeof code);
        const char *a = "=ACMGRSVTWYHKDBN";
        for (int i = 0; i < 16; ++i) {
            code[(uint8_t)a[i]] = (uint8_t)i;
            code[(uint8_t)std::tolower(a[i])] = (uint8_t)i;
        }
    }
};
const NtTable kNt;

// SAM spec §5.3 bin of [beg, end)
int reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// growable byte buffer with unchecked appends after reserve()
struct Buf {
    std::vector<uint8_t> v;
    size_t n = 0;
    void reserve(size_t more) {
        if (n + more > v.size()) v.resize(std::max(v.size() * 2, n + more + (1 << 20)));
    }
    uint8_t *p() { return v.data() + n; }
    void b(uint8_t x) { v[n++] = x; }
    void raw(const void *s, size_t k) { std::memcpy(v.data() + n, s, k); n += k; }
    void u16(uint32_t x) { wr16(p(), x); n += 2; }
    void u32(uint32_t x) { wr32(p(), x); n += 4; }
    void str(const char *s) { raw(s, std::strlen(s)); }
    void uint(uint32_t x) {
        char t[12];
        int k = 0;
        do { t[k++] = (char)('0' + x % 10); x /= 10; } while (x);
        while (k) v[n++] = (uint8_t)t[--k];
    }
    void sint(int64_t x) {
        if (x < 0) { v[n++] = '-'; x = -x; }
        char t[24];
        int k = 0;
        do { t[k++] = (char)('0' + x % 10); x /= 10; } while (x);
        while (k) v[n++] = (uint8_t)t[--k];
    }
};

// pysam's type code for an untyped int tag value (>= 0 here)
void int_tag(Buf &o, const char *tag, int64_t v) {
    o.raw(tag, 2);
    if (v < 0) {
        if (v >= -128) { o.b('c'); o.b((uint8_t)(int8_t)v); }
        else if (v >= -32768) { o.b('s'); o.u16((uint32_t)(uint16_t)(int16_t)v); }
        else { o.b('i'); o.u32((uint32_t)(int32_t)v); }
    } else if (v <= 255) { o.b('C'); o.b((uint8_t)v); }
    else if (v <= 65535) { o.b('S'); o.u16((uint32_t)v); }
    else { o.b('I'); o.u32((uint32_t)v); }
}

void float_tag(Buf &o, const char *tag, double v) {
    o.raw(tag, 2);
    o.b('f');
    const float f = (float)v;
    uint32_t u;
    std::memcpy(&u, &f, 4);
    o.u32(u);
}

void z_begin(Buf &o, const char *tag) { o.raw(tag, 2); o.b('Z'); }

// ", <v>" for v < 1000 as 8 bytes (length in the last byte)
struct ListTab {
    uint8_t t[1000][8];
    ListTab() {
        for (int v = 0; v < 1000; ++v) {
            char s[8] = {',', ' '};
            int n = std::snprintf(s + 2, 6, "%d", v);
            std::memcpy(t[v], s, 7);
            t[v][7] = (uint8_t)(2 + n);
        }
    }
};
const ListTab kList;

// "[1, 2, 3]" (str() of a list of numpy-1.x ints); the caller reserved
// 7 bytes per value plus slack, so the 8-byte copies may run past the text
void list_text(Buf &o, const char *tag, const uint16_t *v, int32_t n) {
    z_begin(o, tag);
    o.b('[');
    uint8_t *p = o.p();
    for (int32_t i = 0; i < n; ++i) {
        const uint32_t x = v[i];
        if (x < 1000) {
            std::memcpy(p, kList.t[x], 8);
            p += kList.t[x][7];
        } else {
            p[0] = ','; p[1] = ' ';
            p += 2 + std::snprintf((char *)p + 2, 8, "%u", x);
        }
    }
    if (n) {                                   // drop the first ", "
        const size_t len = (size_t)(p - o.p());
        std::memmove(o.p(), o.p() + 2, len - 2);
        p -= 2;
    }
    o.n = (size_t)(p - o.v.data());
    o.b(']');
    o.b(0);
}

void phred_text(Buf &o, const char *tag, const uint8_t *q, int32_t n) {
    z_begin(o, tag);
    uint8_t *p = o.p();
    for (int32_t i = 0; i < n; ++i) p[i] = (uint8_t)(q[i] + 33);
    o.n += (size_t)n;
    o.b(0);
}

// B:C array of uint8 values (pysam infers 'C' for ints in 0..255)
void u8_array(Buf &o, const char *tag, const uint8_t *v, int32_t n) {
    o.raw(tag, 2);
    o.b('B');
    o.b('C');
    o.u32((uint32_t)n);
    o.raw(v, (size_t)n);
}


struct Ctx {
    const dcr_host_batch *hb;
    const dcr_fmt_out *ss, *ds;
};

// one BGZF block of in[0, len) (len <= 0xff00) at out (>= 64 KiB); returns its size
size_t bgzf_block(const uint8_t *in, size_t len, int level, uint8_t *out) {
    size_t clen = libdeflate_deflate_compress(tl_comp.get(level), in, len, out + 18, 0x10000 - 26);
    if (clen == 0) clen = libdeflate_deflate_compress(tl_comp.get(0), in, len, out + 18, 0x10000 - 26);
    if (clen == 0) return 0;
    out[0] = 0x1f; out[1] = 0x8b; out[2] = 8; out[3] = 4;
    wr32(out + 4, 0); out[8] = 0; out[9] = 0xff;
    wr16(out + 10, 6); out[12] = 66; out[13] = 67; wr16(out + 14, 2);
    wr16(out + 16, (uint32_t)(clen + 25));
    wr32(out + 18 + clen, libdeflate_crc32(0, in, len));
    wr32(out + 22 + clen, (uint32_t)len);
    return clen + 26;
}

}  // namespace

struct dcr_bgzw {
    FILE *f = nullptr;
    int level = 6;
    // the pool and the pending buffer are made on first use: the side-file
    // writers of most runs never write a record
    int n_threads = 0;
    std::unique_ptr<Pool> pool;
    std::unique_ptr<uint8_t[]> in;   // pending uncompressed bytes [in_cap]
    size_t in_cap = 0, n_in = 0;
    Pool &pl() {
        if (!pool) pool.reset(new Pool(pick_threads(n_threads)));
        return *pool;
    }
    std::vector<std::vector<uint8_t>> out;
    std::vector<size_t> out_len;
    int64_t bytes_in = 0, bytes_out = 0;
    bool bad = false;

    // deflate in[0, n) as blocks of 0xff00 bytes on the pool, write in order
    bool flush(size_t n) {
        const size_t nb = (n + kBlockData - 1) / kBlockData;
        if (out.size() < nb) { out.resize(nb); out_len.resize(nb); }
        const int lvl = level;
        auto one = [&](size_t i) {
            const size_t off = i * kBlockData, len = std::min(kBlockData, n - off);
            std::vector<uint8_t> &o = out[i];
            if (o.size() < 0x10000) o.resize(0x10000);
            out_len[i] = bgzf_block(in.get() + off, len, lvl, o.data());
            return out_len[i] != 0;
        };
        bool ok = true;
        if (nb == 1) ok = one(0);            // a header, a short tail: no pool needed
        else ok = pl().run(nb, one);
        if (!ok) { g_err = "BGZF block failed to deflate"; return false; }
        for (size_t i = 0; i < nb; ++i) {
            if (std::fwrite(out[i].data(), 1, out_len[i], f) != out_len[i]) { g_err = "write failed"; return false; }
            bytes_out += (int64_t)out_len[i];
        }
        bytes_in += (int64_t)n;
        return true;
    }
    bool put_compressed(const uint8_t *s, size_t n, size_t raw) {
        if (std::fwrite(s, 1, n, f) != n) { g_err = "write failed"; return false; }
        bytes_out += (int64_t)n;
        bytes_in += (int64_t)raw;
        return true;
    }
    bool write(const uint8_t *s, size_t n) {
        if (n && !in_cap) {
            in_cap = kBlockData * (size_t)std::max(64, 8 * pick_threads(n_threads));
            in.reset(new uint8_t[in_cap]);
        }
        while (n > 0) {
            const size_t k = std::min(in_cap - n_in, n);
            std::memcpy(in.get() + n_in, s, k);
            n_in += k; s += k; n -= k;
            if (n_in == in_cap) {
                if (!flush(n_in)) return false;
                n_in = 0;
            }
        }
        return true;
    }
};

namespace {

// one duplex record (pe j of processed family f)
void format_record(const Ctx &c, int32_t f, int j, const char *code, size_t l_code, Buf &o) {
    const dcr_host_batch *hb = c.hb;
    const dcr_fmt_out *ss = c.ss, *ds = c.ds;
    const int32_t k = 2 * f + j, a = 4 * f + 2 * j, b = a + 1;
    const int32_t pos = ds->pos[k], opos = ds->pos[2 * f + 1 - j];
    const int32_t len = ds->len[k];
    const int32_t tlen = ds->pos[2 * f + 1] + ds->len[2 * f + 1] - ds->pos[2 * f];
    const int32_t tid = hb->fam_tid[f];
    const int64_t ro = hb->ds_col_off[k], ao = hb->ss_col_off[a], bo = hb->ss_col_off[b];
    const size_t rec0 = o.n;
    o.u32(0);                                        // block_size
    o.u32((uint32_t)tid);                            // reference_id = read0's (:1363)
    o.u32((uint32_t)pos);                            // reference_start (:790)
    const char *pe = j == 0 ? "_paired-end1" : "_paired-end2";
    const size_t l_rn = 16 + l_code + 12 + 1;        // "consensus_family" code pe NUL
    o.b((uint8_t)l_rn);
    o.b((uint8_t)(ds->mapq[k] & 0xff));
    int64_t rl = 0;
    const uint32_t *cg = ds->cigar + ro;
    const int32_t nc = ds->n_cig[k];
    for (int32_t i = 0; i < nc; ++i) {
        const uint32_t op = cg[i] & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[i] >> 4;
    }
    o.u16(pos >= 0 ? (uint32_t)reg2bin(pos, pos + (rl > 0 ? rl : 1)) : 4680u);
    o.u16((uint32_t)nc);
    o.u16(j == 0 ? 99u : 147u);                      // get_consensus_flag (:959-963)
    o.u32((uint32_t)len);
    o.u32((uint32_t)tid);                            // fix_paired_end_fields (:1406-1416)
    o.u32((uint32_t)opos);
    o.u32((uint32_t)(j == 0 ? tlen : -tlen));
    o.str("consensus_family");                       // get_consensus_id (:925-933)
    o.raw(code, l_code);
    o.str(pe);
    o.b(0);
    for (int32_t i = 0; i < nc; ++i) o.u32(cg[i]);
    const uint8_t *sq = ds->seq + ro;
    for (int32_t i = 0; i + 1 < len; i += 2) o.b((uint8_t)((kNt.code[sq[i]] << 4) | kNt.code[sq[i + 1]]));
    if (len & 1) o.b((uint8_t)(kNt.code[sq[len - 1]] << 4));
    o.raw(ds->qual + ro, (size_t)len);
    // tags, in add_tags' order (:1117-1120)
    z_begin(o, "MI");
    o.raw(code, l_code);
    o.b(0);
    z_begin(o, "RX");
    o.str(hb->names + hb->fam_rx[2 * f + j]);
    o.b(0);
    const int32_t a0 = hb->sub_off[a], a1 = hb->sub_off[a + 1], b0 = hb->sub_off[b], b1 = hb->sub_off[b + 1];
    u8_array(o, "aQ", hb->read_mapq + a0, a1 - a0);
    u8_array(o, "bQ", hb->read_mapq + b0, b1 - b0);
    // cQ: the two single-strand MAPQs (ints <= 255 -> 'C')
    o.raw("cQ", 2); o.b('B'); o.b('C'); o.u32(2);
    o.b((uint8_t)ss->mapq[a]); o.b((uint8_t)ss->mapq[b]);
    list_text(o, "ad", ss->d + ao, ss->n_de[a]);
    list_text(o, "bd", ss->d + bo, ss->n_de[b]);
    list_text(o, "cd", ds->d + ro, ds->n_de[k]);
    int_tag(o, "aD", ss->D[a]); int_tag(o, "bD", ss->D[b]); int_tag(o, "cD", ds->D[k]);
    int_tag(o, "aM", ss->M[a]); int_tag(o, "bM", ss->M[b]); int_tag(o, "cM", ds->M[k]);
    list_text(o, "ae", ss->e + ao, ss->n_de[a]);
    list_text(o, "be", ss->e + bo, ss->n_de[b]);
    list_text(o, "ce", ds->e + ro, ds->n_de[k]);
    float_tag(o, "aE", ss->E[a]); float_tag(o, "bE", ss->E[b]); float_tag(o, "cE", ds->E[k]);
    z_begin(o, "ac"); o.raw(ss->seq + ao, (size_t)ss->len[a]); o.b(0);
    z_begin(o, "bc"); o.raw(ss->seq + bo, (size_t)ss->len[b]); o.b(0);
    phred_text(o, "aq", ss->qual + ao, ss->len[a]);
    phred_text(o, "bq", ss->qual + bo, ss->len[b]);
    wr32(o.v.data() + rec0, (uint32_t)(o.n - rec0 - 4));
}

size_t record_bound(const Ctx &c, int32_t f, int j, size_t l_code) {
    const int32_t k = 2 * f + j, a = 4 * f + 2 * j, b = a + 1;
    size_t n = 36 + 16 + l_code + 13 + 4 * (size_t)c.ds->n_cig[k] + (size_t)c.ds->len[k] * 2;
    n += 8 + l_code + 4 + std::strlen(c.hb->names + c.hb->fam_rx[2 * f + j]);
    n += 24 + (size_t)(c.hb->sub_off[a + 1] - c.hb->sub_off[a]) + (size_t)(c.hb->sub_off[b + 1] - c.hb->sub_off[b]);
    n += 16 + 8 * (2 * (size_t)c.ss->n_de[a] + 2 * (size_t)c.ss->n_de[b] + 2 * (size_t)c.ds->n_de[k]) + 64;
    n += 9 * 8 + 3 * 8 + 2 * ((size_t)c.ss->len[a] + c.ss->len[b]) + 32;
    return n;
}

// one single-strand record (subfamily k of processed family f): the record
// make_consensus_read(method="single_strand") returns (:1352-1384), tags of
// add_tags (:1054-1073); mate fields stay unset (-1, -1, 0)
void format_record_ss(const Ctx &c, int32_t f, int k, const char *code, size_t l_code, Buf &o) {
    static const char *const kSub[4] = {"_A1", "_B2", "_B1", "_A2"};   // get_consensus_id (:909-920)
    const dcr_host_batch *hb = c.hb;
    const dcr_fmt_out *ss = c.ss;
    const int32_t s = 4 * f + k;
    const int32_t pos = ss->pos[s], len = ss->len[s], tid = hb->fam_tid[f];
    const int64_t ro = hb->ss_col_off[s];
    const size_t rec0 = o.n;
    o.u32(0);                                        // block_size
    o.u32((uint32_t)tid);
    o.u32((uint32_t)pos);
    o.b((uint8_t)(16 + l_code + 3 + 1));             // "consensus_family" code _XX NUL
    o.b((uint8_t)(ss->mapq[s] & 0xff));
    int64_t rl = 0;
    const uint32_t *cg = ss->cigar + ro;
    const int32_t nc = ss->n_cig[s];
    for (int32_t i = 0; i < nc; ++i) {
        const uint32_t op = cg[i] & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += cg[i] >> 4;
    }
    o.u16(pos >= 0 ? (uint32_t)reg2bin(pos, pos + (rl > 0 ? rl : 1)) : 4680u);
    o.u16((uint32_t)nc);
    o.u16(hb->sub_flag[s]);                          // get_consensus_flag (:957-958): read0's
    o.u32((uint32_t)len);
    o.u32(0xffffffffu);                              // next_refID, next_pos -1; tlen 0
    o.u32(0xffffffffu);
    o.u32(0);
    o.str("consensus_family");
    o.raw(code, l_code);
    o.str(kSub[k]);
    o.b(0);
    for (int32_t i = 0; i < nc; ++i) o.u32(cg[i]);
    const uint8_t *sq = ss->seq + ro;
    for (int32_t i = 0; i + 1 < len; i += 2) o.b((uint8_t)((kNt.code[sq[i]] << 4) | kNt.code[sq[i + 1]]));
    if (len & 1) o.b((uint8_t)(kNt.code[sq[len - 1]] << 4));
    o.raw(ss->qual + ro, (size_t)len);
    z_begin(o, "MI");
    o.str(hb->names + hb->sub_mi[s]);
    o.b(0);
    z_begin(o, "RX");
    o.str(hb->names + hb->sub_rx[s]);
    o.b(0);
    u8_array(o, "sQ", hb->read_mapq + hb->sub_off[s], hb->sub_off[s + 1] - hb->sub_off[s]);
    list_text(o, "sd", ss->d + ro, ss->n_de[s]);
    int_tag(o, "sD", ss->D[s]);
    int_tag(o, "sM", ss->M[s]);
    list_text(o, "se", ss->e + ro, ss->n_de[s]);
    float_tag(o, "sE", ss->E[s]);
    wr32(o.v.data() + rec0, (uint32_t)(o.n - rec0 - 4));
}

size_t record_bound_ss(const Ctx &c, int32_t f, int k, size_t l_code) {
    const int32_t s = 4 * f + k;
    size_t n = 36 + 16 + l_code + 4 + 4 * (size_t)c.ss->n_cig[s] + (size_t)c.ss->len[s] * 2;
    n += 8 + std::strlen(c.hb->names + c.hb->sub_mi[s]) + std::strlen(c.hb->names + c.hb->sub_rx[s]);
    n += 8 + (size_t)(c.hb->sub_off[s + 1] - c.hb->sub_off[s]);
    n += 16 + 8 * 2 * (size_t)c.ss->n_de[s] + 64;
    n += 3 * 8 + 32;
    return n;
}

// Families [0, n_fam) in chunks, each formatted (fmt(f, code, l_code, buf)
// appends the family's records) and deflated by one task into its own run of
// BGZF blocks (a record may span blocks), written in order.
template <typename Fmt>
int write_chunked(dcr_bgzw *w, const dcr_host_batch *hb, int32_t n_fam, Fmt fmt) {
    const int64_t *code_of = hb->fam_code;
    // pending bytes first (blocks stay in order)
    if (w->n_in) {
        if (!w->flush(w->n_in)) { w->bad = true; return DCR_IO_EFILE; }
        w->n_in = 0;
    }
    const int32_t chunk = 128;
    const int32_t nch = (n_fam + chunk - 1) / chunk;
    const int32_t group = std::max(1, 4 * w->pl().size());
    struct Task { Buf raw; std::vector<uint8_t> comp; size_t n_comp = 0; };
    std::vector<Task> tasks((size_t)std::min(nch, group));
    const int lvl = w->level;
    for (int32_t g0 = 0; g0 < nch; g0 += group) {
        const int32_t g1 = std::min(nch, g0 + group);
        const bool ok = w->pl().run((size_t)(g1 - g0), [&](size_t gi) {
            Task &t = tasks[gi];
            Buf &o = t.raw;
            o.n = 0;
            const int32_t f0 = (g0 + (int32_t)gi) * chunk, f1 = std::min(n_fam, f0 + chunk);
            for (int32_t f = f0; f < f1; ++f) {
                const char *code = hb->names + code_of[f];
                fmt(f, code, std::strlen(code), o);
            }
            const size_t nb = (o.n + kBlockData - 1) / kBlockData;
            if (t.comp.size() < nb * 0x10000) t.comp.resize(nb * 0x10000);
            t.n_comp = 0;
            for (size_t b = 0; b < nb; ++b) {
                const size_t off = b * kBlockData, len = std::min(kBlockData, o.n - off);
                const size_t cl = bgzf_block(o.v.data() + off, len, lvl, t.comp.data() + t.n_comp);
                if (!cl) return false;
                t.n_comp += cl;
            }
            return true;
        });
        if (!ok) { w->bad = true; return fail(DCR_IO_EFILE, "BGZF block failed to deflate"); }
        for (int32_t gi = 0; gi < g1 - g0; ++gi)
            if (!w->put_compressed(tasks[(size_t)gi].comp.data(), tasks[(size_t)gi].n_comp, tasks[(size_t)gi].raw.n)) {
                w->bad = true;
                return DCR_IO_EFILE;
            }
    }
    return DCR_IO_OK;
}

}  // namespace

extern "C" {

dcr_bgzw *dcr_bgzw_open(const char *path, int level, int n_threads) {
    if (!path || level < 0 || level > 12) { g_err = "bad arguments"; return nullptr; }
    // truncated at open, as fopen("wb"): works for any output (a FIFO,
    // /dev/null) and a run that never reaches close leaves a short file with
    // no BGZF EOF marker, never a new prefix over an old file's tail
    const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    FILE *f = fd >= 0 ? ::fdopen(fd, "wb") : nullptr;
    if (!f) {
        if (fd >= 0) ::close(fd);
        g_err = std::string("cannot open ") + path;
        return nullptr;
    }
    auto *w = new dcr_bgzw;
    w->f = f;
    w->level = level;
    w->n_threads = n_threads;
    return w;
}

int dcr_bgzw_write(dcr_bgzw *w, const void *bytes, int64_t n) {
    if (!w || n < 0 || (n > 0 && !bytes)) return fail(DCR_IO_EARG, "bad arguments");
    if (w->bad) return fail(DCR_IO_EFILE, "writer failed earlier");
    if (!w->write((const uint8_t *)bytes, (size_t)n)) { w->bad = true; return DCR_IO_EFILE; }
    return DCR_IO_OK;
}

int dcr_bgzw_put_blocks(dcr_bgzw *w, const void *blocks, int64_t n, int64_t raw_bytes) {
    if (!w || n < 0 || (n > 0 && !blocks)) return fail(DCR_IO_EARG, "bad arguments");
    if (w->bad) return fail(DCR_IO_EFILE, "writer failed earlier");
    if (w->n_in) {                      // pending bytes first: blocks stay in order
        if (!w->flush(w->n_in)) { w->bad = true; return DCR_IO_EFILE; }
        w->n_in = 0;
    }
    if (n && !w->put_compressed((const uint8_t *)blocks, (size_t)n, (size_t)raw_bytes)) {
        w->bad = true;
        return DCR_IO_EFILE;
    }
    return DCR_IO_OK;
}

int dcr_bgzw_close(dcr_bgzw *w) {
    if (!w) return fail(DCR_IO_EARG, "NULL writer");
    int rc = DCR_IO_OK;
    if (!w->bad && w->n_in && !w->flush(w->n_in)) rc = DCR_IO_EFILE;
    if (std::fwrite(kEof, 1, sizeof kEof, w->f) != sizeof kEof) rc = fail(DCR_IO_EFILE, "write failed");
    if (std::fflush(w->f) != 0) rc = fail(DCR_IO_EFILE, "write failed");
    if (std::fclose(w->f) != 0) rc = fail(DCR_IO_EFILE, "close failed");
    delete w;
    return rc;
}

int dcr_bgzw_sizes(dcr_bgzw *w, int64_t *out2) {
    if (!w || !out2) return fail(DCR_IO_EARG, "NULL argument");
    out2[0] = w->bytes_out;
    out2[1] = w->bytes_in + (int64_t)w->n_in;
    return DCR_IO_OK;
}

int32_t dcr_fmt_scan(const dcr_host_batch *hb, const dcr_fmt_out *ss, const dcr_fmt_out *ds,
                     const int32_t *read_status, int32_t n_fam, int32_t *kind, int32_t *which) {
    *kind = DCR_FAIL_NONE;
    *which = -1;
    auto st_fail = [](int st) { return st != 0 && st != DCR_ST_UPSTREAM && !(st & DCR_ST_PREP); };
    auto unicode = [&](int32_t s) {
        const int64_t o = hb->ss_col_off[s];
        for (int32_t i = 0; i < ss->len[s]; ++i)
            if (ss->qual[o + i] >= 95) return true;   // chr(q + 33) outside ASCII
        return false;
    };
    for (int32_t f = 0; f < n_fam; ++f) {
        // preprocess_family's read loop (:1272-1283): the first subfamily
        // holding a failing read (DCR_ST_PREP | that read's status)
        (void)read_status;
        for (int k = 0; k < 4; ++k)
            if (ss->status[4 * f + k] & DCR_ST_PREP) {
                *kind = ss->status[4 * f + k] & 0x0f;
                *which = 8 + k;
                return f;
            }
        for (int k = 0; k < 4; ++k)                   // make_consensus_read x4 (:1564-1569)
            if (st_fail(ss->status[4 * f + k])) { *kind = ss->status[4 * f + k]; *which = k; return f; }
        for (int j = 0; j < 2; ++j) {                 // x2 duplex (:1581-1582), then its set_tags (:1384)
            if (st_fail(ds->status[2 * f + j])) { *kind = ds->status[2 * f + j]; *which = 4 + j; return f; }
            if (unicode(4 * f + 2 * j) || unicode(4 * f + 2 * j + 1)) { *kind = DCR_FAIL_UNICODE; *which = 4 + j; return f; }
        }
    }
    return n_fam;
}

int dcr_fmt_write_filt(dcr_bgzw *w, const dcr_host_batch *hb, const dcr_fmt_out *ss, const dcr_fmt_out *ds,
                       int32_t n_fam, const int32_t *fam_filt) {
    if (!w || !hb || !ss || !ds || n_fam < 0 || n_fam > hb->n_fam) return fail(DCR_IO_EARG, "bad arguments");
    if (w->bad) return fail(DCR_IO_EFILE, "writer failed earlier");
    const Ctx c{hb, ss, ds};
    return write_chunked(w, hb, n_fam, [&](int32_t f, const char *code, size_t lc, Buf &o) {
        if (fam_filt && (fam_filt[f] & 0xff)) return;
        for (int j = 0; j < 2; ++j) {
            o.reserve(record_bound(c, f, j, lc));
            format_record(c, f, j, code, lc, o);
        }
    });
}

int dcr_fmt_write(dcr_bgzw *w, const dcr_host_batch *hb, const dcr_fmt_out *ss, const dcr_fmt_out *ds,
                  int32_t n_fam) {
    return dcr_fmt_write_filt(w, hb, ss, ds, n_fam, nullptr);
}

int dcr_fmt_write_ss_filt(dcr_bgzw *w, const dcr_host_batch *hb, const dcr_fmt_out *ss, int32_t n_fam,
                          const int32_t *fam_filt) {
    if (!w || !hb || !ss || n_fam < 0 || n_fam > hb->n_fam) return fail(DCR_IO_EARG, "bad arguments");
    if (!hb->sub_flag || !hb->sub_mi || !hb->sub_rx)
        return fail(DCR_IO_EARG, "the batch carries no single-strand metadata (DCR_INGEST_SS_META)");
    if (!ss->pos || !ss->n_cig || !ss->cigar) return fail(DCR_IO_EARG, "single-strand pos / n_cig / cigar missing");
    if (w->bad) return fail(DCR_IO_EFILE, "writer failed earlier");
    const Ctx c{hb, ss, nullptr};
    return write_chunked(w, hb, n_fam, [&](int32_t f, const char *code, size_t lc, Buf &o) {
        if (fam_filt && (fam_filt[f] & 0xff)) return;
        for (int k = 0; k < 4; ++k) {
            o.reserve(record_bound_ss(c, f, k, lc));
            format_record_ss(c, f, k, code, lc, o);
        }
    });
}

int dcr_fmt_write_ss(dcr_bgzw *w, const dcr_host_batch *hb, const dcr_fmt_out *ss, int32_t n_fam) {
    return dcr_fmt_write_ss_filt(w, hb, ss, n_fam, nullptr);
}

// the rules of include/dcr.h (dcr_filter), as dcr_writer.hip's k_filter applies them
int dcr_fmt_filter(const dcr_host_batch *hb, const dcr_fmt_out *ss, const dcr_fmt_out *ds, const dcr_filter *T,
                   int32_t n_fam, int32_t *fam_filt) {
    if (!hb || !ss || !ds || !T || !fam_filt || n_fam < 0 || n_fam > hb->n_fam) return fail(DCR_IO_EARG, "bad arguments");
    const uint32_t minq =
        (T->active & DCR_FILT_MASK_BASES) ? (uint32_t)(T->min_base_quality < 256 ? T->min_base_quality : 256) : 0u;
    for (int32_t f = 0; f < n_fam; ++f) {
        uint32_t why = 0, masked = 0;
        for (int j = 0; j < 2; ++j) {
            const int32_t k = 2 * f + j, a = 4 * f + 2 * j, b = a + 1;
            const int64_t ro = hb->ds_col_off[k];
            const int64_t L = ds->len[k];
            uint8_t *sq = const_cast<uint8_t *>(ds->seq) + ro, *ql = const_cast<uint8_t *>(ds->qual) + ro;
            uint32_t n_n = 0, q_sum = 0;
            for (int64_t i = 0; i < L; ++i) {
                if (ql[i] < minq) {
                    sq[i] = 'N';
                    if (ql[i] > 2) ql[i] = 2;
                    ++masked;
                }
                n_n += sq[i] == 'N';
                q_sum += ql[i];
            }
            const int32_t aD = ss->D[a], bD = ss->D[b];
            if (T->active & DCR_FILT_MIN_READS) {
                const int32_t hi = aD > bD ? aD : bD, lo = aD > bD ? bD : aD;
                if (!((int64_t)aD + bD >= T->min_reads[0] && hi >= T->min_reads[1] && lo >= T->min_reads[2]))
                    why |= DCR_FILT_MIN_READS;
            }
            if (T->active & DCR_FILT_ERROR_RATE)
                if (!(ds->E[k] <= T->max_error_rate[0] && ss->E[a] <= T->max_error_rate[1] &&
                      ss->E[b] <= T->max_error_rate[1]))
                    why |= DCR_FILT_ERROR_RATE;
            // one double multiply each (built with -ffp-contract=off)
            if ((T->active & DCR_FILT_NO_CALL) && (double)n_n > T->max_no_call_fraction * (double)L)
                why |= DCR_FILT_NO_CALL;
            if ((T->active & DCR_FILT_MEAN_QUAL) && (double)q_sum < T->min_mean_base_quality * (double)L)
                why |= DCR_FILT_MEAN_QUAL;
        }
        fam_filt[f] = (int32_t)(why | (masked << 8));
    }
    return DCR_IO_OK;
}

// the overlapping mates of include/dcr.h (dcr_set_mate_overlap), as dcr_writer.hip's k_mate_overlap
// rewrites them: the two CIGARs walked run by run, the run that ends first advanced
struct MoRec {
    const uint32_t *cig;
    uint8_t *seq, *qual;
    int64_t len, ncig, pos;
};
struct MoCur {
    int64_t k, rp, bi;      // next operation, its reference position and base index
    int64_t r0, b0, n;      // the M run found last (n == 0: none left)
};
static void mo_next(const MoRec &R, MoCur &c) {
    c.n = 0;
    while (c.k < R.ncig && c.bi < R.len) {
        const uint32_t v = R.cig[c.k++];
        const int64_t n = v >> 4;
        const uint32_t op = v & 15u;
        if (op == 0u || op == 7u || op == 8u) {
            c.r0 = c.rp;
            c.b0 = c.bi;
            c.n = std::min(n, R.len - c.bi);
            c.rp += n;
            c.bi += n;
            if (c.n > 0) return;
        } else if (op == 1u || op == 4u) {
            c.bi += n;
        } else if (op == 2u || op == 3u) {
            c.rp += n;
        }
    }
}

int dcr_fmt_mate_overlap(const dcr_host_batch *hb, const dcr_fmt_out *ds, int mode, int32_t n_fam, int32_t *fam_ovl) {
    if (!hb || !ds || !fam_ovl || n_fam < 0 || n_fam > hb->n_fam || (mode != DCR_OVL_MASK && mode != DCR_OVL_CONSENSUS))
        return fail(DCR_IO_EARG, "bad arguments");
    auto clampi = [](int64_t v, int64_t hi) { return v < 0 ? (int64_t)0 : v > hi ? hi : v; };
    for (int32_t f = 0; f < n_fam; ++f) {
        MoRec R[2];
        for (int j = 0; j < 2; ++j) {
            const int32_t k = 2 * f + j;
            const int64_t ro = hb->ds_col_off[k], room = hb->ds_col_off[k + 1] - ro;
            R[j] = MoRec{ds->cigar + ro, const_cast<uint8_t *>(ds->seq) + ro, const_cast<uint8_t *>(ds->qual) + ro,
                         clampi(ds->len[k], room), clampi(ds->n_cig[k], room), ds->pos[k]};
        }
        uint32_t cmp = 0, dis = 0, chg = 0;
        MoCur c0{0, R[0].pos, 0, 0, 0, 0}, c1{0, R[1].pos, 0, 0, 0, 0};
        mo_next(R[0], c0);
        mo_next(R[1], c1);
        while (c0.n > 0 && c1.n > 0) {
            const int64_t e0 = c0.r0 + c0.n, e1 = c1.r0 + c1.n;
            const int64_t lo = std::max(c0.r0, c1.r0), hi = std::min(e0, e1);
            for (int64_t p = lo; p < hi; ++p) {
                uint8_t &x = R[0].seq[c0.b0 + (p - c0.r0)], &qx = R[0].qual[c0.b0 + (p - c0.r0)];
                uint8_t &y = R[1].seq[c1.b0 + (p - c1.r0)], &qy = R[1].qual[c1.b0 + (p - c1.r0)];
                if (x == 'N' || y == 'N') continue;
                ++cmp;
                uint8_t nx = x, nqx = qx, ny = y, nqy = qy;
                if (x == y) {
                    if (mode == DCR_OVL_CONSENSUS) nqx = nqy = (uint8_t)std::min(qx + qy, 93);
                } else {
                    ++dis;
                    if (mode == DCR_OVL_CONSENSUS && qx != qy) {
                        nx = ny = qx > qy ? x : y;
                        nqx = nqy = (uint8_t)(qx > qy ? qx - qy : qy - qx);
                    } else {
                        nx = ny = 'N';
                        nqx = std::min<uint8_t>(qx, 2);
                        nqy = std::min<uint8_t>(qy, 2);
                    }
                }
                chg += (nx != x || nqx != qx) + (ny != y || nqy != qy);
                x = nx;
                qx = nqx;
                y = ny;
                qy = nqy;
            }
            if (e0 <= e1)
                mo_next(R[0], c0);
            else
                mo_next(R[1], c1);
        }
        fam_ovl[3 * f] = (int32_t)cmp;
        fam_ovl[3 * f + 1] = (int32_t)dis;
        fam_ovl[3 * f + 2] = (int32_t)chg;
    }
    return DCR_IO_OK;
}

// the allele counts of include/dcr.h (dcr_set_allele_sites), as dcr_writer.hip's k_allele_counts
// counts them; here site by site: both records' calls from a walk of their CIGARs
static int ac_base(const MoRec &R, int64_t i, int min_q) {
    if ((int)R.qual[i] < min_q) return 4;
    const uint8_t b = R.seq[i];
    return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4;
}

// the call of a record at p (-1: none); *end, when given, receives the position after the walk
static int ac_call_at(const MoRec &R, int64_t p, int min_q, int64_t *end = nullptr) {
    int64_t rp = R.pos, bi = 0;
    int call = -1;
    for (int64_t k = 0; k < R.ncig && bi < R.len; ++k) {
        const uint32_t v = R.cig[k];
        const int64_t n = v >> 4;
        const uint32_t op = v & 15u;
        if (op == 0u || op == 7u || op == 8u) {
            if (p >= rp && p < rp + n && bi + (p - rp) < R.len) call = ac_base(R, bi + (p - rp), min_q);
            rp += n;
            bi += n;
        } else if (op == 2u) {
            if (p >= rp && p < rp + n) call = 5;
            rp += n;
        } else if (op == 1u || op == 4u) {
            bi += n;
        } else if (op == 3u) {
            rp += n;
        }
    }
    if (end) *end = rp;
    return call;
}

int dcr_fmt_allele_counts(const dcr_host_batch *hb, const dcr_fmt_out *ds, const int64_t *keys, int64_t n_keys,
                          int min_base_quality, int32_t n_fam, const int32_t *fam_filt, uint64_t *table) {
    if (!hb || !ds || !keys || !table || n_keys <= 0 || n_keys > DCR_ALLELE_MAX_SITES || min_base_quality < 0 ||
        n_fam < 0 || n_fam > hb->n_fam)
        return fail(DCR_IO_EARG, "bad arguments");
    for (int64_t i = 0; i < n_keys; ++i)
        if (keys[i] < 0 || (keys[i] & 0x80000000ll) || (i && keys[i] <= keys[i - 1]))
            return fail(DCR_IO_EARG, "allele sites: keys must be tid << 32 | pos, strictly increasing");
    auto clampi = [](int64_t v, int64_t hi) { return v < 0 ? (int64_t)0 : v > hi ? hi : v; };
    const int64_t pos_end = (int64_t)1 << 31;
    for (int32_t f = 0; f < n_fam; ++f) {
        if (fam_filt && (fam_filt[f] & 0xff)) continue;
        const int64_t tid = hb->fam_tid[f];
        if (tid < 0) continue;
        MoRec R[2];
        int64_t end[2];
        for (int j = 0; j < 2; ++j) {
            const int32_t k = 2 * f + j;
            const int64_t ro = hb->ds_col_off[k], room = hb->ds_col_off[k + 1] - ro;
            R[j] = MoRec{ds->cigar + ro, const_cast<uint8_t *>(ds->seq) + ro, const_cast<uint8_t *>(ds->qual) + ro,
                         clampi(ds->len[k], room), clampi(ds->n_cig[k], room), ds->pos[k]};
            (void)ac_call_at(R[j], 0, 0, &end[j]);
        }
        const int64_t lo = clampi(std::min(R[0].pos, R[1].pos), pos_end), hi = clampi(std::max(end[0], end[1]), pos_end);
        const int64_t *a = std::lower_bound(keys, keys + n_keys, (tid << 32) + lo);
        const int64_t *b = std::lower_bound(a, keys + n_keys, (tid << 32) + hi);
        for (const int64_t *s = a; s < b; ++s) {
            const int64_t p = *s - (tid << 32);
            const int c0 = ac_call_at(R[0], p, min_base_quality), c1 = ac_call_at(R[1], p, min_base_quality);
            if (c0 < 0 && c1 < 0) continue;
            int col;
            if (c1 < 0 || c0 == c1)
                col = c0;
            else if (c0 < 0 || c0 == 4)
                col = c1;
            else if (c1 == 4)
                col = c0;
            else
                col = 6;
            uint64_t *row = table + (s - keys) * DCR_ALLELE_COLS;
            ++row[col];
            if (c0 >= 0 && c1 >= 0) ++row[7];
        }
    }
    return DCR_IO_OK;
}

// the tables of include/dcr.h (dcr_metrics), as dcr_writer.hip's k_metrics counts them
static int met_err_bin(double E) {
    // one double multiply (built with -ffp-contract=off); NaN fails both compares
    return (E >= 0.0 && E <= 1.0) ? (int)std::rint(E * 1000.0) : DCR_MET_ERR_BINS - 1;
}

int dcr_fmt_metrics(const dcr_host_batch *hb, const dcr_fmt_out *ss, const dcr_fmt_out *ds, int32_t n_fam,
                    const int32_t *fam_fail, dcr_metrics *m) {
    if (!hb || !ss || !ds || !m || n_fam < 0 || n_fam > hb->n_fam) return fail(DCR_IO_EARG, "bad arguments");
    auto clampi = [](int64_t v, int64_t hi) { return v < 0 ? (int64_t)0 : v > hi ? hi : v; };
    auto columns = [&](int kind, bool rev, const uint16_t *d, const uint16_t *e, int64_t n) {
        for (int64_t c = 0; c < n; ++c) {
            const int64_t cp = rev ? n - 1 - c : c;
            const int64_t b = cp < DCR_MET_COL_BINS - 1 ? cp : DCR_MET_COL_BINS - 1;
            m->col[kind][0][b] += 1;
            m->col[kind][1][b] += d[c];
            m->col[kind][2][b] += e[c];
        }
    };
    for (int32_t f = 0; f < n_fam; ++f) {
        if (fam_fail && fam_fail[f] != 0) continue;
        m->n[0] += 1;
        for (int k = 0; k < 4; ++k) {
            const int32_t s = 4 * f + k;
            const int64_t ro = hb->ss_col_off[s], room = hb->ss_col_off[s + 1] - ro;
            const int64_t L = clampi(ss->len[s], room), N = clampi(ss->n_de[s], room);
            m->n[1] += (uint64_t)L;
            m->n[4] += (uint64_t)N;
            const int64_t nr = clampi((int64_t)hb->sub_off[s + 1] - hb->sub_off[s], DCR_MET_READS_BINS - 1);
            m->ss_reads[k][nr] += 1;
            for (int64_t i = 0; i < L; ++i) m->ss_qual[ss->qual[ro + i]] += 1;
            columns(0, k >= 2, ss->d + ro, ss->e + ro, N);
        }
        for (int j = 0; j < 2; ++j) {
            const int32_t r = 2 * f + j, a = 4 * f + 2 * j, b = a + 1;
            const int64_t ro = hb->ds_col_off[r], room = hb->ds_col_off[r + 1] - ro;
            const int64_t L = clampi(ds->len[r], room), N = clampi(ds->n_de[r], room);
            m->n[2] += (uint64_t)L;
            m->n[5] += (uint64_t)N;
            const int64_t aD = clampi(ss->D[a], DCR_MET_DEPTH_BINS - 1), bD = clampi(ss->D[b], DCR_MET_DEPTH_BINS - 1);
            m->ds_depth[aD > bD ? aD : bD][aD > bD ? bD : aD] += 1;
            m->err_c[met_err_bin(ds->E[r])] += 1;
            const int ea = met_err_bin(ss->E[a]), eb = met_err_bin(ss->E[b]);
            m->err_s[ea > eb ? ea : eb] += 1;
            for (int64_t i = 0; i < L; ++i) {
                m->ds_qual[ds->qual[ro + i]] += 1;
                m->n[3] += ds->seq[ro + i] == 'N';
            }
            columns(1, j == 1, ds->d + ro, ds->e + ro, N);
        }
    }
    return DCR_IO_OK;
}

// the tables of include/dcr.h (dcr_genome_metrics), as dcr_writer.hip's k_genome_metrics counts them;
// here one record after the other, run by run, the genome's three codes sliding along an M run
namespace {
struct GmGenome {
    const uint8_t *codes;
    const int64_t *ref_off;
    int32_t n_ref;
    // the sequence of tid: its codes and length (absent or out of range: length 0)
    const uint8_t *seq(int64_t tid, int64_t &len) const {
        if (tid < 0 || tid >= n_ref) {
            len = 0;
            return codes;
        }
        len = ref_off[tid + 1] - ref_off[tid];
        return codes + ref_off[tid];
    }
};
inline int gm_at(const uint8_t *g, int64_t glen, int64_t p) {
    if (p < 0 || p >= glen) return 4;
    return g[p] < 4 ? g[p] : 4;
}
inline int gm_base(uint8_t c) {
    switch (c | 0x20) {
        case 'a': return 0; case 'c': return 1; case 'g': return 2; case 't': return 3;
        default: return 4;
    }
}
void gm_record(const GmGenome &G, int64_t tid, const dcr_fmt_out *o, int64_t ro, int64_t room, int32_t r, int lv,
               int j, dcr_genome_metrics *m) {
    auto clampi = [](int64_t v, int64_t hi) { return v < 0 ? (int64_t)0 : v > hi ? hi : v; };
    const int64_t len = clampi(o->len[r], room), ncig = clampi(o->n_cig[r], room);
    const uint32_t *cig = o->cigar + ro;
    const uint8_t *seq = o->seq + ro, *qual = o->qual + ro;
    int64_t glen;
    const uint8_t *g = G.seq(tid, glen);
    uint64_t *n = m->n[lv];
    n[0] += 1;
    int64_t rp = o->pos[r], bi = 0;
    for (int64_t k = 0; k < ncig && bi < len; ++k) {
        const int64_t cnt = cig[k] >> 4;
        const uint32_t op = cig[k] & 15u;
        const int64_t here = std::min(cnt, len - bi);
        if (op == 0u || op == 7u || op == 8u) {
            int g5 = gm_at(g, glen, rp - 1), gc = gm_at(g, glen, rp);
            for (int64_t t = 0; t < here; ++t) {
                const int64_t i = bi + t;
                const int g3 = gm_at(g, glen, rp + t + 1);
                const int x = gm_base(seq[i]);
                n[1] += 1;
                if (gc == 4) {
                    n[5] += 1;
                } else if (x == 4) {
                    n[4] += 1;
                } else {
                    const int mis = gc != x;
                    n[2 + mis] += 1;
                    m->sub[lv][j][gc][x] += 1;
                    if (g5 < 4 && g3 < 4) m->tri[lv][j][g5][gc][g3][x] += 1;
                    const int64_t ip = j == 0 ? i : len - 1 - i;
                    const int64_t b = std::min<int64_t>(ip, DCR_GMET_CYC_BINS - 1);
                    m->cyc[lv][j][0][b] += 1;
                    m->qual[lv][0][qual[i]] += 1;
                    if (mis) {
                        m->cyc[lv][j][1][b] += 1;
                        m->qual[lv][1][qual[i]] += 1;
                    }
                }
                g5 = gc;
                gc = g3;
            }
            rp += cnt;
            bi += cnt;
        } else if (op == 1u) {
            n[6] += 1;
            n[7] += (uint64_t)here;
            bi += cnt;
        } else if (op == 4u) {
            bi += cnt;
        } else if (op == 2u) {
            n[8] += 1;
            n[9] += (uint64_t)cnt;
            rp += cnt;
        } else if (op == 3u) {
            rp += cnt;
        }
    }
}
}  // namespace

int dcr_fmt_genome_metrics(const dcr_host_batch *hb, const dcr_fmt_out *ss, const dcr_fmt_out *ds,
                           const uint8_t *codes, const int64_t *ref_off, int32_t n_ref, int32_t n_fam,
                           const int32_t *fam_fail, dcr_genome_metrics *m) {
    if (!hb || !ss || !ds || !codes || !ref_off || !m || n_ref <= 0 || n_fam < 0 || n_fam > hb->n_fam)
        return fail(DCR_IO_EARG, "bad arguments");
    if (!ss->pos || !ss->n_cig || !ss->cigar)
        return fail(DCR_IO_EARG, "genome metrics: the single-strand results lack pos, n_cig or cigar");
    if (ref_off[0] != 0) return fail(DCR_IO_EARG, "genome: ref_off[0] must be 0");
    for (int32_t t = 0; t < n_ref; ++t)
        if (ref_off[t + 1] < ref_off[t]) return fail(DCR_IO_EARG, "genome: ref_off must not decrease");
    const GmGenome G{codes, ref_off, n_ref};
    for (int32_t f = 0; f < n_fam; ++f) {
        if (fam_fail && fam_fail[f] != 0) continue;
        const int64_t tid = hb->fam_tid[f];
        for (int k = 0; k < 4; ++k) {
            const int32_t s = 4 * f + k;
            gm_record(G, tid, ss, hb->ss_col_off[s], hb->ss_col_off[s + 1] - hb->ss_col_off[s], s, 0, k >> 1, m);
        }
        for (int j = 0; j < 2; ++j) {
            const int32_t r = 2 * f + j;
            gm_record(G, tid, ds, hb->ds_col_off[r], hb->ds_col_off[r + 1] - hb->ds_col_off[r], r, 1, j, m);
        }
    }
    return DCR_IO_OK;
}

}  // extern "C"
