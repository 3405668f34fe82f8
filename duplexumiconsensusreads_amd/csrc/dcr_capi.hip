// dcr_capi.hip — C-ABI of libdcr.so (include/dcr.h): context, workspace,
// launches and timing for the gfx950 kernels in dcr_kernels.hip.
//
// One context per GPU: its own HIP stream, device copy of the parameters, and
// a grow-only workspace (reserve it once; the launch path never allocates,
// so a caller may capture dcr_run_batch into a hipGraph).
//
// Every device buffer is laid out by one walk of a Plan (256-byte regions):
// plan_workspace (the kernels' scratch), plan_io (a batch's inputs and both
// strands' outputs) and plan_writer (the device record writer).  A caller
// sizes with a null base, ensures the buffer, then walks again to fill the
// pointers.  plan_io, upload_inputs and download_outputs loop over kInFields /
// kOutFields, one row per array of dcr_batch / dcr_out in struct order.
// dcr_submit and dcr_submit_write share slot_open (streams, the slot's events,
// the busy check) and slot_run (wait for the upload, run, fetch the flag);
// launch_strand<DUPLEX> is the kernel sequence of one strand.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "dcr_internal.h"
#include "dcr_deflate.h"
#include "dcr_writer.h"

namespace {
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(DCR_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, n ? n : 16);
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

// One walk over a buffer's regions.  take<T>(n) returns the next region, n
// elements of T, and advances by its bytes (at least one) rounded up to 256.
// With a null base it only sizes: off ends as the bytes the buffer needs.
struct Plan {
    char *base = nullptr;
    size_t off = 0;
    template <typename T> T *take(size_t n) {
        T *p = base ? (T *)(base + off) : nullptr;
        off = align_up(off + std::max<size_t>(n * sizeof(T), 1));
        return p;
    }
};

// The kernels' workspace for a batch of these sizes.
void plan_workspace(const dcr_batch &s, Plan &p, dcr::Workspace &w) {
    const size_t n_reads = (size_t)std::max<int64_t>(s.n_reads, 1);
    const size_t cols = (size_t)std::max<int64_t>(std::max(s.ss_cols, s.ds_cols), 1);
    const size_t n_rec = (size_t)std::max<int64_t>(4LL * s.n_fam, 1);
    const size_t n_lay = (size_t)std::max<int64_t>(6LL * s.n_fam, 1);
    w.info = p.take<dcr_read_info>(n_reads);
    w.norm_cig = p.take<uint32_t>((size_t)std::max<int64_t>(s.n_cigar, 1));
    w.cons = p.take<int32_t>(cols);
    w.et = p.take<double>(cols);
    w.insflag = p.take<uint8_t>((size_t)std::max<int64_t>(s.ss_cols, 1));
    w.state = p.take<int4>(n_reads);
    // one 64-byte block, reset as a whole per batch (dcr_run_batch)
    dcr::Counters *ctr = (dcr::Counters *)p.take<char>(64);
    w.stamps = p.take<unsigned long long>(64);
    w.ovf = p.take<int>(n_rec);
    w.xlist = p.take<int>(n_rec);
    w.deep = p.take<int>(n_rec);
    w.meta = p.take<dcr::RecMeta>(n_rec);
    w.rmeta = p.take<uint2>(std::max<size_t>((size_t)s.n_reads, n_rec));
    w.rows = p.take<uint4>(n_rec);
    // insertion layouts: a row of kLayRow codes per single-strand read and per
    // duplex input (two per duplex record)
    w.lay_base = p.take<int>(n_lay);
    w.lay_mask = p.take<uint64_t>(4 * n_lay);
    w.lay = p.take<uint16_t>((size_t)dcr::kLayRow * (size_t)std::max<int64_t>(s.n_reads + 4LL * s.n_fam, 1));
    if (!ctr) return;
    w.err = &ctr->err;
    w.ovf_count = ctr->ovf_count;
    w.fast_count = ctr->fast_count;
    w.xcount = ctr->xcount;
    w.gen_next = ctr->gen_next;
    w.deep_count = &ctr->deep_count;
    w.lay_next = ctr->lay_next;
}

// The arrays of dcr_batch and dcr_out, in struct order: where the pointer
// sits, its element size and which of the batch's sizes counts its elements.
enum Count { kSubOff /* 4F + 1 */, kReads, kCigar, kBases, kDsOff /* 2F + 1 */, kRecords, kColumns };
struct Field {
    size_t at, elem;
    Count count;
};
#define DCR_FIELD(S, m, count) {offsetof(S, m), sizeof(*((S *)nullptr)->m), count}
constexpr Field kInFields[] = {
    DCR_FIELD(dcr_batch, sub_off, kSubOff),   DCR_FIELD(dcr_batch, read_pos, kReads),
    DCR_FIELD(dcr_batch, read_mapq, kReads),  DCR_FIELD(dcr_batch, seq_off, kReads),
    DCR_FIELD(dcr_batch, seq_len, kReads),    DCR_FIELD(dcr_batch, cig_off, kReads),
    DCR_FIELD(dcr_batch, cig_n, kReads),      DCR_FIELD(dcr_batch, cigar, kCigar),
    DCR_FIELD(dcr_batch, bases, kBases),      DCR_FIELD(dcr_batch, quals, kBases),
    DCR_FIELD(dcr_batch, ss_col_off, kSubOff), DCR_FIELD(dcr_batch, ds_col_off, kDsOff)};
constexpr Field kOutFields[] = {
    DCR_FIELD(dcr_out, status, kRecords), DCR_FIELD(dcr_out, pos, kRecords),   DCR_FIELD(dcr_out, mapq, kRecords),
    DCR_FIELD(dcr_out, len, kRecords),    DCR_FIELD(dcr_out, n_cig, kRecords), DCR_FIELD(dcr_out, n_de, kRecords),
    DCR_FIELD(dcr_out, D, kRecords),      DCR_FIELD(dcr_out, M, kRecords),     DCR_FIELD(dcr_out, E, kRecords),
    DCR_FIELD(dcr_out, seq, kColumns),    DCR_FIELD(dcr_out, qual, kColumns),  DCR_FIELD(dcr_out, cigar, kColumns),
    DCR_FIELD(dcr_out, d, kColumns),      DCR_FIELD(dcr_out, e, kColumns)};
#undef DCR_FIELD
// a pointer added to include/dcr.h without its row here does not compile
template <size_t N> constexpr bool consecutive(const Field (&t)[N], size_t first) {
    for (size_t i = 0; i < N; ++i)
        if (t[i].at != first + i * sizeof(void *)) return false;
    return true;
}
static_assert(sizeof(kInFields) / sizeof(Field) == 12 && sizeof(kOutFields) / sizeof(Field) == 14, "one row per array");
static_assert(sizeof(dcr_batch) - offsetof(dcr_batch, sub_off) == 12 * sizeof(void *), "dcr_batch ends in 12 pointers");
static_assert(sizeof(dcr_out) == 14 * sizeof(void *), "dcr_out is 14 pointers");
static_assert(consecutive(kInFields, offsetof(dcr_batch, sub_off)) && consecutive(kOutFields, 0), "rows in struct order");

void *field_ptr(const void *obj, const Field &f) {
    void *p;
    std::memcpy(&p, (const char *)obj + f.at, sizeof(p));
    return p;
}
void set_field_ptr(void *obj, const Field &f, void *p) { std::memcpy((char *)obj + f.at, &p, sizeof(p)); }

// elements of an input array of batch h
size_t in_count(const dcr_batch *h, Count k) {
    const int64_t n[] = {4 * (int64_t)h->n_fam + 1, h->n_reads, h->n_cigar, h->n_bases, 2 * (int64_t)h->n_fam + 1};
    return (size_t)n[k];
}

// Device layout of one batch's inputs and outputs in a single buffer; with a
// base it also fills the device views db (inputs) and dout[0..1]
// (single-strand, duplex outputs).
void plan_io(const dcr_batch *h, Plan &p, dcr_batch *db, dcr_out dout[2]) {
    if (p.base) *db = *h;
    for (const Field &f : kInFields) {
        char *r = p.take<char>(f.elem * in_count(h, f.count));
        if (p.base) set_field_ptr(db, f, r);
    }
    const int64_t nrec[2] = {4 * (int64_t)h->n_fam, 2 * (int64_t)h->n_fam};
    const int64_t ncol[2] = {h->ss_cols, h->ds_cols};
    for (int k = 0; k < 2; ++k)
        for (const Field &f : kOutFields) {
            char *r = p.take<char>(f.elem * (size_t)(f.count == kRecords ? nrec[k] : ncol[k]));
            if (p.base) set_field_ptr(&dout[k], f, r);
        }
}

size_t io_bytes(const dcr_batch *h) {
    Plan sz;
    plan_io(h, sz, nullptr, nullptr);
    return sz.off;
}

// the host batch's inputs -> device views (async on stream s)
hipError_t upload_inputs(const dcr_batch *h, const dcr_batch &db, hipStream_t s) {
    for (const Field &f : kInFields)
        if (const size_t bytes = f.elem * in_count(h, f.count)) {
            hipError_t e = hipMemcpyAsync(field_ptr(&db, f), field_ptr(h, f), bytes, hipMemcpyHostToDevice, s);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// device outputs -> the host dcr_out arrays that are not NULL (async on stream s)
hipError_t download_outputs(const dcr_out *dev, dcr_out *host, int64_t R, int64_t C, hipStream_t s) {
    for (const Field &f : kOutFields) {
        const size_t bytes = f.elem * (size_t)(f.count == kRecords ? R : C);
        if (field_ptr(host, f) && bytes) {
            hipError_t e = hipMemcpyAsync(field_ptr(host, f), field_ptr(dev, f), bytes, hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

// The device record writer's buffer: the metadata uploaded with the batch,
// the per-record sizes and offsets, the record stream and the BGZF blocks.
struct WriterBufs {
    char *names;
    int64_t *fam_code, *fam_rx;
    int32_t *fam_tid, *fam_fail, *ds_len;
    int64_t *rec_size, *rec_off, *scan;
    uint8_t *stream, *slots;
    int64_t *bsz, *boff;    // block sizes (+ the scan's total, then k_deflate's block counter), offsets
    uint8_t *comp;
    int64_t *tot;
    uint32_t *tok;
    int32_t *fam_filt;      // k_filter's outcomes; null unless a filter is set (dcr_set_filter)
    dcr_metrics *metrics;   // k_metrics' accumulator; null unless metrics are on (dcr_set_metrics)
    // null unless a base filter is set (dcr_set_base_filter): k_base_filter's count per family
    int32_t *base_masked;
    // null unless a base filter or the per-base tags (dcr_set_base_tags) are on: the column maps
    // k_consensus_general_map stores for them
    dcr::BaseMap bmap;
    dcr_base_metrics *base_metrics;   // k_base_metrics' accumulator; null unless base metrics are on (dcr_set_base_metrics)
    int32_t *fam_ovl;       // k_mate_overlap's counters [3F]; null unless a mode is set (dcr_set_mate_overlap)
    dcr_genome_metrics *genome_metrics;   // k_genome_metrics' block; null unless a genome is set (dcr_set_genome)
};

// The second stream of dcr_submit_write_ss: the single-strand records'
// metadata, sizes and offsets, their record stream and its BGZF blocks
// (k_deflate's slot, size and claim buffers of its second launch).
struct WriterSsBufs {
    int64_t B, nbm;         // the stream's bound in bytes and blocks (stream_bound_ss), set by the caller
    unsigned gd;            // k_deflate workgroups
    uint16_t *sub_flag;
    int64_t *sub_mi, *sub_rx;
    int64_t *rec_size, *rec_off, *scan;
    uint8_t *stream, *slots;
    int64_t *bsz, *boff;
    uint8_t *comp;
    int64_t *tot;
    uint32_t *tok;
};

// the single-strand stream's regions (plan_writer)
void plan_writer_ss(int64_t F, Plan &p, WriterSsBufs &ws) {
    ws.sub_flag = p.take<uint16_t>(4 * (size_t)F);
    ws.sub_mi = p.take<int64_t>(4 * (size_t)F);
    ws.sub_rx = p.take<int64_t>(4 * (size_t)F);
    ws.rec_size = p.take<int64_t>((size_t)(4 * F + 1));
    ws.rec_off = p.take<int64_t>((size_t)(4 * F + 1));
    ws.scan = (int64_t *)p.take<char>(
        std::max(dcrw::scan_tmp_bytes((int)(4 * F + 1)), dcrw::scan_tmp_bytes((int)(ws.nbm + 1))));
    ws.stream = p.take<uint8_t>((size_t)ws.B);
    ws.slots = p.take<uint8_t>((size_t)ws.nbm * dfl::kSlot);
    ws.bsz = p.take<int64_t>((size_t)(ws.nbm + 2));
    ws.boff = p.take<int64_t>((size_t)(ws.nbm + 1));
    ws.comp = p.take<uint8_t>((size_t)ws.nbm * dfl::kSlot);
    ws.tot = p.take<int64_t>(4);
    ws.tok = p.take<uint32_t>((size_t)ws.gd * dfl::kTokWords);
}

// F families, n_names bytes of names, a record stream of at most B bytes in
// at most nbm blocks, gd k_deflate workgroups; with ws, the single-strand
// stream's regions after them (the first stream's layout does not change)
// and with filt, k_filter's outcomes (no region without it); with met,
// k_metrics' accumulator (none without it); with bfilt (a base filter is set)
// k_base_filter's counts and with maps (the batch, when a base filter or the
// per-base tags or the base metrics are on) the column maps, after every
// other region (none without them); with bmet, k_base_metrics' accumulator
// after those; with ovl (dcr_set_mate_overlap) k_mate_overlap's counters; with
// gmet (dcr_set_genome) k_genome_metrics' block last
void plan_writer(int64_t F, int64_t n_names, int64_t B, int64_t nbm, unsigned gd, Plan &p, WriterBufs &w,
                 WriterSsBufs *ws = nullptr, bool filt = false, bool met = false, const dcr_batch *maps = nullptr,
                 bool bfilt = false, bool bmet = false, bool ovl = false, bool gmet = false) {
    w.names = p.take<char>((size_t)n_names + 1);
    w.fam_code = p.take<int64_t>((size_t)F);
    w.fam_rx = p.take<int64_t>(2 * (size_t)F);
    w.fam_tid = p.take<int32_t>((size_t)F);
    w.fam_fail = p.take<int32_t>((size_t)F);
    w.ds_len = p.take<int32_t>(2 * (size_t)F);
    w.rec_size = p.take<int64_t>((size_t)(2 * F + 1));
    w.rec_off = p.take<int64_t>((size_t)(2 * F + 1));
    w.scan = (int64_t *)p.take<char>(std::max(dcrw::scan_tmp_bytes((int)(2 * F + 1)), dcrw::scan_tmp_bytes((int)(nbm + 1))));
    w.stream = p.take<uint8_t>((size_t)B);
    w.slots = p.take<uint8_t>((size_t)nbm * dfl::kSlot);
    w.bsz = p.take<int64_t>((size_t)(nbm + 2));
    w.boff = p.take<int64_t>((size_t)(nbm + 1));
    w.comp = p.take<uint8_t>((size_t)nbm * dfl::kSlot);
    w.tot = p.take<int64_t>(4);
    w.tok = p.take<uint32_t>((size_t)gd * dfl::kTokWords);
    w.fam_filt = filt ? p.take<int32_t>((size_t)F) : nullptr;
    w.metrics = met ? p.take<dcr_metrics>(1) : nullptr;
    if (ws) plan_writer_ss(F, p, *ws);
    w.base_masked = nullptr;
    w.bmap = dcr::BaseMap{};
    if (bfilt) w.base_masked = p.take<int32_t>((size_t)F);
    if (maps) {
        w.bmap.flag = p.take<uint8_t>(6 * (size_t)F);
        w.bmap.ss_col = p.take<uint32_t>((size_t)maps->ss_cols);
        w.bmap.ds_col = p.take<uint32_t>((size_t)maps->ds_cols);
        w.bmap.ds_aln = p.take<uint32_t>((size_t)maps->ds_cols);
    }
    w.base_metrics = bmet ? p.take<dcr_base_metrics>(1) : nullptr;
    w.fam_ovl = ovl ? p.take<int32_t>(3 * (size_t)F) : nullptr;
    w.genome_metrics = gmet ? p.take<dcr_genome_metrics>(1) : nullptr;
}
}  // namespace

int dcr::set_error(int code, const std::string &msg) { return fail(code, msg); }

// The batch streams run at the device's highest priority: the input
// inflater's long launches (include/dcr_inflate.h) share the GPU and a
// batch's kernels should not queue behind spans inflated far ahead.
static hipError_t hi_prio_stream(hipStream_t *s) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest);
}

struct dcr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // ev[0] batch start, ev[1..8] after k_recmeta<ss>, fast<ss>, exact<ss>, general<ss>,
    // k_recmeta<ds>, fast<ds>, exact<ds>, general<ds>
    hipEvent_t ev[DCR_N_KERNEL_TIMES + 1] = {};
    dcr_params *d_params = nullptr;
    DevBuf ws;          // workspace
    DevBuf io;          // staging for the host-pointer entry point
    // streaming (dcr_submit / dcr_wait): copy streams and per-slot device buffers
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    // dcr_wait_write's copy of the compressed blocks: a stream of its own, so
    // that it does not queue behind the next batch's downloads on s_d2h
    // (which wait for that batch's kernels)
    hipStream_t s_fetch = nullptr;
    hipEvent_t ev_fetch = nullptr;      // blocking-sync event after the compressed-block copy
    struct Slot {
        DevBuf buf;
        DevBuf wbuf;              // device record writer: metadata, record stream, BGZF blocks
        int64_t *d_rec_off = nullptr;
        uint8_t *d_stream = nullptr, *d_comp = nullptr;
        // the single-strand stream of dcr_submit_write_ss (writer_ss)
        int64_t *d_ss_rec_off = nullptr;
        uint8_t *d_ss_stream = nullptr, *d_ss_comp = nullptr;
        uint8_t *d_map_flag = nullptr;   // the batch's BaseMap::flag when the column maps were made, else null
        int64_t n_fam = 0;
        bool writer = false, writer_ss = false;
        hipEvent_t ev_h2d = nullptr, ev_comp = nullptr, ev_d2h = nullptr;
        int *h_err = nullptr;     // pinned copy of the batch's capacity flag
        int32_t *h_fam_filt = nullptr;   // the caller's pinned fam_filt (dcr_slot_filter_out), or null
        dcr_metrics *h_metrics = nullptr;   // the caller's pinned counters (dcr_slot_metrics_out), or null
        dcr_base_metrics *h_base_metrics = nullptr;   // the same for dcr_slot_base_metrics_out
        dcr_genome_metrics *h_genome_metrics = nullptr;   // the same for dcr_slot_genome_metrics_out
        int32_t *h_fam_ovl = nullptr;    // the caller's pinned fam_ovl (dcr_slot_overlap_out), or null
        bool busy = false;
    } slots[DCR_MAX_SLOTS];
    dcr::Workspace w{};
    int64_t last_reads = 0;
    bool timed = false;
    int fast_ok = 0;    // fast_allowed(): the fast kernel may take records
    int options = 0;    // DCR_OPT_*
    int wide_ok = 0;    // the general kernel's decision pass may run (wide_table)
    dcr_params host_params{};
    dcr_filter filter{};    // dcr_set_filter; active == 0: off
    bool metrics = false;   // dcr_set_metrics
    dcr_base_filter base_filter{};   // dcr_set_base_filter; active == 0: off
    bool base_tags = false;          // dcr_set_base_tags
    bool base_metrics = false;       // dcr_set_base_metrics
    int mate_overlap = 0;            // dcr_set_mate_overlap: 0 off, DCR_OVL_MASK, DCR_OVL_CONSENSUS
    // dcr_set_allele_sites: the sorted keys and the table [n_allele][DCR_ALLELE_COLS] every slot's
    // k_allele_counts adds into; all null / 0: off
    int64_t *d_allele_keys = nullptr;
    unsigned long long *d_allele_tab = nullptr;
    int64_t n_allele = 0;
    int allele_min_q = 0;
    // dcr_set_genome: one code a base for n_ref sequences back to back and their offsets [n_ref + 1],
    // read by every slot's k_genome_metrics; all null / 0: off
    uint8_t *d_genome = nullptr;
    int64_t *d_ref_off = nullptr;
    int32_t n_ref = 0;
    // the column maps of the batch being submitted (submit_write sets them around its
    // dcr_run_batch when a base filter, the per-base tags or the base metrics are on); all null otherwise
    dcr::BaseMap bmap{};
    // fast-kernel constants (fast_constants)
    uint32_t fast_kq = 0, fast_kqlo = 0;
    int fast_maxq = 0, fast_t16 = 0, fast_r_safe = 0, fast_qlo = 0;
    int fast_t8 = 0, fast_narrow = 0;   // the common fast instantiation's narrow rows (1/8 nat)
    // single-strand records of at most this many reads skip the common fast
    // pass (the exact pass takes them whole); DCR_EXACT_DIRECT_R overrides
    int direct_r = 3;
    // the largest single-strand subfamily of the batch being submitted, when
    // the host knows it (dcr_submit / dcr_submit_write: host sub_off), else -1:
    // the kernels only records that large can need (k_prep_big > 64 reads,
    // k_decide_deep >= kDeepReads) are not launched for batches without them
    int max_r_hint = -1;
    uint16_t *d_llr16 = nullptr;   // device [128]
    uint16_t *d_llr8 = nullptr;    // device [128]
    uint32_t *d_r2tab = nullptr;   // device [dcr::kR2Entries]: two-read column outcomes (EXACT pass)
    double *d_e1000 = nullptr;     // device [1001]: k / 1000 (the fast kernel's E)
    uint32_t *d_wtab = nullptr;    // device [DCR_LUT_N] (general kernel's decision pass)
    int n_cu = 256;     // compute units (persistent grid size)
    int dfl_blocks = 1; // resident k_deflate workgroups per CU (dynamic LDS = sizeof(dfl::Shared))
    int fast_blocks[4] = {1, 1, 1, 1};   // resident k_consensus_fast blocks per CU (ss, ds; exact ss, exact ds)
};

// The fast kernel's assumptions (dcr_kernels.hip, fast kernel v2): every
// likelihood factor in [0, 1]; the quality formula reduces to e (no pre/post
// labelling error, :700-709); qualities fit a byte (:1383).  Otherwise every
// record takes the general kernel.
static int fast_allowed(const dcr_params *p) {
    for (int i = 0; i < DCR_LUT_N; ++i)
        if (!(p->match[i] >= 0.0 && p->match[i] <= 1.0 && p->mismatch[i] >= 0.0 && p->mismatch[i] <= 1.0))
            return 0;
    return p->error_rate_pre_labeling == 0 && p->error_rate_post_labeling == 0 && p->max_base_quality <= 255 &&
           p->min_base_quality <= 255;
}

// Host constants of the fast kernel's decision (dcr_kernels.hip, fast kernel v6):
//   llr16[q] = floor(16 ln(match[q] / mismatch[q]) - 1e-6)  (a lower bound; + 1 an upper one)
//   t16      = ceil(16 ln(5 / cc)) + 1,  cc = min(qthresh[maxQ], 1 - threshold, 1/4)
//   fast_qlo = the lowest quality from which every row has match >= mismatch > 0
//   r_safe   = the most reads R with R c_max <= 700 nats, c_max bounding -ln of either factor of
//              the rows a fast record can hold (q <= 122; the call's rows have q >= fast_qlo).
//              ln L_b >= -R c_max, so up to r_safe reads the call's likelihood stays a normal
//              double (e^-700 > DBL_MIN = e^-708.4).
//              Above it the reference's products can underflow to 0 (S = 0, NaN posterior, call
//              'A' :613), which the LLR bound does not see: every column then takes the exact path.
//   llrn[q], tn: the same in 1/u nat for the common fast instantiation's
//              narrow rows (dcr_kernels.hip, Evidence8: 15 rows of at most 273
//              fit 12 bits), u = 16 when every row fits (default parameters:
//              qualities capped at max_base_quality 60 give <= 246), else 8, else
//              4; narrow = 0 when none does (then that instantiation queues every
//              record for the EXACT one)
// Returns 0 when the decision cannot be made for these parameters (then every
// record takes the general kernel).
static int fast_constants(const dcr_params &hp, uint16_t llr16[128], uint16_t llr8[128], uint32_t &kq, uint32_t &kqlo,
                          int &maxq, int &t16, int &t8, int &narrow, int &r_safe, int &qlo_out) {
    const int mb = std::min(std::max(hp.min_base_quality, 0), 255);
    kq = (uint32_t)(255 - mb) * 0x01010101u;
    maxq = hp.max_base_quality;
    int qlo = 123;
    while (qlo > 0 && hp.mismatch[qlo - 1] > 0.0 && hp.match[qlo - 1] >= hp.mismatch[qlo - 1]) --qlo;
    kqlo = (uint32_t)(0x80 - qlo) * 0x01010101u;
    qlo_out = qlo;
    double lmax = 0.0;
    for (int q = 0; q < 128; ++q) {
        llr16[q] = 0;
        if (q >= qlo && q <= 122) {
            const double v = std::floor(16.0 * std::log(hp.match[q] / hp.mismatch[q]) - 1e-6);
            if (!(v <= 1040.0)) return 0;                  // 63 rows must fit a 16-bit field
            llr16[q] = (uint16_t)std::max(v, 0.0);
            lmax = std::max(lmax, std::log(hp.match[q] / hp.mismatch[q]));
        }
    }
    // the narrow rows' unit: 15 rows must fit 12 bits
    int un = 16;
    while (un > 4 && std::floor(un * lmax - 1e-6) > 273.0) un /= 2;
    narrow = std::floor(un * lmax - 1e-6) <= 273.0 ? 1 : 0;
    for (int q = 0; q < 128; ++q) {
        llr8[q] = 0;
        if (narrow && q >= qlo && q <= 122)
            llr8[q] = (uint16_t)std::max(std::floor(un * std::log(hp.match[q] / hp.mismatch[q]) - 1e-6), 0.0);
    }
    const int mq = std::min(std::max(hp.max_base_quality, 0), DCR_MAX_QTHRESH - 1);
    const double cc = std::min(std::min(hp.qthresh[mq], 1.0 - hp.post_threshold), 0.25);
    if (!(cc > 1e-12)) return 0;
    t16 = (int)std::ceil(16.0 * std::log(5.0 / cc)) + 1;
    t8 = (int)std::ceil(un * std::log(5.0 / cc)) + 1;
    double cmax = 0.0;                                 // per-row bound on -ln(factor), either factor
    for (int q = 0; q <= 122; ++q) {
        cmax = std::max(cmax, -std::log(hp.mismatch[q]));
        if (q >= qlo) cmax = std::max(cmax, -std::log(hp.match[q]));
    }
    r_safe = cmax > 0.0 ? (int)std::min(1e6, std::floor(700.0 / cmax)) : 1000000;
    return 1;
}

// The general kernel's decision pass (dcr_kernels.hip: decide_record) per LUT
// row v (quality byte, '+' 256, '-' 257):
//   bits 0-15   llr16 = floor(16 ln(match[v] / mismatch[v]) - 1e-6), a lower bound
//   bits 16-30  z16   = ceil(16 (-ln mismatch[v]) + 1e-6), an upper bound
//   bit 31      the row cannot be a call's row (quality above 122 or below fast_qlo; '+' / '-' with 1-p' < p'/5)
// Returns 0 when some z16 does not fit (then the pass is not used).
static int wide_table(const dcr_params &hp, uint32_t wtab[DCR_LUT_N]) {
    int qlo = 123;
    while (qlo > 0 && hp.mismatch[qlo - 1] > 0.0 && hp.match[qlo - 1] >= hp.mismatch[qlo - 1]) --qlo;
    for (int v = 0; v < DCR_LUT_N; ++v) {
        const double mm = hp.mismatch[v], m = hp.match[v];
        if (!(mm > 0.0)) return 0;
        const double z = std::ceil(-16.0 * std::log(mm) + 1e-6);
        if (!(z >= 0.0 && z <= 32767.0)) return 0;
        uint32_t w = (uint32_t)z << 16;
        const bool call_row = v >= DCR_LUT_PLUS ? m >= mm : (v >= qlo && v <= 122);   // '+', '-' rows
        if (call_row) {
            const double l = std::floor(16.0 * std::log(m / mm) - 1e-6);
            if (!(l <= 1040.0)) return 0;
            w |= (uint32_t)std::max(l, 0.0);
        } else {
            w |= 1u << 31;
        }
        wtab[v] = w;
    }
    return 1;
}

static int upload_fast(dcr_ctx *c, const dcr_params *params) {
    uint16_t llr[128], llr8[128];
    uint32_t wtab[DCR_LUT_N];
    const int ok = fast_constants(*params, llr, llr8, c->fast_kq, c->fast_kqlo, c->fast_maxq, c->fast_t16, c->fast_t8,
                                 c->fast_narrow, c->fast_r_safe, c->fast_qlo);
    c->fast_ok = fast_allowed(params) && ok;
    c->wide_ok = c->fast_ok && wide_table(*params, wtab);
    if (hipMemcpy(c->d_llr16, llr, sizeof(llr), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_llr8, llr8, sizeof(llr8), hipMemcpyHostToDevice) != hipSuccess ||
        (c->wide_ok && hipMemcpy(c->d_wtab, wtab, sizeof(wtab), hipMemcpyHostToDevice) != hipSuccess))
        return fail(DCR_EHIP, "fast-kernel table upload failed");
    // the two-read outcomes from the device parameters just uploaded, by the
    // EXACT pass's own products and posterior (bit-identical by construction)
    hipLaunchKernelGGL(dcr::k_r2_table, dim3((dcr::kR2Entries + 255) / 256), dim3(256), 0, c->stream, c->d_params,
                       c->d_r2tab);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(DCR_EHIP, "two-read table build failed");
    return DCR_OK;
}

// the fast kernel's arguments for one strand of a batch
static dcr::FastArgs fast_args(const dcr_ctx *c, bool duplex, const dcr_batch *in, const dcr_out *ss,
                               const dcr_out *ds) {
    dcr::FastArgs f{};
    f.gb = duplex ? ss->seq : in->bases;
    f.gq = duplex ? ss->qual : in->quals;
    f.nbytes = duplex ? in->ss_cols : in->n_bases;
    f.meta = c->w.meta;
    f.rows = c->w.rows;
    f.rmeta = c->w.rmeta;
    f.fast_count = c->w.fast_count + (duplex ? 1 : 0);
    f.info = c->w.info;
    f.norm_cig = c->w.norm_cig;
    f.cig_off = in->cig_off;
    f.ovf = c->w.ovf;
    f.ovf_count = c->w.ovf_count + (duplex ? 1 : 0);
    f.xlist = c->w.xlist;
    f.xcount = c->w.xcount + (duplex ? 1 : 0);
    f.O = duplex ? *ds : *ss;
    f.P = c->d_params;
    f.stamps = c->w.stamps;
    f.kq = c->fast_kq;
    f.kqlo = c->fast_kqlo;
    f.maxq = c->fast_maxq;
    f.t16 = c->fast_t16;
    f.r_safe = c->fast_r_safe;
    f.minbq = duplex ? -1 : c->host_params.min_base_quality;
    f.lo_check = duplex || c->host_params.min_base_quality < c->fast_qlo;
    f.llr16 = c->d_llr16;
    f.llr8 = c->d_llr8;
    f.r2tab = c->d_r2tab;
    f.t8 = c->fast_t8;
    f.narrow = c->fast_narrow;
    f.e1000 = c->d_e1000;
    {
        // record-scalar stores at 32-bit offsets from the lowest array
        // (k_consensus_fast): every array + its largest index within 4 GiB
        const dcr_out &O = f.O;
        const int64_t nrec = (duplex ? 2 : 4) * in->n_fam, ncol = duplex ? in->ds_cols : in->ss_cols;
        const uint8_t *p[10] = {(const uint8_t *)O.pos, (const uint8_t *)O.mapq, (const uint8_t *)O.len,
                                (const uint8_t *)O.n_cig, (const uint8_t *)O.n_de, (const uint8_t *)O.D,
                                (const uint8_t *)O.M, (const uint8_t *)O.E, (const uint8_t *)O.E + 4,
                                (const uint8_t *)O.cigar};
        const uint8_t *lo = p[0];
        for (int k = 1; k < 10; ++k) lo = std::min(lo, p[k]);
        bool ok = lo != nullptr;
        for (int k = 0; k < 10 && ok; ++k) {
            const uint64_t reach = (uint64_t)(p[k] - lo) + (k == 9 ? 4 * (uint64_t)ncol : (k == 7 || k == 8 ? 8 : 4) * (uint64_t)nrec);
            ok = p[k] != nullptr && reach < 0xFFFFFFF0ull;
            f.sofs[k] = (uint32_t)(p[k] - lo);
        }
        f.sbase = ok ? (uint8_t *)lo : nullptr;
    }
    f.want_info = (c->options & DCR_OPT_READ_INFO) ? 1 : 0;
    f.direct_r = duplex ? 0 : c->direct_r;
    return f;
}

// One strand of a batch: k_recmeta classifies every record (fast list /
// general list / status written), then the fast kernel (8 records per wave)
// drains the fast list and the persistent general kernel the rest
// (insertions, > 64 reads, wide layouts).  Events ev[0..3] of the strand.
template <bool DUPLEX>
static int launch_strand(dcr_ctx *c, dcr::Args &a, const dcr_batch *in, const dcr_out *ss, const dcr_out *ds) {
    a.n_rec = (DUPLEX ? 2LL : 4LL) * in->n_fam;
    const int64_t n_rec = a.n_rec;
    const dcr::FastArgs fa = fast_args(c, DUPLEX, in, ss, ds);
    auto grid_for = [&](unsigned cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n_rec + 3) / 4, cap)); };
    // k_recmeta: 64 records per wave, or fewer when the reads per record
    // exceed 16 on average (about 1,024 reads per wave)
    int rpw = 64;
    if (!DUPLEX && n_rec > 0) {
        const int64_t avg = (int64_t)in->n_reads / n_rec;
        while (rpw > 1 && (int64_t)rpw * avg > 1024) rpw >>= 1;
    }
    a.rpw = rpw;
    const int rm_waves = rpw == 64 ? dcr::kRecmetaWaves : 4;    // heavy records: small blocks
    const int64_t rpb = (int64_t)rm_waves * rpw;                // records per k_recmeta block
    const unsigned nb = (unsigned)((n_rec + rpb - 1) / rpb);
    hipEvent_t *ev = c->ev + (DUPLEX ? 5 : 1);
    // persistent fast kernel: the resident blocks (16 waves each), at least
    // ~8 records per wave
    const unsigned gf = (unsigned)std::max<int64_t>(
        1, std::min<int64_t>((n_rec + 127) / 128, (int64_t)c->fast_blocks[DUPLEX ? 1 : 0] * c->n_cu));
    // the exact queue is filled by the common kernel; its length is only
    // known on the device, so the exact kernel gets the resident grid
    const unsigned gx = (unsigned)((int64_t)c->fast_blocks[DUPLEX ? 3 : 2] * c->n_cu);
    hipLaunchKernelGGL(dcr::k_recmeta<DUPLEX>, dim3(nb), dim3(rm_waves * dcr::kWave), dcr::recmeta_lds_bytes(rm_waves),
                       c->stream, a);
    if constexpr (!DUPLEX)
        if (c->max_r_hint < 0 || c->max_r_hint > dcr::kWave)
            hipLaunchKernelGGL(dcr::k_prep_big, dim3(grid_for(2048)), dim3(256), 0, c->stream, a);
    HIP_TRY(hipEventRecord(ev[0], c->stream));
    hipLaunchKernelGGL((dcr::k_consensus_fast<DUPLEX, false>), dim3(gf), dim3(dcr::kFastBlock), 0, c->stream, fa);
    // k_fast_rows: one lane per fast-list entry (the list is at most n_rec long)
    hipLaunchKernelGGL(dcr::k_fast_rows, dim3((unsigned)std::max<int64_t>(1, (n_rec + 255) / 256)), dim3(256), 0,
                       c->stream, fa);
    HIP_TRY(hipEventRecord(ev[1], c->stream));
    hipLaunchKernelGGL((dcr::k_consensus_fast<DUPLEX, true>), dim3(gx), dim3(dcr::kFastBlock), 0, c->stream, fa);
    HIP_TRY(hipEventRecord(ev[2], c->stream));
    hipLaunchKernelGGL(dcr::k_decide<DUPLEX>, dim3(grid_for(2048)), dim3(256), 0, c->stream, a);
    // k_decide_deep only when the batch may hold a deep record (its 66 KB
    // blocks wait for room beside the inflate waves in the whole-node
    // pipeline even when they find none: up to 7 ms per C2 pass, profiles/r06g)
    if constexpr (!DUPLEX)
        if (c->max_r_hint < 0 || c->max_r_hint >= dcr::kDeepReads)
            hipLaunchKernelGGL(dcr::k_decide_deep, dim3(2 * c->n_cu), dim3(dcr::kDeepWaves * dcr::kWave), 0, c->stream, a);
    // after k_decide_deep: it reads the general list's entries, which
    // k_ins_layout marks decided (bit 31) for the records it decides
    hipLaunchKernelGGL(dcr::k_ins_layout<DUPLEX>, dim3(grid_for(2048)), dim3(256), 0, c->stream, a);
    // with a base filter, the per-base tags or the base metrics on, the instantiation that also stores the base maps
    if (c->bmap.flag)
        hipLaunchKernelGGL(dcr::k_consensus_general_map<DUPLEX>, dim3(grid_for(1024)), dim3(256), 0, c->stream, a, c->bmap);
    else
        hipLaunchKernelGGL(dcr::k_consensus_general<DUPLEX>, dim3(grid_for(1024)), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[3], c->stream));
    return DCR_OK;
}

extern "C" {

int dcr_abi_version(void) { return DCR_ABI_VERSION; }

const char *dcr_last_error(void) { return g_err.c_str(); }

static int check_params(const dcr_params *p) {
    if (!p) return fail(DCR_EARG, "params is NULL");
    if (p->max_base_quality < 0 || p->max_base_quality > DCR_MAX_QTHRESH - 1)
        return fail(DCR_EARG, "max_base_quality out of range [0, 256]");
    if (p->n_qthresh != p->max_base_quality + 1)
        return fail(DCR_EARG, "n_qthresh must equal max_base_quality + 1");
    return DCR_OK;
}

dcr_ctx *dcr_create(int device, const dcr_params *params) {
    if (check_params(params) != DCR_OK) return nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        fail(DCR_ENODEV, "no HIP device " + std::to_string(device));
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(DCR_ENODEV, std::string("device is not gfx950 (MI355X): ") + prop.gcnArchName);
        return nullptr;
    }
    dcr_ctx *c = new dcr_ctx();
    c->device = device;
    if (const char *e = std::getenv("DCR_EXACT_DIRECT_R")) c->direct_r = std::atoi(e);   // A/B runs
    if (hipSetDevice(device) != hipSuccess ||
        hi_prio_stream(&c->stream) != hipSuccess ||
        hipMalloc(&c->d_params, sizeof(dcr_params)) != hipSuccess ||
        hipMalloc(&c->d_llr16, 128 * sizeof(uint16_t)) != hipSuccess ||
        hipMalloc(&c->d_llr8, 128 * sizeof(uint16_t)) != hipSuccess ||
        hipMalloc(&c->d_r2tab, dcr::kR2Entries * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&c->d_e1000, 1001 * sizeof(double)) != hipSuccess ||
        hipMalloc(&c->d_wtab, DCR_LUT_N * sizeof(uint32_t)) != hipSuccess) {
        fail(DCR_EHIP, "context allocation failed");
        delete c;
        return nullptr;
    }
    for (auto &e : c->ev) (void)hipEventCreate(&e);
    (void)hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device);
    // the persistent fast kernel's grid = what is resident at once (a block
    // beyond that would start only when a resident one has finished its range)
    const void *fk[4] = {(const void *)dcr::k_consensus_fast<false, false>, (const void *)dcr::k_consensus_fast<true, false>,
                         (const void *)dcr::k_consensus_fast<false, true>, (const void *)dcr::k_consensus_fast<true, true>};
    for (int k = 0; k < 4; ++k)
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->fast_blocks[k], fk[k], dcr::kFastBlock, 0) != hipSuccess ||
            c->fast_blocks[k] < 1)
            c->fast_blocks[k] = 1;
    if (hipFuncSetAttribute((const void *)dcrw::k_deflate, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)sizeof(dfl::Shared)) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&c->dfl_blocks, dcrw::k_deflate, dfl::kT, sizeof(dfl::Shared)) !=
            hipSuccess ||
        c->dfl_blocks < 1)
        c->dfl_blocks = 1;
    c->host_params = *params;
    double e1000[1001];
    for (int k = 0; k <= 1000; ++k) e1000[k] = (double)k / 1000.0;   // IEEE division: numpy's rint(x)/1000
    if (hipMemcpy(c->d_params, params, sizeof(dcr_params), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_e1000, e1000, sizeof(e1000), hipMemcpyHostToDevice) != hipSuccess ||
        upload_fast(c, params) != DCR_OK) {
        fail(DCR_EHIP, "params upload failed");
        dcr_destroy(c);
        return nullptr;
    }
    return c;
}

void dcr_destroy(dcr_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    c->ws.release();
    c->io.release();
    for (auto &S : c->slots) {
        if (S.ev_d2h) (void)hipEventSynchronize(S.ev_d2h);
        S.buf.release();
        S.wbuf.release();
        if (S.ev_h2d) (void)hipEventDestroy(S.ev_h2d);
        if (S.ev_comp) (void)hipEventDestroy(S.ev_comp);
        if (S.ev_d2h) (void)hipEventDestroy(S.ev_d2h);
        if (S.h_err) (void)hipHostFree(S.h_err);
    }
    if (c->s_h2d) (void)hipStreamDestroy(c->s_h2d);
    if (c->s_d2h) (void)hipStreamDestroy(c->s_d2h);
    if (c->s_fetch) (void)hipStreamDestroy(c->s_fetch);
    if (c->ev_fetch) (void)hipEventDestroy(c->ev_fetch);
    if (c->d_params) (void)hipFree(c->d_params);
    if (c->d_llr16) (void)hipFree(c->d_llr16);
    if (c->d_llr8) (void)hipFree(c->d_llr8);
    if (c->d_r2tab) (void)hipFree(c->d_r2tab);
    if (c->d_e1000) (void)hipFree(c->d_e1000);
    if (c->d_wtab) (void)hipFree(c->d_wtab);
    if (c->d_allele_keys) (void)hipFree(c->d_allele_keys);
    if (c->d_allele_tab) (void)hipFree(c->d_allele_tab);
    if (c->d_genome) (void)hipFree(c->d_genome);
    if (c->d_ref_off) (void)hipFree(c->d_ref_off);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int dcr_set_params(dcr_ctx *c, const dcr_params *params) {
    if (!c) return fail(DCR_EARG, "ctx is NULL");
    int rc = check_params(params);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->d_params, params, sizeof(dcr_params), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->host_params = *params;
    return upload_fast(c, params);
}

void *dcr_stream(dcr_ctx *c) { return c ? (void *)c->stream : nullptr; }

int dcr_set_options(dcr_ctx *c, int flags) {
    if (!c) return fail(DCR_EARG, "ctx is NULL");
    if (flags & ~DCR_OPT_READ_INFO) return fail(DCR_EARG, "unknown option");
    c->options = flags;
    return DCR_OK;
}

int dcr_reserve(dcr_ctx *c, const dcr_batch *s) {
    if (!c || !s) return fail(DCR_EARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    Plan sz;
    dcr::Workspace unused;
    plan_workspace(*s, sz, unused);
    if (sz.off > c->ws.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->ws.ensure(sz.off + sz.off / 8));
    }
    Plan p{(char *)c->ws.p};
    plan_workspace(*s, p, c->w);
    return DCR_OK;
}

int dcr_run_batch(dcr_ctx *c, const dcr_batch *in, dcr_out *ss, dcr_out *ds) {
    if (!c || !in || !ss || !ds) return fail(DCR_EARG, "NULL argument");
    if (in->n_fam < 0 || in->n_reads < 0) return fail(DCR_EARG, "negative batch size");
    int rc = dcr_reserve(c, in);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->w.err, 0, 64, c->stream));   // dcr::Counters
    c->last_reads = in->n_reads;
    // per-read preprocessing (:191-325) is fused: k_recmeta<ss> analyses the
    // clips and fully preprocesses the reads of records the fast kernel does
    // not take; the fast kernel does the 3' trim of its own records
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    dcr::Args a;
    a.in = *in;
    a.P = c->d_params;
    std::memcpy(&a.ws, &c->w, sizeof(a.ws));
    a.ss = *ss;
    a.ds = *ds;
    a.fast_ok = c->fast_ok;
    a.t16 = c->wide_ok ? c->fast_t16 : -1;     // -1: no decision pass
    a.wtab = c->d_wtab;
    if (in->n_fam > 0) {
        if ((rc = launch_strand<false>(c, a, in, ss, ds))) return rc;
        if ((rc = launch_strand<true>(c, a, in, ss, ds))) return rc;
    } else {
        for (int k = 1; k <= DCR_N_KERNEL_TIMES; ++k) HIP_TRY(hipEventRecord(c->ev[k], c->stream));
    }
    c->timed = true;
    return DCR_OK;
}

int dcr_sync(dcr_ctx *c) {
    if (!c) return fail(DCR_EARG, "ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->w.err) {
        int err = 0;
        HIP_TRY(hipMemcpy(&err, c->w.err, sizeof(int), hipMemcpyDeviceToHost));
        if (err) return fail(DCR_ECAPACITY, "a consensus needed more columns than its output region");
    }
    return DCR_OK;
}

int dcr_last_timing(dcr_ctx *c, float *ms4) {
    if (!c || !ms4) return fail(DCR_EARG, "NULL argument");
    if (!c->timed) return fail(DCR_EARG, "no batch has run");
    const int last = DCR_N_KERNEL_TIMES;
    HIP_TRY(hipEventSynchronize(c->ev[last]));
    ms4[0] = 0.0f;                       // preprocessing is fused into k_recmeta / the fast kernel
    HIP_TRY(hipEventElapsedTime(&ms4[1], c->ev[0], c->ev[4]));
    HIP_TRY(hipEventElapsedTime(&ms4[2], c->ev[4], c->ev[last]));
    HIP_TRY(hipEventElapsedTime(&ms4[3], c->ev[0], c->ev[last]));
    return DCR_OK;
}

// diagnostic (not in include/dcr.h): phase cycle counters of DCR_STAMP builds
int dcr_debug_stamps(dcr_ctx *c, unsigned long long *out, int n, int reset) {
    if (!c || !out || n > 64) return fail(DCR_EARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->w.stamps, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(c->w.stamps, 0, sizeof(unsigned long long) * 64));
    return DCR_OK;
}

// diagnostic (not in include/dcr.h): the last batch's queue counters -- err,
// ovf_count[2], fast_count[2], xcount[2] (exact queue), gen_next[2], deep_count
int dcr_debug_counts(dcr_ctx *c, int *out10) {
    if (!c || !out10) return fail(DCR_EARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out10, c->w.err, sizeof(int) * 10, hipMemcpyDeviceToHost));
    return DCR_OK;
}

int dcr_last_kernel_timing(dcr_ctx *c, float *ms) {
    if (!c || !ms) return fail(DCR_EARG, "NULL argument");
    if (!c->timed) return fail(DCR_EARG, "no batch has run");
    HIP_TRY(hipEventSynchronize(c->ev[DCR_N_KERNEL_TIMES]));
    for (int k = 0; k < DCR_N_KERNEL_TIMES; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], c->ev[k], c->ev[k + 1]));
    return DCR_OK;
}

int dcr_read_info_host(dcr_ctx *c, dcr_read_info *out, int64_t n) {
    if (!c || !out) return fail(DCR_EARG, "NULL argument");
    if (n > c->last_reads) return fail(DCR_EARG, "more reads requested than the last batch held");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n > 0) HIP_TRY(hipMemcpy(out, c->w.info, sizeof(dcr_read_info) * n, hipMemcpyDeviceToHost));
    return DCR_OK;
}

// host-pointer entry point: one staging allocation, H2D, run, D2H
int dcr_run_batch_host(dcr_ctx *c, const dcr_batch *h, dcr_out *hss, dcr_out *hds) {
    if (!c || !h || !hss || !hds) return fail(DCR_EARG, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = io_bytes(h);
    if (need > c->io.cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(c->io.ensure(need));
    }
    dcr_batch db;
    dcr_out dout[2];
    Plan p{(char *)c->io.p};
    plan_io(h, p, &db, dout);
    HIP_TRY(upload_inputs(h, db, c->stream));
    int rc = dcr_run_batch(c, &db, &dout[0], &dout[1]);
    if (rc) return rc;
    HIP_TRY(download_outputs(&dout[0], hss, 4 * (int64_t)h->n_fam, h->ss_cols, c->stream));
    HIP_TRY(download_outputs(&dout[1], hds, 2 * (int64_t)h->n_fam, h->ds_cols, c->stream));
    return dcr_sync(c);
}

// ---- streaming (pinned host batches, per-slot device buffers, copy streams) ----

void *dcr_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
        g_err = "hipHostMalloc failed";
        return nullptr;
    }
    return p;
}

void dcr_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

// the largest subfamily of a host batch (sub_off is a host array here)
static int host_max_r(const dcr_batch *h) {
    int m = 0;
    const int64_t n = 4 * (int64_t)h->n_fam;
    if (n > 0 && !h->sub_off) return -1;
    for (int64_t i = 0; i < n; ++i) m = std::max(m, h->sub_off[i + 1] - h->sub_off[i]);
    return m;
}

// The front of a submit: the copy streams, the slot's events and pinned flag
// (all created on first use), and the slot must be idle.
static int slot_open(dcr_ctx *c, int slot, dcr_ctx::Slot **out) {
    if (slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "slot out of range");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->s_h2d) {
        HIP_TRY(hi_prio_stream(&c->s_h2d));
        HIP_TRY(hi_prio_stream(&c->s_d2h));
        HIP_TRY(hi_prio_stream(&c->s_fetch));
    }
    dcr_ctx::Slot &S = c->slots[slot];
    if (!S.ev_h2d) {
        HIP_TRY(hipEventCreateWithFlags(&S.ev_h2d, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&S.ev_comp, hipEventDisableTiming));
        // the host waits on this one (dcr_wait / dcr_wait_write): blocking, so the
        // waiting thread sleeps instead of spinning on a core the ingest needs
        HIP_TRY(hipEventCreateWithFlags(&S.ev_d2h, hipEventDisableTiming | hipEventBlockingSync));
        HIP_TRY(hipHostMalloc((void **)&S.h_err, sizeof(int), hipHostMallocDefault));
        *S.h_err = 0;
    }
    if (S.busy) return fail(DCR_EARG, "slot still in flight (dcr_wait it first)");
    *out = &S;
    return DCR_OK;
}

// After the slot's uploads are enqueued on s_h2d: the consensus kernels on the
// compute stream once the uploads are done, then the capacity flag.
static int slot_run(dcr_ctx *c, dcr_ctx::Slot &S, const dcr_batch *h, dcr_batch *db, dcr_out dout[2]) {
    HIP_TRY(hipEventRecord(S.ev_h2d, c->s_h2d));
    HIP_TRY(hipStreamWaitEvent(c->stream, S.ev_h2d, 0));
    c->max_r_hint = host_max_r(h);
    const int rc = dcr_run_batch(c, db, &dout[0], &dout[1]);
    c->max_r_hint = -1;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(S.h_err, c->w.err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    return DCR_OK;
}

int dcr_submit(dcr_ctx *c, int slot, const dcr_batch *h, dcr_out *hss, dcr_out *hds, int32_t *read_status) {
    if (!c || !h || !hss || !hds) return fail(DCR_EARG, "NULL argument");
    dcr_ctx::Slot *Sp = nullptr;
    int rc = slot_open(c, slot, &Sp);
    if (rc) return rc;
    dcr_ctx::Slot &S = *Sp;
    const size_t need = io_bytes(h);
    if (need > S.buf.cap) HIP_TRY(S.buf.ensure(need + need / 8));   // idle slot: nothing in flight uses it
    dcr_batch db;
    dcr_out dout[2];
    Plan p{(char *)S.buf.p};
    plan_io(h, p, &db, dout);
    HIP_TRY(upload_inputs(h, db, c->s_h2d));
    if ((rc = slot_run(c, S, h, &db, dout))) return rc;
    if (read_status && h->n_reads > 0)
        HIP_TRY(hipMemcpy2DAsync(read_status, sizeof(int32_t), (const char *)c->w.info + offsetof(dcr_read_info, status),
                                 sizeof(dcr_read_info), sizeof(int32_t), (size_t)h->n_reads, hipMemcpyDeviceToHost,
                                 c->stream));
    HIP_TRY(hipEventRecord(S.ev_comp, c->stream));
    // D2H of the outputs on the second copy stream
    HIP_TRY(hipStreamWaitEvent(c->s_d2h, S.ev_comp, 0));
    HIP_TRY(download_outputs(&dout[0], hss, 4 * (int64_t)h->n_fam, h->ss_cols, c->s_d2h));
    HIP_TRY(download_outputs(&dout[1], hds, 2 * (int64_t)h->n_fam, h->ds_cols, c->s_d2h));
    HIP_TRY(hipEventRecord(S.ev_d2h, c->s_d2h));
    S.writer = false;
    S.writer_ss = false;
    S.busy = true;
    return DCR_OK;
}

int dcr_wait(dcr_ctx *c, int slot) {
    if (!c || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    dcr_ctx::Slot &S = c->slots[slot];
    if (!S.busy) return DCR_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(S.ev_d2h));
    S.busy = false;
    if (*S.h_err) return fail(DCR_ECAPACITY, "a consensus needed more columns than its output region");
    return DCR_OK;
}


// ---- device record writer ----------------------------------------------------

// Upper bound of the formatted duplex records of a batch (dcr_writer.hip
// rec_size): regions bound lengths, CIGARs and depth lists.  Per record, with
// Td / Ta / Tb the columns of its own and its two strands' regions:
//   fixed parts  36 core + 29 + lc name + (4 + lc) MI + (4 + lr) RX + 26 + reads
//                aQ bQ cQ + at most 42 aD..cM + 21 aE..cE + the heads of the ten
//                per-column tags (at most 6 * 8 + 4 * 4 = 64): under 400 + 2 lc +
//                lr + reads
//   default      per column of Td 4 CIGAR + 1.5 SEQ / QUAL + 2 * 7 of the cd /
//                ce list entries ("65535, "): 19.5 <= 20; per column of Ta / Tb
//                2 * 7 of ad / ae + 2 of ac / aq: 16
//   tags         (rec_size_tags) len <= Td bases and n_cig <= Td: 4 CIGAR + 0.5 +
//                1 SEQ / QUAL (+ 0.5 for an odd len) + 6 * 2 of the B:s arrays + 4
//                of the strings = 21.5 Td + 0.5 <= 22 Td; nothing per strand column
// Neither bound can be exceeded by a batch whose records stay inside their
// regions (the kernels raise DCR_ECAPACITY otherwise).  The compressed blocks
// are another matter: the caller's cap_bgzf is checked against totals[0] in
// fetch_blocks, and a slot whose blocks do not fit is fetched again
// (dcr_slot_fetch what 2 / 5); tagged records take that path like any other.
static int64_t stream_bound(const dcr_batch *h, const dcr_wmeta *m, bool tags) {
    int64_t B = 0;
    for (int32_t f = 0; f < h->n_fam; ++f) {
        const int64_t lc = (int64_t)std::strlen(m->names + m->fam_code[f]);
        for (int j = 0; j < 2; ++j) {
            const int a = 4 * f + 2 * j, b = a + 1;
            const int64_t Td = h->ds_col_off[2 * f + j + 1] - h->ds_col_off[2 * f + j];
            const int64_t Ta = h->ss_col_off[a + 1] - h->ss_col_off[a];
            const int64_t Tb = h->ss_col_off[b + 1] - h->ss_col_off[b];
            const int64_t lr = (int64_t)std::strlen(m->names + m->fam_rx[2 * f + j]);
            B += 400 + 2 * lc + lr + (tags ? 22 * Td : 20 * Td + 16 * (Ta + Tb)) + (h->sub_off[a + 1] - h->sub_off[a]) +
                 (h->sub_off[b + 1] - h->sub_off[b]);
        }
    }
    return B;
}

// Upper bound of the formatted single-strand records of a batch
// (dcr_writer.hip rec_size_ss): per column of the region at most 4 bytes of
// CIGAR, 1.5 of sequence and quality and 7 + 7 of the two depth lists: 19.5 <=
// 20.  With the per-base tags (rec_size_ss_tags) the lists are two B:s arrays
// of len <= T entries: 4 + 1.5 + 2 * 2 = 9.5 T + 0.5 <= 10 T; the fixed parts
// (36 + 20 + lc + 8 + lmi + lrx + 8 + reads + 14 sD sM + 7 sE + 16 array
// heads = 109 + ...) stay under 160 either way.
static int64_t stream_bound_ss(const dcr_batch *h, const dcr_wmeta *m, const dcr_wmeta_ss *ms, bool tags) {
    int64_t B = 0;
    for (int32_t f = 0; f < h->n_fam; ++f) {
        const int64_t lc = (int64_t)std::strlen(m->names + m->fam_code[f]);
        for (int s = 4 * f; s < 4 * f + 4; ++s)
            B += 160 + lc + (int64_t)std::strlen(m->names + ms->sub_mi[s]) + (int64_t)std::strlen(m->names + ms->sub_rx[s]) +
                 (tags ? 10 : 20) * (h->ss_col_off[s + 1] - h->ss_col_off[s]) + (h->sub_off[s + 1] - h->sub_off[s]);
    }
    return B;
}

// dcr_submit_write, and with ms / res_ss dcr_submit_write_ss: the same
// launches and copies, then the single-strand stream's
static int submit_write(dcr_ctx *c, int slot, const dcr_batch *h, const dcr_wmeta *m, const dcr_wmeta_ss *ms,
                        dcr_wres *res, dcr_wres *res_ss) {
    dcr_ctx::Slot *Sp = nullptr;
    int rc = slot_open(c, slot, &Sp);
    if (rc) return rc;
    dcr_ctx::Slot &S = *Sp;
    const int64_t F = h->n_fam;
    // consensus buffers
    const size_t need = io_bytes(h);
    if (need > S.buf.cap) HIP_TRY(S.buf.ensure(need + need / 8));
    dcr_batch db;
    dcr_out dout[2];
    Plan p{(char *)S.buf.p};
    plan_io(h, p, &db, dout);
    // writer buffers
    const bool btags = c->base_tags;
    const int64_t B = stream_bound(h, m, btags);
    const int64_t nbm = B / (int64_t)dfl::kMaxIn + 2;
    const unsigned gd = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nbm, (int64_t)c->n_cu * c->dfl_blocks));
    WriterBufs wb;
    WriterSsBufs wsb{};
    if (ms) {
        wsb.B = stream_bound_ss(h, m, ms, btags);
        wsb.nbm = wsb.B / (int64_t)dfl::kMaxIn + 2;
        wsb.gd = (unsigned)std::max<int64_t>(1, std::min<int64_t>(wsb.nbm, (int64_t)c->n_cu * c->dfl_blocks));
    }
    // a base filter alone still gives fam_filt: k_filter runs to add the masked counts into it
    const bool bfilt = c->base_filter.active != 0;
    const bool filt = c->filter.active != 0 || bfilt;
    const bool bmet = c->base_metrics;
    const bool maps = bfilt || btags || bmet;   // the column maps: planned, zeroed and filled for any of them
    if (filt && F && !S.h_fam_filt)
        return fail(DCR_EARG, "a filter is set but the slot has no fam_filt destination (dcr_slot_filter_out)");
    const bool met = c->metrics;
    if (met && !S.h_metrics)
        return fail(DCR_EARG, "metrics are on but the slot has no destination (dcr_slot_metrics_out)");
    if (bmet && !S.h_base_metrics)
        return fail(DCR_EARG, "base metrics are on but the slot has no destination (dcr_slot_base_metrics_out)");
    const bool ovl = c->mate_overlap != 0;
    if (ovl && F && !S.h_fam_ovl)
        return fail(DCR_EARG, "a mate overlap mode is set but the slot has no fam_ovl destination (dcr_slot_overlap_out)");
    const bool gmet = c->n_ref != 0;
    if (gmet && !S.h_genome_metrics)
        return fail(DCR_EARG, "a genome is set but the slot has no destination (dcr_slot_genome_metrics_out)");
    Plan wsz;
    plan_writer(F, m->n_names, B, nbm, gd, wsz, wb, ms ? &wsb : nullptr, filt, met, maps ? h : nullptr, bfilt, bmet,
                ovl, gmet);
    if (wsz.off > S.wbuf.cap) HIP_TRY(S.wbuf.ensure(wsz.off + wsz.off / 8));
    Plan wp{(char *)S.wbuf.p};
    plan_writer(F, m->n_names, B, nbm, gd, wp, wb, ms ? &wsb : nullptr, filt, met, maps ? h : nullptr, bfilt, bmet,
                ovl, gmet);
    // H2D: inputs and writer metadata on the copy stream
    HIP_TRY(upload_inputs(h, db, c->s_h2d));
    if (m->n_names) HIP_TRY(hipMemcpyAsync(wb.names, m->names, (size_t)m->n_names, hipMemcpyHostToDevice, c->s_h2d));
    if (F) {
        HIP_TRY(hipMemcpyAsync(wb.fam_code, m->fam_code, 8 * (size_t)F, hipMemcpyHostToDevice, c->s_h2d));
        HIP_TRY(hipMemcpyAsync(wb.fam_rx, m->fam_rx, 16 * (size_t)F, hipMemcpyHostToDevice, c->s_h2d));
        HIP_TRY(hipMemcpyAsync(wb.fam_tid, m->fam_tid, 4 * (size_t)F, hipMemcpyHostToDevice, c->s_h2d));
    }
    if (ms && F) {
        HIP_TRY(hipMemcpyAsync(wsb.sub_flag, ms->sub_flag, 8 * (size_t)F, hipMemcpyHostToDevice, c->s_h2d));
        HIP_TRY(hipMemcpyAsync(wsb.sub_mi, ms->sub_mi, 32 * (size_t)F, hipMemcpyHostToDevice, c->s_h2d));
        HIP_TRY(hipMemcpyAsync(wsb.sub_rx, ms->sub_rx, 32 * (size_t)F, hipMemcpyHostToDevice, c->s_h2d));
    }
    // with a base filter, the per-base tags or the base metrics the general kernels store the column maps
    // of the records with insertion columns and flag them; the flags start from zero for every batch
    if (maps && F) HIP_TRY(hipMemsetAsync(wb.bmap.flag, 0, 6 * (size_t)F, c->stream));
    c->bmap = wb.bmap;
    rc = slot_run(c, S, h, &db, dout);
    c->bmap = dcr::BaseMap{};
    if (rc) return rc;
    // record writer
    dcrw::FmtArgs A{};
    A.ss = dout[0];
    A.ds = dout[1];
    A.sub_off = db.sub_off;
    A.read_mapq = db.read_mapq;
    A.ss_col_off = db.ss_col_off;
    A.ds_col_off = db.ds_col_off;
    A.info = c->w.info;
    A.names = wb.names;
    A.fam_code = wb.fam_code;
    A.fam_rx = wb.fam_rx;
    A.fam_tid = wb.fam_tid;
    A.n_fam = (int32_t)F;
    A.fam_fail = wb.fam_fail;
    A.ds_len_out = wb.ds_len;
    A.rec_size = wb.rec_size;
    A.rec_off = wb.rec_off;
    A.stream = wb.stream;
    A.fam_filt = wb.fam_filt;
    HIP_TRY(hipMemsetAsync(wb.rec_size, 0, 8 * (size_t)(2 * F + 1), c->stream));
    HIP_TRY(hipMemsetAsync(wb.bsz, 0, 8 * (size_t)(nbm + 2), c->stream));
    // the slot's counters start from zero for every batch (an empty batch gives zeros)
    if (met) HIP_TRY(hipMemsetAsync(wb.metrics, 0, sizeof(dcr_metrics), c->stream));
    if (bmet) HIP_TRY(hipMemsetAsync(wb.base_metrics, 0, sizeof(dcr_base_metrics), c->stream));
    if (gmet) HIP_TRY(hipMemsetAsync(wb.genome_metrics, 0, sizeof(dcr_genome_metrics), c->stream));
    if (F) {
        hipLaunchKernelGGL(dcrw::k_famfail, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, c->stream, A);
        if (met) {
            // one wave per family, before k_filter masks the duplex seq / qual; at most one
            // workgroup per CU: every workgroup ends with a global add per non-zero bin
            dcrw::MetricsArgs Ma{dout[0], dout[1], db.sub_off, db.ss_col_off, db.ds_col_off, wb.fam_fail, (int32_t)F,
                                 wb.metrics};
            const int wpg = dcrw::kMetThreads / 64;
            const unsigned gm = (unsigned)std::max<int64_t>(1, std::min<int64_t>((F + wpg - 1) / wpg, (int64_t)c->n_cu));
            hipLaunchKernelGGL(dcrw::k_metrics, dim3(gm), dim3(dcrw::kMetThreads), 0, c->stream, Ma);
        }
        if (bmet) {
            // one wave per duplex record, after k_metrics and before the filters mask the duplex seq /
            // qual; at most one workgroup per CU: every workgroup ends with a global add per non-zero
            // bin.  A launch's 32-bit LDS bins take one per base: families are launched in ranges whose
            // duplex regions (which bound len, itself an int32) hold fewer than 2^32 columns, one range
            // for every batch but an enormous one
            dcrw::BaseMetricsArgs Ba{dout[0], dout[1], db.sub_off, db.read_pos, db.ss_col_off, db.ds_col_off,
                                     wb.fam_fail, wb.bmap.ss_col, wb.bmap.ds_col, wb.bmap.ds_aln, wb.bmap.flag,
                                     (int32_t)F, 0, 0, wb.base_metrics};
            const int wpg = dcrw::kBmThreads / 64;
            const int64_t lim = (int64_t)1 << 32, rmax = 0x7fffffff;
            for (int64_t f0 = 0; f0 < F;) {
                int64_t f1 = F;
                if (h->ds_cols >= lim) {
                    int64_t cols = 0;
                    for (f1 = f0; f1 < F; ++f1) {
                        const int64_t n = std::min(h->ds_col_off[2 * f1 + 1] - h->ds_col_off[2 * f1], rmax) +
                                          std::min(h->ds_col_off[2 * f1 + 2] - h->ds_col_off[2 * f1 + 1], rmax);
                        if (cols + n >= lim) break;
                        cols += n;
                    }
                }
                Ba.f0 = (int32_t)f0;
                Ba.f1 = (int32_t)f1;
                const unsigned gb = (unsigned)std::max<int64_t>(
                    1, std::min<int64_t>((2 * (f1 - f0) + wpg - 1) / wpg, (int64_t)c->n_cu));
                hipLaunchKernelGGL(dcrw::k_base_metrics, dim3(gb), dim3(dcrw::kBmThreads), 0, c->stream, Ba);
                f0 = f1;
            }
        }
        if (gmet) {
            // one wave per record, the single-strand level and then the duplex level, in k_base_metrics'
            // place: before k_mate_overlap and the filters rewrite the duplex seq / qual.  At most one
            // workgroup per CU (each ends with a global add per non-zero bin).  A launch's 32-bit LDS bins
            // take at most one per base: the records are launched in ranges whose regions hold fewer
            // than 2^32 columns, one range for every batch but an enormous one
            const int wpg = dcrw::kGmThreads / 64;
            const int64_t lim = (int64_t)1 << 32;
            for (int lv = 0; lv < 2; ++lv) {
                const int per = lv == 0 ? 4 : 2;
                const int64_t *off = lv == 0 ? h->ss_col_off : h->ds_col_off;
                const int64_t cols = lv == 0 ? h->ss_cols : h->ds_cols;
                dcrw::GenomeMetricsArgs Ga{dout[lv], lv == 0 ? db.ss_col_off : db.ds_col_off, wb.fam_fail, wb.fam_tid,
                                           c->d_genome, c->d_ref_off, c->n_ref, lv, 0, 0, wb.genome_metrics};
                for (int64_t r0 = 0; r0 < per * F;) {
                    int64_t r1 = per * F;
                    if (cols >= lim) {
                        // at least one record a launch: its len is an int32, below 2^32 whatever its region
                        for (r1 = r0 + 1; r1 < per * F && off[r1 + 1] - off[r0] < lim; ++r1) {}
                    }
                    Ga.r0 = r0;
                    Ga.r1 = r1;
                    const unsigned gg = (unsigned)std::max<int64_t>(
                        1, std::min<int64_t>((r1 - r0 + wpg - 1) / wpg, (int64_t)c->n_cu));
                    hipLaunchKernelGGL(dcrw::k_genome_metrics, dim3(gg), dim3(dcrw::kGmThreads), 0, c->stream, Ga);
                    r0 = r1;
                }
            }
        }
        if (ovl) {
            // one wave per family, after the QC tables (they describe the consensus as called) and
            // before the filters, which see the two mates as this step leaves them
            dcrw::MateOverlapArgs Oa{dout[1], db.ds_col_off, wb.fam_fail, wb.fam_ovl, (int32_t)F, c->mate_overlap};
            const unsigned go = (unsigned)std::max<int64_t>(1, std::min<int64_t>((F + 3) / 4, (int64_t)c->n_cu * 8));
            hipLaunchKernelGGL(dcrw::k_mate_overlap, dim3(go), dim3(256), 0, c->stream, Oa);
        }
        if (filt) {
            // one wave per family, before anything reads the duplex seq / qual
            const unsigned gf = (unsigned)std::max<int64_t>(1, std::min<int64_t>((F + 3) / 4, (int64_t)c->n_cu * 8));
            if (bfilt) {
                // after k_metrics (the tables describe the consensus as called), before k_filter
                // (its record rules see the bases masked here); the bases k_filter's own
                // quality rule masks are left to it, so every masked base is counted once
                const bool mq = (c->filter.active & DCR_FILT_MASK_BASES) != 0;
                dcrw::BaseFilterArgs Ba{dout[0], dout[1], db.sub_off, db.read_pos, db.ss_col_off, db.ds_col_off,
                                        wb.fam_fail, wb.bmap.ss_col, wb.bmap.ds_col, wb.bmap.ds_aln, wb.bmap.flag,
                                        wb.base_masked, (int32_t)F,
                                        mq ? std::min<int32_t>(c->filter.min_base_quality, 256) : 0, c->base_filter};
                hipLaunchKernelGGL(dcrw::k_base_filter, dim3(gf), dim3(256), 0, c->stream, Ba);
            }
            dcrw::FilterArgs Fa{dout[0], dout[1], db.ds_col_off, wb.fam_fail, wb.fam_filt, (int32_t)F, c->filter,
                                wb.base_masked};
            hipLaunchKernelGGL(dcrw::k_filter, dim3(gf), dim3(256), 0, c->stream, Fa);
        }
        if (c->n_allele) {
            // one wave per family, after the last kernel that rewrites or drops a duplex record: it
            // counts the records as they will be written, into the context's table
            dcrw::AlleleArgs Aa{dout[1], db.ds_col_off, wb.fam_fail, wb.fam_filt, wb.fam_tid, c->d_allele_keys,
                                c->d_allele_tab, c->n_allele, (int32_t)F, c->allele_min_q};
            const unsigned ga = (unsigned)std::max<int64_t>(1, std::min<int64_t>((F + 3) / 4, (int64_t)c->n_cu * 8));
            hipLaunchKernelGGL(dcrw::k_allele_counts, dim3(ga), dim3(256), 0, c->stream, Aa);
        }
        const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((2 * F + 3) / 4, (int64_t)c->n_cu * 8));
        if (btags)
            hipLaunchKernelGGL(dcrw::k_fmt_size_tags, dim3(g), dim3(256), 0, c->stream, A);
        else
            hipLaunchKernelGGL(dcrw::k_fmt_size, dim3(g), dim3(256), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(dcrw::scan_excl_i64(wb.rec_size, wb.rec_off, (int)(2 * F + 1), wb.scan, c->stream));
        if (btags) {
            // after the filters like k_fmt_write: it copies the masked seq / qual, and reads nothing else they write
            dcrw::FmtTagArgs At{A, db.read_pos, wb.bmap.ss_col, wb.bmap.ds_col, wb.bmap.ds_aln, wb.bmap.flag};
            hipLaunchKernelGGL(dcrw::k_fmt_write_tags, dim3(g), dim3(256), 0, c->stream, At);
        } else {
            hipLaunchKernelGGL(dcrw::k_fmt_write, dim3(g), dim3(256), 0, c->stream, A);
        }
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(wb.rec_off, 0, 8, c->stream));
    }
    dcrw::DflArgs D{wb.stream, wb.rec_off + 2 * F, wb.slots, wb.bsz, wb.tok, nullptr,
                    (unsigned long long *)(wb.bsz + nbm + 1)};
    hipLaunchKernelGGL(dcrw::k_deflate, dim3(gd), dim3(dfl::kT), sizeof(dfl::Shared), c->stream, D);
    HIP_TRY(hipGetLastError());
    HIP_TRY(dcrw::scan_excl_i64(wb.bsz, wb.boff, (int)(nbm + 1), wb.scan, c->stream));
    dcrw::CompactArgs C{wb.slots, wb.bsz, wb.boff, wb.rec_off + 2 * F, wb.comp, wb.tot};
    hipLaunchKernelGGL(dcrw::k_compact, dim3(gd), dim3(256), 0, c->stream, C);
    HIP_TRY(hipGetLastError());
    if (ms) {
        // the single-strand stream: its own sizes, offsets and records
        // (k_famfail's outcomes are shared), then k_deflate and k_compact again
        dcrw::FmtSsArgs As{};
        As.ss = dout[0];
        As.sub_off = db.sub_off;
        As.read_mapq = db.read_mapq;
        As.ss_col_off = db.ss_col_off;
        As.names = wb.names;
        As.fam_code = wb.fam_code;
        As.fam_tid = wb.fam_tid;
        As.sub_flag = wsb.sub_flag;
        As.sub_mi = wsb.sub_mi;
        As.sub_rx = wsb.sub_rx;
        As.n_fam = (int32_t)F;
        As.fam_fail = wb.fam_fail;
        As.fam_filt = wb.fam_filt;
        As.rec_size = wsb.rec_size;
        As.rec_off = wsb.rec_off;
        As.stream = wsb.stream;
        HIP_TRY(hipMemsetAsync(wsb.rec_size, 0, 8 * (size_t)(4 * F + 1), c->stream));
        HIP_TRY(hipMemsetAsync(wsb.bsz, 0, 8 * (size_t)(wsb.nbm + 2), c->stream));
        if (F) {
            const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>(F, (int64_t)c->n_cu * 8));
            if (btags)
                hipLaunchKernelGGL(dcrw::k_fmt_size_ss_tags, dim3(g), dim3(256), 0, c->stream, As);
            else
                hipLaunchKernelGGL(dcrw::k_fmt_size_ss, dim3(g), dim3(256), 0, c->stream, As);
            HIP_TRY(hipGetLastError());
            HIP_TRY(dcrw::scan_excl_i64(wsb.rec_size, wsb.rec_off, (int)(4 * F + 1), wsb.scan, c->stream));
            if (btags) {
                dcrw::FmtSsTagArgs Ast{As, db.read_pos, wb.bmap.ss_col, wb.bmap.flag};
                hipLaunchKernelGGL(dcrw::k_fmt_write_ss_tags, dim3(g), dim3(256), 0, c->stream, Ast);
            } else {
                hipLaunchKernelGGL(dcrw::k_fmt_write_ss, dim3(g), dim3(256), 0, c->stream, As);
            }
            HIP_TRY(hipGetLastError());
        } else {
            HIP_TRY(hipMemsetAsync(wsb.rec_off, 0, 8, c->stream));
        }
        dcrw::DflArgs Ds{wsb.stream, wsb.rec_off + 4 * F, wsb.slots, wsb.bsz, wsb.tok, nullptr,
                         (unsigned long long *)(wsb.bsz + wsb.nbm + 1)};
        hipLaunchKernelGGL(dcrw::k_deflate, dim3(wsb.gd), dim3(dfl::kT), sizeof(dfl::Shared), c->stream, Ds);
        HIP_TRY(hipGetLastError());
        HIP_TRY(dcrw::scan_excl_i64(wsb.bsz, wsb.boff, (int)(wsb.nbm + 1), wsb.scan, c->stream));
        dcrw::CompactArgs Cs{wsb.slots, wsb.bsz, wsb.boff, wsb.rec_off + 4 * F, wsb.comp, wsb.tot};
        hipLaunchKernelGGL(dcrw::k_compact, dim3(wsb.gd), dim3(256), 0, c->stream, Cs);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(S.ev_comp, c->stream));
    // D2H of the per-family outcome and the totals on the second copy stream
    HIP_TRY(hipStreamWaitEvent(c->s_d2h, S.ev_comp, 0));
    if (F) {
        HIP_TRY(hipMemcpyAsync(res->fam_fail, wb.fam_fail, 4 * (size_t)F, hipMemcpyDeviceToHost, c->s_d2h));
        HIP_TRY(hipMemcpyAsync(res->ds_len, wb.ds_len, 8 * (size_t)F, hipMemcpyDeviceToHost, c->s_d2h));
        if (filt) HIP_TRY(hipMemcpyAsync(S.h_fam_filt, wb.fam_filt, 4 * (size_t)F, hipMemcpyDeviceToHost, c->s_d2h));
        if (ovl) HIP_TRY(hipMemcpyAsync(S.h_fam_ovl, wb.fam_ovl, 12 * (size_t)F, hipMemcpyDeviceToHost, c->s_d2h));
    }
    if (met) HIP_TRY(hipMemcpyAsync(S.h_metrics, wb.metrics, sizeof(dcr_metrics), hipMemcpyDeviceToHost, c->s_d2h));
    if (bmet)
        HIP_TRY(hipMemcpyAsync(S.h_base_metrics, wb.base_metrics, sizeof(dcr_base_metrics), hipMemcpyDeviceToHost,
                               c->s_d2h));
    if (gmet)
        HIP_TRY(hipMemcpyAsync(S.h_genome_metrics, wb.genome_metrics, sizeof(dcr_genome_metrics), hipMemcpyDeviceToHost,
                               c->s_d2h));
    HIP_TRY(hipMemcpyAsync(res->totals, wb.tot, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c->s_d2h));
    if (ms) HIP_TRY(hipMemcpyAsync(res_ss->totals, wsb.tot, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, c->s_d2h));
    HIP_TRY(hipEventRecord(S.ev_d2h, c->s_d2h));
    S.d_rec_off = wb.rec_off;
    S.d_stream = wb.stream;
    S.d_comp = wb.comp;
    S.d_ss_rec_off = ms ? wsb.rec_off : nullptr;
    S.d_ss_stream = ms ? wsb.stream : nullptr;
    S.d_ss_comp = ms ? wsb.comp : nullptr;
    S.d_map_flag = wb.bmap.flag;
    S.n_fam = F;
    S.writer = true;
    S.writer_ss = ms != nullptr;
    S.busy = true;
    return DCR_OK;
}

int dcr_set_filter(dcr_ctx *c, const dcr_filter *f) {
    if (!c) return fail(DCR_EARG, "NULL context");
    if (!f || f->active == 0) {
        c->filter = dcr_filter{};
        return DCR_OK;
    }
    const int all = DCR_FILT_MIN_READS | DCR_FILT_ERROR_RATE | DCR_FILT_NO_CALL | DCR_FILT_MEAN_QUAL | DCR_FILT_MASK_BASES;
    if (f->active & ~all) return fail(DCR_EARG, "unknown filter bits");
    if ((f->active & DCR_FILT_MASK_BASES) && f->min_base_quality < 0) return fail(DCR_EARG, "filter min_base_quality < 0");
    if ((f->active & DCR_FILT_MIN_READS) && !(f->min_reads[0] >= f->min_reads[1] && f->min_reads[1] >= f->min_reads[2]))
        return fail(DCR_EARG, "filter min_reads must be total >= larger strand >= smaller strand");
    auto unit = [](double x) { return x >= 0.0 && x <= 1.0; };
    if ((f->active & DCR_FILT_ERROR_RATE) && !(unit(f->max_error_rate[0]) && unit(f->max_error_rate[1])))
        return fail(DCR_EARG, "filter max_error_rate outside [0, 1]");
    if ((f->active & DCR_FILT_NO_CALL) && !unit(f->max_no_call_fraction))
        return fail(DCR_EARG, "filter max_no_call_fraction outside [0, 1]");
    if ((f->active & DCR_FILT_MEAN_QUAL) && !(f->min_mean_base_quality >= 0.0))
        return fail(DCR_EARG, "filter min_mean_base_quality < 0");
    c->filter = *f;
    return DCR_OK;
}

int dcr_set_base_filter(dcr_ctx *c, const dcr_base_filter *f) {
    if (!c) return fail(DCR_EARG, "NULL context");
    if (!f || f->active == 0) {
        c->base_filter = dcr_base_filter{};
        return DCR_OK;
    }
    if (f->active & ~(DCR_BF_MIN_READS | DCR_BF_ERROR_RATE | DCR_BF_AGREEMENT))
        return fail(DCR_EARG, "unknown base filter bits");
    if ((f->active & DCR_BF_MIN_READS) && !(f->min_reads[0] >= f->min_reads[1] && f->min_reads[1] >= f->min_reads[2]))
        return fail(DCR_EARG, "base filter min_reads must be total >= larger strand >= smaller strand");
    if ((f->active & DCR_BF_ERROR_RATE) && !(f->max_error_rate >= 0.0 && f->max_error_rate <= 1.0))
        return fail(DCR_EARG, "base filter max_error_rate outside [0, 1]");
    c->base_filter = *f;
    return DCR_OK;
}

int dcr_slot_filter_out(dcr_ctx *c, int slot, int32_t *fam_filt) {
    if (!c || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    if (c->slots[slot].busy) return fail(DCR_EARG, "slot still in flight (dcr_wait it first)");
    c->slots[slot].h_fam_filt = fam_filt;
    return DCR_OK;
}

int dcr_set_mate_overlap(dcr_ctx *c, int mode) {
    if (!c) return fail(DCR_EARG, "NULL context");
    if (mode != 0 && mode != DCR_OVL_MASK && mode != DCR_OVL_CONSENSUS)
        return fail(DCR_EARG, "mate overlap mode must be 0, DCR_OVL_MASK or DCR_OVL_CONSENSUS");
    c->mate_overlap = mode;
    return DCR_OK;
}

int dcr_slot_overlap_out(dcr_ctx *c, int slot, int32_t *fam_ovl) {
    if (!c || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    if (c->slots[slot].busy) return fail(DCR_EARG, "slot still in flight (dcr_wait it first)");
    c->slots[slot].h_fam_ovl = fam_ovl;
    return DCR_OK;
}

int dcr_set_allele_sites(dcr_ctx *c, const int64_t *keys, int64_t n, int min_base_quality) {
    if (!c) return fail(DCR_EARG, "NULL context");
    if (!keys || n == 0) {
        if (c->n_allele) {
            // the table may still be counted into: the batches in flight first
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_allele_keys);
            (void)hipFree(c->d_allele_tab);
        }
        c->d_allele_keys = nullptr;
        c->d_allele_tab = nullptr;
        c->n_allele = 0;
        c->allele_min_q = 0;
        return DCR_OK;
    }
    if (n < 0 || n > DCR_ALLELE_MAX_SITES) return fail(DCR_EARG, "allele sites: n outside [0, DCR_ALLELE_MAX_SITES]");
    if (min_base_quality < 0) return fail(DCR_EARG, "allele sites: min_base_quality < 0");
    for (int64_t i = 0; i < n; ++i) {
        if (keys[i] < 0 || (keys[i] & 0x80000000ll)) return fail(DCR_EARG, "allele sites: tid or pos outside [0, 2^31)");
        if (i && keys[i] <= keys[i - 1]) return fail(DCR_EARG, "allele sites: keys must be strictly increasing");
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int64_t *dk = nullptr;
    unsigned long long *dt = nullptr;
    const size_t tab_bytes = (size_t)n * DCR_ALLELE_COLS * sizeof(unsigned long long);
    hipError_t e = hipMalloc(&dk, (size_t)n * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc(&dt, tab_bytes);
    if (e == hipSuccess) e = hipMemcpy(dk, keys, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dt, 0, tab_bytes);
    if (e != hipSuccess) {
        if (dk) (void)hipFree(dk);
        if (dt) (void)hipFree(dt);
        return fail(DCR_EHIP, hipGetErrorString(e));
    }
    if (c->d_allele_keys) (void)hipFree(c->d_allele_keys);
    if (c->d_allele_tab) (void)hipFree(c->d_allele_tab);
    c->d_allele_keys = dk;
    c->d_allele_tab = dt;
    c->n_allele = n;
    c->allele_min_q = std::min(min_base_quality, 256);
    return DCR_OK;
}

int dcr_allele_counts_fetch(dcr_ctx *c, uint64_t *dst) {
    if (!c || !dst) return fail(DCR_EARG, "NULL argument");
    if (!c->n_allele) return fail(DCR_EARG, "no allele sites are set (dcr_set_allele_sites)");
    HIP_TRY(hipSetDevice(c->device));
    // every slot's kernels run on the context's stream
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(dst, c->d_allele_tab, (size_t)c->n_allele * DCR_ALLELE_COLS * sizeof(uint64_t),
                      hipMemcpyDeviceToHost));
    return DCR_OK;
}

int dcr_set_genome(dcr_ctx *c, const uint8_t *codes, const int64_t *ref_off, int32_t n_ref) {
    if (!c) return fail(DCR_EARG, "NULL context");
    if (!codes || !ref_off || n_ref == 0) {
        if (c->n_ref) {
            // the genome may still be read: the batches in flight first
            HIP_TRY(hipSetDevice(c->device));
            HIP_TRY(hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_genome);
            (void)hipFree(c->d_ref_off);
        }
        c->d_genome = nullptr;
        c->d_ref_off = nullptr;
        c->n_ref = 0;
        return DCR_OK;
    }
    if (n_ref < 0) return fail(DCR_EARG, "genome: n_ref < 0");
    if (ref_off[0] != 0) return fail(DCR_EARG, "genome: ref_off[0] must be 0");
    for (int32_t t = 0; t < n_ref; ++t)
        if (ref_off[t + 1] < ref_off[t]) return fail(DCR_EARG, "genome: ref_off must not decrease");
    const int64_t total = ref_off[n_ref];
    for (int64_t i = 0; i < total; ++i)
        if (codes[i] > 4) return fail(DCR_EARG, "genome: a code above 4");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    uint8_t *dg = nullptr;
    int64_t *dr = nullptr;
    // never a zero-size allocation: a genome of absent sequences only still turns the counting on
    hipError_t e = hipMalloc(&dg, (size_t)std::max<int64_t>(total, 16));
    if (e == hipSuccess) e = hipMalloc(&dr, ((size_t)n_ref + 1) * sizeof(int64_t));
    // a pageable source in chunks: the runtime stages each through its own pinned buffer
    const int64_t chunk = (int64_t)64 << 20;
    for (int64_t at = 0; e == hipSuccess && at < total; at += chunk)
        e = hipMemcpy(dg + at, codes + at, (size_t)std::min(chunk, total - at), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dr, ref_off, ((size_t)n_ref + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (dg) (void)hipFree(dg);
        if (dr) (void)hipFree(dr);
        return fail(DCR_EHIP, hipGetErrorString(e));
    }
    if (c->d_genome) (void)hipFree(c->d_genome);
    if (c->d_ref_off) (void)hipFree(c->d_ref_off);
    c->d_genome = dg;
    c->d_ref_off = dr;
    c->n_ref = n_ref;
    return DCR_OK;
}

int dcr_slot_genome_metrics_out(dcr_ctx *c, int slot, dcr_genome_metrics *pinned_dst) {
    if (!c || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    if (c->slots[slot].busy) return fail(DCR_EARG, "slot still in flight (dcr_wait it first)");
    c->slots[slot].h_genome_metrics = pinned_dst;
    return DCR_OK;
}

int dcr_set_metrics(dcr_ctx *c, int on) {
    if (!c) return fail(DCR_EARG, "NULL context");
    c->metrics = on != 0;
    return DCR_OK;
}

int dcr_set_base_tags(dcr_ctx *c, int on) {
    if (!c) return fail(DCR_EARG, "NULL context");
    c->base_tags = on != 0;
    return DCR_OK;
}

int dcr_set_base_metrics(dcr_ctx *c, int on) {
    if (!c) return fail(DCR_EARG, "NULL context");
    c->base_metrics = on != 0;
    return DCR_OK;
}

int dcr_slot_base_metrics_out(dcr_ctx *c, int slot, dcr_base_metrics *pinned_dst) {
    if (!c || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    if (c->slots[slot].busy) return fail(DCR_EARG, "slot still in flight (dcr_wait it first)");
    c->slots[slot].h_base_metrics = pinned_dst;
    return DCR_OK;
}

int dcr_slot_metrics_out(dcr_ctx *c, int slot, dcr_metrics *pinned_dst) {
    if (!c || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    if (c->slots[slot].busy) return fail(DCR_EARG, "slot still in flight (dcr_wait it first)");
    c->slots[slot].h_metrics = pinned_dst;
    return DCR_OK;
}

int dcr_submit_write(dcr_ctx *c, int slot, const dcr_batch *h, const dcr_wmeta *m, dcr_wres *res) {
    if (!c || !h || !m || !res) return fail(DCR_EARG, "NULL argument");
    return submit_write(c, slot, h, m, nullptr, res, nullptr);
}

int dcr_submit_write_ss(dcr_ctx *c, int slot, const dcr_batch *h, const dcr_wmeta *m, const dcr_wmeta_ss *ms,
                        dcr_wres *res, dcr_wres *res_ss) {
    if (!c || !h || !m || !ms || !res || !res_ss) return fail(DCR_EARG, "NULL argument");
    if (h->n_fam > 0 && (!ms->sub_flag || !ms->sub_mi || !ms->sub_rx))
        return fail(DCR_EARG, "single-strand metadata missing");
    return submit_write(c, slot, h, m, ms, res, res_ss);
}

// the tail of dcr_wait_write: a finished slot's compressed blocks into res->bgzf
static int fetch_blocks(dcr_ctx *c, const uint8_t *d_comp, dcr_wres *res) {
    const int64_t n = res->totals[0];
    if (n > res->cap_bgzf) return fail(DCR_ECAPACITY, "BGZF output larger than cap_bgzf (see totals[0])");
    if (n > 0) {
        if (!c->ev_fetch) HIP_TRY(hipEventCreateWithFlags(&c->ev_fetch, hipEventDisableTiming | hipEventBlockingSync));
        HIP_TRY(hipMemcpyAsync(res->bgzf, d_comp, (size_t)n, hipMemcpyDeviceToHost, c->s_fetch));
        HIP_TRY(hipEventRecord(c->ev_fetch, c->s_fetch));
        HIP_TRY(hipEventSynchronize(c->ev_fetch));
    }
    return DCR_OK;
}

int dcr_wait_write(dcr_ctx *c, int slot, dcr_wres *res) {
    if (!c || !res || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    dcr_ctx::Slot &S = c->slots[slot];
    if (!S.busy || !S.writer) return fail(DCR_EARG, "slot has no writer batch in flight");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(S.ev_d2h));
    S.busy = false;
    if (*S.h_err) return fail(DCR_ECAPACITY, "a consensus needed more columns than its output region");
    return fetch_blocks(c, S.d_comp, res);
}

int dcr_wait_write_ss(dcr_ctx *c, int slot, dcr_wres *res, dcr_wres *res_ss) {
    if (!c || !res || !res_ss || slot < 0 || slot >= DCR_MAX_SLOTS) return fail(DCR_EARG, "bad argument");
    dcr_ctx::Slot &S = c->slots[slot];
    if (!S.busy || !S.writer || !S.writer_ss) return fail(DCR_EARG, "slot has no single-strand writer batch in flight");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(S.ev_d2h));
    S.busy = false;
    if (*S.h_err) return fail(DCR_ECAPACITY, "a consensus needed more columns than its output region");
    // both streams are tried, so that after DCR_ECAPACITY the caller can
    // tell from the two totals[0] which of them to fetch again
    const int rc = fetch_blocks(c, S.d_comp, res);
    if (rc != DCR_OK && rc != DCR_ECAPACITY) return rc;
    const int rc_ss = fetch_blocks(c, S.d_ss_comp, res_ss);
    return rc_ss != DCR_OK ? rc_ss : rc;
}

int dcr_slot_fetch(dcr_ctx *c, int slot, int what, int64_t off, int64_t n, void *dst) {
    if (!c || !dst || slot < 0 || slot >= DCR_MAX_SLOTS || off < 0 || n < 0) return fail(DCR_EARG, "bad argument");
    dcr_ctx::Slot &S = c->slots[slot];
    if (!S.writer) return fail(DCR_EARG, "slot holds no writer batch");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(S.ev_d2h));
    if (what == 0) {
        if (n) HIP_TRY(hipMemcpy(dst, S.d_stream + off, (size_t)n, hipMemcpyDeviceToHost));
    } else if (what == 1) {
        if (off + n > 2 * S.n_fam + 1) return fail(DCR_EARG, "record offsets out of range");
        if (n) HIP_TRY(hipMemcpy(dst, S.d_rec_off + off, 8 * (size_t)n, hipMemcpyDeviceToHost));
    } else if (what == 2) {
        if (n) HIP_TRY(hipMemcpy(dst, S.d_comp + off, (size_t)n, hipMemcpyDeviceToHost));
    } else if (what >= 3 && what <= 5) {
        if (!S.writer_ss) return fail(DCR_EARG, "slot holds no single-strand writer batch");
        if (what == 3) {
            if (n) HIP_TRY(hipMemcpy(dst, S.d_ss_stream + off, (size_t)n, hipMemcpyDeviceToHost));
        } else if (what == 4) {
            if (off + n > 4 * S.n_fam + 1) return fail(DCR_EARG, "record offsets out of range");
            if (n) HIP_TRY(hipMemcpy(dst, S.d_ss_rec_off + off, 8 * (size_t)n, hipMemcpyDeviceToHost));
        } else {
            if (n) HIP_TRY(hipMemcpy(dst, S.d_ss_comp + off, (size_t)n, hipMemcpyDeviceToHost));
        }
    } else if (what == 6) {
        if (!S.d_map_flag) return fail(DCR_EARG, "slot's batch ran without a base filter, the per-base tags or the base metrics");
        if (off + n > 6 * S.n_fam) return fail(DCR_EARG, "map flags out of range");
        if (n) HIP_TRY(hipMemcpy(dst, S.d_map_flag + off, (size_t)n, hipMemcpyDeviceToHost));
    } else {
        return fail(DCR_EARG, "what must be 0 (record bytes), 1 (record offsets), 2 (BGZF blocks), 3 to 5 "
                              "(the same of the single-strand stream) or 6 (stored-map flags)");
    }
    return DCR_OK;
}

// diagnostic (not in include/dcr.h): k_deflate alone over n host bytes with
// per-phase s_memtime cycle totals (summed over workgroups) and the HIP-event
// time; returns the compressed bytes in *comp_bytes and, when slots_out is
// given (ceil(n / 0xff00) * 65536 bytes), each block's BGZF member at the
// start of its 64 KiB slot, the member sizes in sizes_out
int dcr_deflate_probe(dcr_ctx *c, const uint8_t *host, int64_t n, unsigned long long *stamps12, float *ms,
                      int64_t *comp_bytes, uint8_t *slots_out, int64_t *sizes_out) {
    if (!c || !host || n <= 0 || !stamps12 || !ms || !comp_bytes) return fail(DCR_EARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t nb = (n + dfl::kMaxIn - 1) / dfl::kMaxIn;
    uint8_t *d_in = nullptr, *d_slots = nullptr;
    int64_t *d_n = nullptr, *d_sizes = nullptr;
    unsigned long long *d_st = nullptr;
    uint32_t *d_tok = nullptr;
    HIP_TRY(hipMalloc(&d_in, (size_t)n));
    HIP_TRY(hipMalloc(&d_slots, (size_t)nb * dfl::kSlot));
    HIP_TRY(hipMalloc(&d_n, 8));
    HIP_TRY(hipMalloc(&d_sizes, 8 * (size_t)nb));
    HIP_TRY(hipMalloc(&d_st, 8 * 12));
    const unsigned gd = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nb, (int64_t)c->n_cu * c->dfl_blocks));
    HIP_TRY(hipMalloc(&d_tok, (size_t)gd * dfl::kTokWords * 4));
    HIP_TRY(hipMemcpy(d_in, host, (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_n, &n, 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_st, 0, 96));
    dcrw::DflArgs D{d_in, d_n, d_slots, d_sizes, d_tok, d_st, nullptr};
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, c->stream));
    hipLaunchKernelGGL(dcrw::k_deflate, dim3(gd), dim3(dfl::kT), sizeof(dfl::Shared), c->stream, D);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e1, c->stream));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(ms, e0, e1));
    HIP_TRY(hipMemcpy(stamps12, d_st, 96, hipMemcpyDeviceToHost));
    std::vector<int64_t> sz((size_t)nb);
    HIP_TRY(hipMemcpy(sz.data(), d_sizes, 8 * (size_t)nb, hipMemcpyDeviceToHost));
    int64_t tot = 0;
    for (int64_t v : sz) tot += v;
    *comp_bytes = tot;
    if (sizes_out) std::memcpy(sizes_out, sz.data(), 8 * (size_t)nb);
    if (slots_out) HIP_TRY(hipMemcpy(slots_out, d_slots, (size_t)nb * dfl::kSlot, hipMemcpyDeviceToHost));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(d_in);
    (void)hipFree(d_slots);
    (void)hipFree(d_n);
    (void)hipFree(d_sizes);
    (void)hipFree(d_st);
    (void)hipFree(d_tok);
    return DCR_OK;
}

// test entry (not in include/dcr.h; tests/test_gpu_deflate_blocks.py):
// k_deflate alone over n host bytes, shaped so that a wrong byte shows.
//   max_wg     0: the pipeline's grid, min(blocks, CUs x resident workgroups);
//              else at most that many workgroups (1: one workgroup compresses
//              every block in turn, on the LDS the block before left)
//   use_claim  a zeroed block counter in DflArgs::claim, as the pipeline passes
//   the device input is allocated to a multiple of 16 bytes (the staging loads
//   16 at a time) and the bytes past n hold 0xff
//   slots_out  (blocks + 1) x 65536 bytes: every slot and one guard slot behind
//              the last are filled with `fill` before the launch and returned whole
//   sizes_out  [blocks], -1 where the kernel wrote none
int dcr_deflate_blocks(dcr_ctx *c, const uint8_t *host, int64_t n, int max_wg, int use_claim, int fill,
                       uint8_t *slots_out, int64_t *sizes_out) {
    if (!c || !host || n <= 0 || max_wg < 0 || !slots_out || !sizes_out) return fail(DCR_EARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    const int64_t nb = (n + dfl::kMaxIn - 1) / dfl::kMaxIn;
    const size_t n_in = ((size_t)n + 15) & ~(size_t)15, n_slots = (size_t)(nb + 1) * dfl::kSlot;
    unsigned gd = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nb, (int64_t)c->n_cu * c->dfl_blocks));
    if (max_wg) gd = std::min(gd, (unsigned)max_wg);
    uint8_t *d_in = nullptr, *d_slots = nullptr;
    int64_t *d_n = nullptr, *d_sizes = nullptr;
    unsigned long long *d_claim = nullptr;
    uint32_t *d_tok = nullptr;
    auto run = [&]() -> int {
        HIP_TRY(hipMalloc(&d_in, n_in));
        HIP_TRY(hipMalloc(&d_slots, n_slots));
        HIP_TRY(hipMalloc(&d_n, 8));
        HIP_TRY(hipMalloc(&d_sizes, 8 * (size_t)nb));
        HIP_TRY(hipMalloc(&d_claim, 8));
        HIP_TRY(hipMalloc(&d_tok, (size_t)gd * dfl::kTokWords * 4));
        HIP_TRY(hipMemsetAsync(d_in, 0xff, n_in, c->stream));
        HIP_TRY(hipMemsetAsync(d_slots, fill & 0xff, n_slots, c->stream));
        HIP_TRY(hipMemsetAsync(d_sizes, 0xff, 8 * (size_t)nb, c->stream));
        HIP_TRY(hipMemsetAsync(d_claim, 0, 8, c->stream));
        HIP_TRY(hipMemcpyAsync(d_in, host, (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_n, &n, 8, hipMemcpyHostToDevice, c->stream));
        dcrw::DflArgs D{d_in, d_n, d_slots, d_sizes, d_tok, nullptr, use_claim ? d_claim : nullptr};
        hipLaunchKernelGGL(dcrw::k_deflate, dim3(gd), dim3(dfl::kT), sizeof(dfl::Shared), c->stream, D);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipMemcpy(sizes_out, d_sizes, 8 * (size_t)nb, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(slots_out, d_slots, n_slots, hipMemcpyDeviceToHost));
        return DCR_OK;
    };
    const int rc = run();
    (void)hipFree(d_in);
    (void)hipFree(d_slots);
    (void)hipFree(d_n);
    (void)hipFree(d_sizes);
    (void)hipFree(d_claim);
    (void)hipFree(d_tok);
    return rc;
}

}  // extern "C"
