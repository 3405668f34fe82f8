// dcr_writer.h — kernel arguments of the device record writer
// (dcr_writer.hip); not part of the C-ABI (include/dcr.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dcr.h"

namespace dcrw {

struct FmtArgs {
    dcr_out ss, ds;                 // device kernel outputs
    const int32_t *sub_off;         // [4F+1]
    const uint8_t *read_mapq;
    const int64_t *ss_col_off, *ds_col_off;
    const dcr_read_info *info;      // per-read preprocessing status
    const char *names;
    const int64_t *fam_code, *fam_rx;
    const int32_t *fam_tid;
    int32_t n_fam;
    int32_t *fam_fail;              // [F] DCR_FAIL_* | which << 8
    int32_t *ds_len_out;            // [2F]
    int64_t *rec_size;              // [2F+1] (the last one 0: the scan's total)
    int64_t *rec_off;               // [2F+1]
    uint8_t *stream;                // formatted records
    const int32_t *fam_filt;        // [F] from k_filter, or null (no filter set): low byte set = dropped
};

// the consensus filters (k_filter, dcr_set_filter)
struct FilterArgs {
    dcr_out ss, ds;                 // device kernel outputs; ds.seq / ds.qual are masked in place
    const int64_t *ds_col_off;      // [2F+1]
    const int32_t *fam_fail;        // [F] from k_famfail
    int32_t *fam_filt;              // [F] reason bits | masked bases << 8
    int32_t n_fam;
    dcr_filter flt;
    const int32_t *base_masked;     // [F] bases k_base_filter masked, added into fam_filt >> 8; or null
};

// the per-base filters (k_base_filter, dcr_set_base_filter)
struct BaseFilterArgs {
    dcr_out ss, ds;                 // device kernel outputs; ds.seq / ds.qual are masked in place
    const int32_t *sub_off;         // [4F+1]
    const int32_t *read_pos;        // [n_reads]
    const int64_t *ss_col_off, *ds_col_off;
    const int32_t *fam_fail;        // [F] from k_famfail
    // the stored maps of the records with insertion columns (dcr::BaseMap)
    const uint32_t *ss_col, *ds_col, *ds_aln;
    const uint8_t *flag;            // [6F]
    int32_t *masked;                // [F] bases masked here whose new quality min(q, 2) is not below skip_below:
                                    // the others k_filter masks again and counts (0 for failing families)
    int32_t n_fam;
    int32_t skip_below;             // bases of a quality below this are left to k_filter, which masks and counts them
    dcr_base_filter flt;
};

// the consensus QC tables (k_metrics, dcr_set_metrics)
struct MetricsArgs {
    dcr_out ss, ds;                 // device kernel outputs, read only (before k_filter masks ds)
    const int32_t *sub_off;         // [4F+1]
    const int64_t *ss_col_off, *ds_col_off;
    const int32_t *fam_fail;        // [F] from k_famfail
    int32_t n_fam;
    dcr_metrics *out;               // the slot's accumulator, zeroed before the launch
};
constexpr int kMetThreads = 1024;   // k_metrics' workgroup: 16 waves on one set of LDS tables

// the single-strand records' writer (k_fmt_size_ss / k_fmt_write_ss)
struct FmtSsArgs {
    dcr_out ss;                     // device kernel outputs
    const int32_t *sub_off;         // [4F+1]
    const uint8_t *read_mapq;
    const int64_t *ss_col_off;
    const char *names;
    const int64_t *fam_code;        // [F]
    const int32_t *fam_tid;         // [F]
    const uint16_t *sub_flag;       // [4F] read0's flag
    const int64_t *sub_mi, *sub_rx; // [4F] names offsets of read0's MI / RX
    int32_t n_fam;
    const int32_t *fam_fail;        // [F] from k_famfail
    const int32_t *fam_filt;        // [F] from k_filter, or null
    int64_t *rec_size;              // [4F+1] (the last one 0: the scan's total)
    int64_t *rec_off;               // [4F+1]
    uint8_t *stream;                // formatted records
};

// the per-base tags' writers (k_fmt_write_tags / k_fmt_write_ss_tags, dcr_set_base_tags): the
// default writer's arguments and what the column of a base needs (as BaseFilterArgs)
struct FmtTagArgs {
    FmtArgs f;
    const int32_t *read_pos;        // [n_reads]
    const uint32_t *ss_col, *ds_col, *ds_aln;   // the stored maps (dcr::BaseMap)
    const uint8_t *flag;            // [6F]
};
struct FmtSsTagArgs {
    FmtSsArgs f;
    const int32_t *read_pos;        // [n_reads]
    const uint32_t *ss_col;
    const uint8_t *flag;            // [6F]: the single-strand records' are the first 4F
};

// the per-base duplex QC tables (k_base_metrics, dcr_set_base_metrics): what the column of a base
// needs (as BaseFilterArgs), everything read only
struct BaseMetricsArgs {
    dcr_out ss, ds;                 // device kernel outputs (before the filters mask ds)
    const int32_t *sub_off;         // [4F+1]
    const int32_t *read_pos;        // [n_reads]
    const int64_t *ss_col_off, *ds_col_off;
    const int32_t *fam_fail;        // [F] from k_famfail
    const uint32_t *ss_col, *ds_col, *ds_aln;   // the stored maps (dcr::BaseMap)
    const uint8_t *flag;            // [6F]
    int32_t n_fam;
    int32_t f0, f1;                 // the families of this launch: their duplex regions hold fewer than 2^32 columns
    dcr_base_metrics *out;          // the slot's accumulator, zeroed before the first launch
};
constexpr int kBmThreads = 1024;    // k_base_metrics' workgroup: 16 waves on one set of LDS tables

// the overlapping mates (k_mate_overlap, dcr_set_mate_overlap)
struct MateOverlapArgs {
    dcr_out ds;                     // device kernel outputs; ds.seq / ds.qual are rewritten in place
    const int64_t *ds_col_off;      // [2F+1]
    const int32_t *fam_fail;        // [F] from k_famfail
    int32_t *fam_ovl;               // [3F] compared, disagree, changed
    int32_t n_fam;
    int32_t mode;                   // DCR_OVL_MASK or DCR_OVL_CONSENSUS
};

// the allele counts at given sites (k_allele_counts, dcr_set_allele_sites)
struct AlleleArgs {
    dcr_out ds;                     // device kernel outputs, as the filters left them; read only
    const int64_t *ds_col_off;      // [2F+1]
    const int32_t *fam_fail;        // [F] from k_famfail
    const int32_t *fam_filt;        // [F] from k_filter, or null without a filter
    const int32_t *fam_tid;         // [F]
    const int64_t *keys;            // [n_keys] tid << 32 | pos, strictly increasing
    unsigned long long *table;      // [n_keys][DCR_ALLELE_COLS], the context's
    int64_t n_keys;
    int32_t n_fam;
    int32_t min_q;                  // a base below it calls N
};

// the errors against a genome (k_genome_metrics, dcr_set_genome): one level a launch, everything
// read only but the slot's block
struct GenomeMetricsArgs {
    dcr_out o;                      // the level's device kernel outputs: ss (lv 0) or ds (lv 1), as called
    const int64_t *col_off;         // the level's ss_col_off [4F+1] or ds_col_off [2F+1]
    const int32_t *fam_fail;        // [F] from k_famfail
    const int32_t *fam_tid;         // [F]
    const uint8_t *codes;           // the context's genome, one code a base
    const int64_t *ref_off;         // [n_ref + 1]
    int32_t n_ref;
    int32_t lv;                     // 0: four records a family, 1: two
    int64_t r0, r1;                 // the records of this launch: their regions hold fewer than 2^32 columns
    dcr_genome_metrics *out;        // the slot's block, zeroed before the first launch
};
constexpr int kGmThreads = 1024;    // k_genome_metrics' workgroup: 16 waves on one level's LDS tables

struct DflArgs {
    const uint8_t *stream;
    const int64_t *stream_bytes;    // device scalar (rec_off[2F])
    uint8_t *slots;                 // 64 KiB per block
    int64_t *sizes;                 // per block (0 past the last block)
    uint32_t *tok;                  // dfl::kTokWords per workgroup of the grid
    unsigned long long *stamps;     // diagnostic (dcr_deflate_probe): s_memtime cycles per phase, or null
    unsigned long long *claim;      // zeroed block counter: workgroups claim blocks from it (null: a fixed stride)
};

struct CompactArgs {
    const uint8_t *slots;
    const int64_t *sizes;
    const int64_t *offs;            // exclusive scan of sizes
    const int64_t *stream_bytes;
    uint8_t *out;
    int64_t *totals;                // [3] compressed bytes, formatted bytes, blocks
};

__global__ void k_famfail(FmtArgs A);
__global__ void k_filter(FilterArgs A);
__global__ void k_base_filter(BaseFilterArgs A);
__global__ void k_metrics(MetricsArgs A);
__global__ void k_fmt_size(FmtArgs A);
__global__ void k_fmt_write(FmtArgs A);
__global__ void k_fmt_size_ss(FmtSsArgs A);
__global__ void k_fmt_write_ss(FmtSsArgs A);
__global__ void k_fmt_size_tags(FmtArgs A);
__global__ void k_fmt_write_tags(FmtTagArgs T);
__global__ void k_fmt_size_ss_tags(FmtSsArgs A);
__global__ void k_fmt_write_ss_tags(FmtSsTagArgs T);
__global__ void k_base_metrics(BaseMetricsArgs A);
__global__ void k_mate_overlap(MateOverlapArgs A);
__global__ void k_allele_counts(AlleleArgs A);
__global__ void k_genome_metrics(GenomeMetricsArgs A);
__global__ void k_deflate(DflArgs D);
__global__ void k_compact(CompactArgs C);

// exclusive prefix sum out[i] = in[0] + .. + in[i-1] (in != out), tmp of
// scan_tmp_bytes(n) bytes; launches on s
size_t scan_tmp_bytes(int n);
hipError_t scan_excl_i64(const int64_t *in, int64_t *out, int n, int64_t *tmp, hipStream_t s);

}  // namespace dcrw
