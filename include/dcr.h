/*
 * dcr.h — C-ABI of the MI355X duplex-consensus hot path (libdcr.so).
 *
 * Replaces, per batch of MI families, the six calls per family the reference
 * makes to
 *     make_consensus_read(list_of_reads, method)
 *         /root/reference/DuplexUMIConsensusReads.py:1291-1386
 * (4x method="single_strand" at :1569, 2x method="double_strand" at :1581-1582)
 * together with the per-read preprocessing they consume
 *     remove_clipping / mask_low_quality_bases / trim_3prime_N   :191-325
 * The reference has no FFI of its own (it is one Python script whose config
 * is module globals, :1432-1469); INTEGRATION.md shows the ctypes binding the
 * host uses (duplexumiconsensusreads_amd/_lib.py) and how a maintainer would
 * call it from the reference's main() loop (:1560-1588).
 *
 * Plain pointers and sizes only.  All batch/out pointers passed to
 * dcr_run_batch are DEVICE pointers (HBM-resident inputs); dcr_run_batch_host
 * takes HOST pointers and stages through the context's device buffers.
 * Errors: functions return 0 or a DCR_E* code; the message is available from
 * dcr_last_error() (thread-local).  Per-record "the reference would raise"
 * outcomes are reported in the status arrays, not as errors.
 */
#ifndef DCR_H
#define DCR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCR_ABI_VERSION 1
#define DCR_LUT_PLUS 256   /* LUT row of '+' (absence of insertion), :667-669 */
#define DCR_LUT_DEL 257    /* LUT row of '-' (deletion), :670-672            */
#define DCR_LUT_N 258
#define DCR_MAX_QTHRESH 257

/* return codes */
enum {
    DCR_OK = 0,
    DCR_EARG = 1,       /* bad argument / params                                */
    DCR_EHIP = 2,       /* HIP runtime error                                    */
    DCR_ECAPACITY = 3,  /* an output region is smaller than the consensus needs */
    DCR_ENODEV = 4      /* no usable gfx950 device                              */
};

/* per-record status (what the reference does on these inputs) */
enum {
    DCR_ST_OK = 0,
    DCR_ST_INDEX_ERROR = 1,    /* IndexError: compress_cigarlist([]) :740, insertion past
                                  the sequence end :485                               */
    DCR_ST_TYPE_ERROR = 2,     /* TypeError: a read/consensus without sequence (:402)  */
    DCR_ST_VALUE_ERROR = 3,    /* ValueError: max() of an empty depth list (:1005)     */
    DCR_ST_OVERFLOW_ERROR = 4, /* OverflowError: quality outside uint8 (:1383)         */
    DCR_ST_EXIT_BADCHAR = 5,   /* sys.exit(1): invalid nucleotide (:582-585)           */
    DCR_ST_UPSTREAM = 6,       /* duplex, not computed: an input consensus failed      */
    DCR_ST_PREP = 0x10         /* single-strand: DCR_ST_PREP | s = the preprocessing of a read
                                  raised s (the subfamily's first failing read, :1272-1283) */
};

/* context options (dcr_set_options) */
#define DCR_OPT_READ_INFO 1    /* every read's dcr_read_info is written (parity tests; costs
                                  24 B of HBM writes per read); otherwise only failing reads' */

/* Numeric flags (:1432-1469) plus host-built tables.  The tables are built on
 * the host with the reference's own Python arithmetic (params.py), so the
 * device never evaluates pow/log10 (bit-exact by construction). */
typedef struct dcr_params {
    int32_t min_base_quality;        /* --min_base_quality (seqQ_threshold)   */
    int32_t max_base_quality;        /* --max_base_quality                    */
    int32_t base_quality_shift;      /* --base_quality_shift                  */
    int32_t error_rate_post_labeling;/* --error_rate_post_labeling (raw int)  */
    int32_t error_rate_pre_labeling; /* --error_rate_pre_labeling (raw int)   */
    int32_t deletion_score;          /* --deletion_score                      */
    int32_t no_insertion_score;      /* --no_insertion_score                  */
    int32_t n_qthresh;               /* entries used in qthresh (= maxQ + 1)  */
    /* (1 - p') and p'/5 for quality codes 0..255, '+' (256), '-' (257);
       p' = post*(1-ps) + (1-post)*ps + post*ps*4/5, ps = 10**(-s/10)  :665-676 */
    double match[DCR_LUT_N];
    double mismatch[DCR_LUT_N];
    double post_threshold;           /* 1 - 10**(-min_base_quality/10)   :679-680 */
    /* qthresh[i] = smallest double x > 0 with int(round(-10*log10(x), 0)) <= i-1,
       i = 0..maxQ (decreasing in i).  For a finite error x > 0 the consensus
       quality (:699-709) is Q = maxQ - #{i : x >= qthresh[i]}; Q < 0 means the
       reference would store a negative quality (OverflowError).  x <= 0 or NaN
       give maxQ (the reference's ValueError branch). */
    double qthresh[DCR_MAX_QTHRESH];
} dcr_params;

/* One batch of families, struct-of-arrays.  Subfamily s = 4*f + k with
 * k = 0..3 for A1, B2, B1, A2 (split_family :132-154); reads of a subfamily
 * are contiguous and in reference order (after check_number_reads' random
 * downsampling, :157-188, which stays on the host). */
typedef struct dcr_batch {
    int32_t n_fam;
    int32_t n_reads;
    int64_t n_cigar;            /* entries of cigar                              */
    int64_t n_bases;            /* entries of bases / quals                      */
    int64_t ss_cols;            /* ss_col_off[4F]                                */
    int64_t ds_cols;            /* ds_col_off[2F]                                */
    const int32_t *sub_off;     /* [4F+1] first read of each subfamily          */
    const int32_t *read_pos;    /* [n_reads] reference_start (0-based)          */
    const uint8_t *read_mapq;   /* [n_reads] mapping_quality                    */
    const int64_t *seq_off;     /* [n_reads] offset into bases/quals            */
    const int32_t *seq_len;     /* [n_reads] query length incl. soft clips      */
    const int32_t *cig_off;     /* [n_reads] offset into cigar                  */
    const int32_t *cig_n;       /* [n_reads] number of cigar ops                */
    const uint32_t *cigar;      /* BAM encoding (len << 4 | op)                 */
    const uint8_t *bases;       /* ASCII bases as stored (before masking)       */
    const uint8_t *quals;       /* phred qualities                              */
    const int64_t *ss_col_off;  /* [4F+1] single-strand output region offsets   */
    const int64_t *ds_col_off;  /* [2F+1] duplex output region offsets          */
} dcr_batch;

/* Results of one consensus kind (single-strand: 4F records, duplex: 2F).
 * Variable-length fields live in the record's region [col_off[i], col_off[i+1]). */
typedef struct dcr_out {
    uint8_t *status;    /* DCR_ST_*                                            */
    int32_t *pos;       /* consensus reference_start (:790)                    */
    int32_t *mapq;      /* trunc(mean(mapq)) (:874-889, :1377)                 */
    int32_t *len;       /* consensus sequence length                           */
    int32_t *n_cig;     /* consensus cigar ops                                 */
    int32_t *n_de;      /* entries of d / e (:1002-1003)                       */
    int32_t *D;         /* max depth                                           */
    int32_t *M;         /* min depth                                           */
    double *E;          /* round(mean(e/d), 3)                                 */
    uint8_t *seq;       /* ASCII consensus bases                               */
    uint8_t *qual;      /* consensus qualities                                 */
    uint32_t *cigar;    /* BAM encoding                                        */
    uint16_t *d;        /* per-column depth                                    */
    uint16_t *e;        /* per-column errors                                   */
} dcr_out;

/* Per-read preprocessing results (exported so the host can rebuild the
 * preprocessed input records the reference would tag; optional). */
typedef struct dcr_read_info {
    int64_t seq_start;  /* offset of the first kept base (after 5' soft clip)  */
    int32_t len;        /* kept length after 3' N trim                         */
    int32_t n_cig;      /* normalised cigar ops (M/I/D only)                   */
    int32_t status;     /* DCR_ST_*                                            */
    int32_t has_ins;    /* any I op kept                                       */
} dcr_read_info;

typedef struct dcr_ctx dcr_ctx;

/* library */
int dcr_abi_version(void);
const char *dcr_last_error(void);

/* context: one per GPU (not thread-safe per context) */
dcr_ctx *dcr_create(int device, const dcr_params *params);
void dcr_destroy(dcr_ctx *ctx);
int dcr_set_params(dcr_ctx *ctx, const dcr_params *params);
int dcr_set_options(dcr_ctx *ctx, int flags);   /* DCR_OPT_* */
/* pre-size internal scratch so a timed loop never allocates */
int dcr_reserve(dcr_ctx *ctx, const dcr_batch *sizes);
void *dcr_stream(dcr_ctx *ctx);   /* the context's hipStream_t */

/* device-pointer batch: asynchronous on the context stream */
int dcr_run_batch(dcr_ctx *ctx, const dcr_batch *in, dcr_out *ss, dcr_out *ds);
/* host-pointer batch: stages H2D, runs, D2H; synchronous */
int dcr_run_batch_host(dcr_ctx *ctx, const dcr_batch *in, dcr_out *ss, dcr_out *ds);
int dcr_sync(dcr_ctx *ctx);
/* copy the last batch's per-read preprocessing info (host pointer, n_reads);
   complete only with DCR_OPT_READ_INFO */
int dcr_read_info_host(dcr_ctx *ctx, dcr_read_info *out, int64_t n_reads);
/* timing of the last dcr_run_batch (HIP events on the context stream), ms:
   [0] prep (always 0: fused into the consensus kernels), [1] single-strand,
   [2] duplex, [3] whole batch */
int dcr_last_timing(dcr_ctx *ctx, float *ms4);
/* per-kernel timing of the last dcr_run_batch (HIP events between launches on
   the context stream), ms: per strand (single-strand, duplex) k_recmeta,
   k_consensus_fast, k_consensus_fast (exact queue), k_consensus_general */
#define DCR_N_KERNEL_TIMES 8
int dcr_last_kernel_timing(dcr_ctx *ctx, float *ms8);

/* Streaming: a context has DCR_MAX_SLOTS slots of device buffers.
 * dcr_submit copies a host batch (pinned memory, dcr_host_alloc) into the
 * slot on a copy stream, runs it on the compute stream and copies the
 * outputs back into the host dcr_out arrays on a second copy stream (NULL
 * fields are not copied); it returns at once.  read_status (optional,
 * n_reads int32) receives dcr_read_info.status of every read.  dcr_wait
 * blocks until the slot's outputs are on the host.  Batches run on the
 * device in submission order; H2D of one batch and D2H of another overlap
 * the kernels of a third. */
#define DCR_MAX_SLOTS 4
void *dcr_host_alloc(size_t bytes);
void dcr_host_free(void *p);
int dcr_submit(dcr_ctx *ctx, int slot, const dcr_batch *host_in, dcr_out *host_ss, dcr_out *host_ds,
               int32_t *read_status);
int dcr_wait(dcr_ctx *ctx, int slot);

/* Device record writer.  dcr_submit_write is dcr_submit followed, on the
 * device, by the reference's per-family outcome (what make_consensus_read /
 * preprocess_family raise, in its order), the two duplex BAM records of every
 * family that does not fail (make_consensus_read :1352-1384, add_tags
 * :1076-1120, fix_paired_end_fields :1390-1419), formatted as the host writer
 * (libdcr_io dcr_fmt_write) formats them, and their BGZF compression; only
 * the compressed blocks, the outcomes and the duplex lengths come back.
 * dcr_wait_write waits for the slot and copies the blocks into res->bgzf.
 * The formatted records stay in the slot until it is submitted again
 * (dcr_slot_fetch: what 0 = record bytes, 1 = int64 record offsets [2F+1],
 * 2 = the BGZF blocks again, e.g. after dcr_wait_write found cap_bgzf too
 * small: totals[0] holds the size). */
typedef struct dcr_wmeta {
    const char *names;           /* string arena (dcr_host_batch.names)          */
    int64_t n_names;
    const int64_t *fam_code;     /* [F] offsets of the family codes (MI prefix)  */
    const int64_t *fam_rx;       /* [2F] offsets of RX of the A1 / B1 read0      */
    const int32_t *fam_tid;      /* [F] reference_id                             */
} dcr_wmeta;
typedef struct dcr_wres {        /* pinned host memory                          */
    uint8_t *bgzf;               /* BGZF blocks of the batch's records, in order */
    int64_t cap_bgzf;
    int32_t *fam_fail;           /* [F] DCR_FAIL_* | which << 8 (include/dcr_io.h), 0: written */
    int32_t *ds_len;             /* [2F] duplex consensus lengths                */
    int64_t *totals;             /* [3] BGZF bytes, record bytes, BGZF blocks    */
} dcr_wres;
int dcr_submit_write(dcr_ctx *ctx, int slot, const dcr_batch *host_in, const dcr_wmeta *meta, dcr_wres *res);
int dcr_wait_write(dcr_ctx *ctx, int slot, dcr_wres *res);
int dcr_slot_fetch(dcr_ctx *ctx, int slot, int what, int64_t off, int64_t n, void *dst);

/* The single-strand consensus reads as a second stream.  dcr_submit_write_ss
 * is dcr_submit_write and, for every family that does not fail, the four
 * records make_consensus_read(method="single_strand") returns (:1352-1384;
 * order A1 B2 B1 A2; name get_consensus_id :909-920, flag of the subfamily's
 * first read :957-958, tags MI RX sQ sd sD sM se sE add_tags :1054-1073, no
 * mate fields), formatted as libdcr_io's dcr_fmt_write_ss formats them and
 * BGZF-compressed on their own.  res_ss: bgzf, cap_bgzf and totals are used.
 * dcr_wait_write_ss fills both results; on DCR_ECAPACITY the totals[0] of the
 * two tell which stream's blocks to fetch again.  dcr_slot_fetch: what 3 =
 * single-strand record bytes, 4 = their int64 record offsets [4F+1], 5 =
 * their BGZF blocks. */
typedef struct dcr_wmeta_ss {
    const uint16_t *sub_flag;    /* [4F] flag of each subfamily's first read       */
    const int64_t *sub_mi;       /* [4F] offsets in dcr_wmeta.names of its whole MI */
    const int64_t *sub_rx;       /* [4F] offsets of its RX                          */
} dcr_wmeta_ss;
int dcr_submit_write_ss(dcr_ctx *ctx, int slot, const dcr_batch *host_in, const dcr_wmeta *meta,
                        const dcr_wmeta_ss *meta_ss, dcr_wres *res, dcr_wres *res_ss);
int dcr_wait_write_ss(dcr_ctx *ctx, int slot, dcr_wres *res, dcr_wres *res_ss);

/* Consensus filters (not a reference feature; the step fgbio's
 * FilterConsensusReads does on the written file).  With a filter set on the
 * context, dcr_submit_write[_ss] first masks, in the slot's duplex seq / qual,
 * every base of a family that does not fail whose quality is below
 * min_base_quality ('N', quality min(q, 2)), then tests both duplex records
 * k = 2f + j (built from single-strand records a = 4f + 2j, b = a + 1) against
 * the active rules.  A family is written iff both records pass every rule;
 * a dropped family's records (and its four single-strand records) get size 0.
 *   DCR_FILT_MIN_READS  D[a] + D[b] >= min_reads[0], max >= [1], min >= [2]
 *   DCR_FILT_ERROR_RATE ds.E[k] <= max_error_rate[0], ss.E[a], ss.E[b] <= [1]
 *                       (IEEE compares: NaN fails)
 *   DCR_FILT_NO_CALL    !( (double)n > max_no_call_fraction * (double)len ),
 *                       n = 'N' bases after masking
 *   DCR_FILT_MEAN_QUAL  !( (double)s < min_mean_base_quality * (double)len ),
 *                       s = sum of the qualities after masking
 * (one double multiply each, no fused contraction).  The per-family outcome
 * word fam_filt[f]: low byte = the DCR_FILT_* bits of the rules that failed
 * (1 min_reads, 2 error rate, 4 no-call fraction, 8 mean quality), the union
 * over both records; bits 8 and up = bases masked in the family's two records; 0 for
 * failing families, which are not filtered. */
#define DCR_FILT_MIN_READS 1     /* active bits; the first four are also reason bits */
#define DCR_FILT_ERROR_RATE 2
#define DCR_FILT_NO_CALL 4
#define DCR_FILT_MEAN_QUAL 8
#define DCR_FILT_MASK_BASES 16
typedef struct dcr_filter {
    int32_t active;               /* DCR_FILT_* bits; 0: no filter             */
    int32_t min_base_quality;     /* DCR_FILT_MASK_BASES                       */
    int32_t min_reads[3];         /* total, larger strand, smaller strand      */
    int32_t reserved0;
    double max_error_rate[2];     /* duplex, single strand                     */
    double max_no_call_fraction;
    double min_mean_base_quality;
} dcr_filter;
/* NULL or active == 0: off (the default; nothing is launched or copied).
 * Holds for the batches submitted after the call. */
int dcr_set_filter(dcr_ctx *ctx, const dcr_filter *filter);
/* Where a slot's fam_filt[F] goes (pinned host memory, at least n_fam int32
 * of every batch submitted on the slot while a filter is set): copied with
 * fam_fail, on the same stream and before the same event, so it is complete
 * when dcr_wait_write[_ss] returns.  NULL removes it. */
int dcr_slot_filter_out(dcr_ctx *ctx, int slot, int32_t *fam_filt);

/* Per-base consensus filters (not a reference feature; the per-base rules of
 * fgbio's FilterConsensusReads: --min-reads per base and
 * --require-single-strand-agreement).  They mask single duplex bases by the
 * raw-read support and the agreement at the alignment column the base came
 * from.  oracle/dcr_oracle.py (consensus_core, reconstruct) is the
 * executable form of the alignment; tests/base_filter_model.py restates the
 * rules over it.
 *
 * Level 1, the column of a base.  For a consensus record (single-strand s or
 * duplex r) let cons be the aligned consensus string (what consensus_core
 * returns as cons: one char per alignment column, '+' where an insertion
 * column was called absent, '-' for a deletion, lower case for a called
 * insertion).  The d-index of a column counts the columns before it whose
 * cons is not '+', so the d / e lists have one entry per d-index (n_de of
 * them).  [t5, t3) is the window the 'N' trim leaves (:770-784; upper-case
 * 'N' only).  Base i of seq is the i-th column inside the window whose cons
 * is neither '+' nor '-'; col(i) is that column's d-index.
 *
 * Level 2, the source bases of a duplex column.  Duplex record r = 2f + j is
 * called from the single-strand records a = 4f + 2j and b = a + 1, laid out
 * as reconstruct([pos_a, pos_b], [cigar_a, cigar_b], [seq_a, seq_b], ..) lays
 * them out (:430-547), quirks included: a column in which either strand's
 * current CIGAR operation is I is an insertion column (the other strand gets
 * '+') and still consumes one reference position, and the layout ends at
 * max(pos + len(seq)).  Every duplex alignment column then holds, per
 * strand, a base index ia / ib into that strand's seq, or nothing ('N'
 * padding, '-', '+').
 *
 * For duplex base i at alignment column t with c = col_r(i):
 *   aD = ss.d[a][col_a(ia)], aE = ss.e[a][col_a(ia)]  (0, 0 when strand a has
 *   no base in column t); bD, bE likewise; cE = ds.e[r][c].
 * Rules (each masks the base exactly as DCR_FILT_MASK_BASES does: 'N',
 * quality min(q, 2), nothing else of the record touched, no re-trim):
 *   DCR_BF_MIN_READS   keep iff aD + bD >= min_reads[0], max(aD, bD) >= [1],
 *                      min(aD, bD) >= [2]
 *   DCR_BF_ERROR_RATE  mask iff (double)(aE + bE) > max_error_rate *
 *                      (double)(aD + bD)   (one double multiply, no fused
 *                      contraction)
 *   DCR_BF_AGREEMENT   mask iff cE > 0
 * The bases masked are the union of these and of DCR_FILT_MASK_BASES; the
 * masking comes before the record rules DCR_FILT_NO_CALL and
 * DCR_FILT_MEAN_QUAL count 'N' and sum qualities, and fam_filt[f] >> 8 counts
 * every masked base once.  Failing families are not touched.  With a base
 * filter set, fam_filt is produced (dcr_slot_filter_out) as with a filter. */
#define DCR_BF_MIN_READS 1
#define DCR_BF_ERROR_RATE 2
#define DCR_BF_AGREEMENT 4
typedef struct dcr_base_filter {
    int32_t active;               /* DCR_BF_* bits; 0: off                     */
    int32_t min_reads[3];         /* total, larger strand, smaller strand      */
    double max_error_rate;        /* in [0, 1]                                 */
} dcr_base_filter;
/* NULL or active == 0: off (the default; nothing is launched, copied, zeroed
 * or allocated).  Holds for the batches submitted after the call.
 * dcr_slot_fetch what 6 (a batch submitted with a base filter set, or with
 * the per-base tags or the base metrics on, dcr_set_base_tags /
 * dcr_set_base_metrics): one byte
 * per record, single-strand 4F then duplex 2F, 1 where the consensus kernels
 * stored the record's column map (it has insertion columns), 0 where the map
 * follows from pos and CIGAR (diagnostic; the tests read it). */
int dcr_set_base_filter(dcr_ctx *ctx, const dcr_base_filter *filter);

/* Per-base tags (not a reference feature; the array and string types that
 * fgbio's FilterConsensusReads / ReviewConsensusVariants and pileup-style
 * callers expect under these tag names: conformance is to the types stated
 * here, fgbio itself was not run).  With the tags on, the ten tags ad bd cd ae
 * be ce ac bc aq bq of every duplex record dcr_submit_write[_ss] writes keep
 * their names and their places in the tag order and carry one value per base
 * of the record's seq, in seq order, instead of one per alignment column.
 * Levels 1 and 2 are the per-base filters' above.  For duplex record
 * r = 2f + j, called from a = 4f + 2j and b = a + 1, and base i of its seq
 * (len bases): c = col_r(i); (ia, ib) the strands' base indices in that
 * alignment column; ca = col_a(ia), cb = col_b(ib).
 *   ad ae bd be  B:s, len entries: ad[i] = min(ss.d[a][ca], 32767), ae[i] =
 *                min(ss.e[a][ca], 32767), both 0 when strand a has no base in
 *                the column; bd be the same for strand b
 *   cd ce        B:s, len entries: cd[i] = min(ds.d[r][c], 32767), ce likewise
 *   ac bc        Z of exactly len characters: ac[i] = ss.seq[a][ia], or 'N'
 *                when strand a has no base there
 *   aq bq        Z of exactly len characters: aq[i] = chr(ss.qual[a][ia] + 33),
 *                or '!' (a written family has no strand quality >= 95: the
 *                reference fails it at :1384, fam_fail says so)
 * Every other field and tag of the record (MI RX aQ bQ cQ, aD..cE, name, flag,
 * CIGAR, SEQ, QUAL) is byte for byte what it is without the tags.  Of the
 * single-strand records s (dcr_submit_write_ss), sd and se become B:s of len
 * entries, sd[i] = min(ss.d[s][col_s(i)], 32767) and se likewise (Level 1
 * only); MI RX sQ sD sM sE do not change.  The tags describe the consensus as
 * called: no filter touches ss.*, ds.d, ds.e or the maps, so a masked base
 * keeps its values; dropped and failing families write nothing, as without.
 * Every index is clamped to its record's region before use.
 * on != 0: on; 0: off (the default; nothing else is launched, copied, zeroed
 * or allocated and no output byte changes).  Holds for the batches submitted
 * after the call.  dcr_slot_fetch what 6 serves such a batch too. */
int dcr_set_base_tags(dcr_ctx *ctx, int on);

/* Consensus QC tables (not a reference feature; what fgbio's
 * CollectDuplexSeqMetrics / ErrorRateByReadPosition read off the written
 * file).  With metrics on, dcr_submit_write[_ss] counts, over the families f
 * of the batch with fam_fail[f] == 0 and before any filter masks or drops,
 * the consensus as called.  Single-strand records s = 4f + k (k = A1 B2 B1
 * A2), duplex records r = 2f + j built from a = 4f + 2j and b = a + 1.  len
 * and n_de are clamped to [0, the record's region], as the filter clamps len.
 *   n[0] families, [1] sum ss.len, [2] sum ds.len, [3] duplex bases == 'N',
 *        [4] sum ss.n_de, [5] sum ds.n_de, [6] [7] 0
 *   ss_reads[k][min(n, 255)]       n = sub_off[s+1] - sub_off[s]
 *   ds_depth[min(hi, 63)][min(lo, 63)]  per duplex record: the larger and the
 *        smaller of ss.D[a], ss.D[b], below 0 counted as 0
 *   err_c[bin(ds.E[r])], err_s[max(bin(ss.E[a]), bin(ss.E[b]))]  per duplex
 *        record; bin(E) = (int)rint(E * 1000.0) when E >= 0 && E <= 1, else
 *        DCR_MET_ERR_BINS - 1 (NaN too); one double multiply
 *   ss_qual[q], ds_qual[q]         every quality byte in [0, len)
 *   col[kind][what][min(c', 511)]  kind 0 ss, 1 ds; what 0 records that have
 *        the column, 1 sum of d, 2 sum of e; for every column c < n_de,
 *        c' = c for forward records (ss k = 0, 1; ds j = 0) and
 *        c' = n_de - 1 - c for reverse ones (ss k = 2, 3; ds j = 1): the
 *        column counted from the read's sequencing 5' end
 * Every table is an integer sum, so totals over batches or devices are sums
 * of the blocks in any order. */
#define DCR_MET_READS_BINS 256
#define DCR_MET_DEPTH_BINS 64
#define DCR_MET_ERR_BINS 1002
#define DCR_MET_QUAL_BINS 256
#define DCR_MET_COL_BINS 512
typedef struct dcr_metrics {
    uint64_t n[8];
    uint64_t ss_reads[4][DCR_MET_READS_BINS];
    uint64_t ds_depth[DCR_MET_DEPTH_BINS][DCR_MET_DEPTH_BINS];
    uint64_t err_c[DCR_MET_ERR_BINS];
    uint64_t err_s[DCR_MET_ERR_BINS];
    uint64_t ss_qual[DCR_MET_QUAL_BINS];
    uint64_t ds_qual[DCR_MET_QUAL_BINS];
    uint64_t col[2][3][DCR_MET_COL_BINS];
} dcr_metrics;
/* on != 0: count (k_metrics, between the failure scan and the filter); 0: off
 * (the default; nothing is launched, copied or allocated).  Holds for the
 * batches submitted after the call. */
int dcr_set_metrics(dcr_ctx *ctx, int on);
/* Where a slot's counters go (pinned host memory, one dcr_metrics, written
 * whole for every batch submitted on the slot while metrics are on: the
 * batch's own counts, not a running total): copied with fam_fail, on the same
 * stream and before the same event, so it is complete when
 * dcr_wait_write[_ss] returns.  NULL removes it. */
int dcr_slot_metrics_out(dcr_ctx *ctx, int slot, dcr_metrics *pinned_dst);

/* Per-base duplex QC tables (not a reference feature; the per-base half of the
 * QC tables above: what a user would otherwise count over the per-base tags of
 * the written file).  With base metrics on, dcr_submit_write[_ss] counts, over
 * the families f of the batch with fam_fail[f] == 0 and before any filter masks
 * or drops, every base of the duplex consensus as called.  Levels 1 and 2 are
 * the per-base filters' above.  For duplex record r = 2f + j, called from
 * a = 4f + 2j and b = a + 1, and base i in [0, len): (c, ia, ib, ca, cb) are
 * exactly those of dcr_set_base_tags; every index is clamped to its record's
 * region, and a column outside [0, n_de) counts as 0, as the tags do.
 *   aD = ss.d[a][ca], aE = ss.e[a][ca], both 0 when strand a has no base in
 *        the column (not clamped to 32767); bD, bE the same for strand b;
 *        cE = ds.e[r][c]
 *   x = code(ss.seq[a][ia]), y = code(ss.seq[b][ib]): A a 0, C c 1, G g 2,
 *        T t 3, anything else 4
 *   cls = 0 when both strands have a base and x == y (two 'N' agree), 1 when
 *        both have a base and x != y, 2 otherwise
 *   s = aD + bD, e = aE + bE
 *   i' = i for j = 0 and len - 1 - i for j = 1: the cycle counted from the
 *        read's sequencing 5' end (the orientation rule of dcr_metrics.col)
 * Tables:
 *   n[0] duplex records, [1] bases, [2] bases with both strands present, [3]
 *        strand a only, [4] strand b only, [5] neither, [6] cls == 1, [7] cE > 0
 *   pair[j][x][y]      bases with both strands present, in SEQ orientation;
 *        split by j so that the reverse read can be folded by complementing
 *   depth[min(max(aD, bD), 63)][min(min(aD, bD), 63)]   every base
 *   err[bin]           every base; bin = (s > 0 && e <= s) ? (1000 * e) / s :
 *        DCR_BMET_ERR_BINS - 1, integer division
 *   qual[cls][ds.qual[r][i]]   every base, the quality as called (unmasked)
 *   cyc[j][what][min(i', 511)]  what 0 bases, 1 ds.seq[r][i] == 'N', 2
 *        cls == 1, 3 cls == 2, 4 sum of s, 5 sum of e
 * Every table is an integer sum (the error bin too: no floating point), so
 * totals over batches or devices are sums of the blocks in any order.
 * Reading the per-base rules off the tables:
 *   --filter_min_base_reads T,A,B masks the bases of the depth bins [hi][lo]
 *        that fail hi + lo >= T, hi >= A, lo >= B (exact while T, A, B stay
 *        below the clamp, 63);
 *   --filter_require_strand_agreement masks n[7] bases;
 *   --filter_max_base_error_rate X masks about the sum of err above bin
 *        1000 * X (bin 1001 included): approximate, because the rule compares
 *        in doubles and the bins are floors of integer quotients. */
#define DCR_BMET_DEPTH_BINS 64
#define DCR_BMET_ERR_BINS 1002
#define DCR_BMET_QUAL_BINS 256
#define DCR_BMET_CYC_BINS 512
typedef struct dcr_base_metrics {
    uint64_t n[8];
    uint64_t pair[2][5][5];
    uint64_t depth[DCR_BMET_DEPTH_BINS][DCR_BMET_DEPTH_BINS];
    uint64_t err[DCR_BMET_ERR_BINS];
    uint64_t qual[3][DCR_BMET_QUAL_BINS];
    uint64_t cyc[2][6][DCR_BMET_CYC_BINS];
} dcr_base_metrics;     /* 12,068 words, 96,544 bytes */
/* on != 0: count (k_base_metrics, after the failure scan and k_metrics, before
 * the filters); 0: off (the default; nothing is launched, copied, zeroed or
 * allocated and no output byte changes).  The column maps are made as for a
 * base filter or the per-base tags, and dcr_slot_fetch what 6 serves such a
 * batch too.  Holds for the batches submitted after the call. */
int dcr_set_base_metrics(dcr_ctx *ctx, int on);
/* Where a slot's per-base counters go (pinned host memory, one
 * dcr_base_metrics, written whole for every batch submitted on the slot while
 * base metrics are on: the batch's own counts, not a running total): copied
 * with fam_fail, on the same stream and before the same event, so it is
 * complete when dcr_wait_write[_ss] returns.  NULL removes it. */
int dcr_slot_base_metrics_out(dcr_ctx *ctx, int slot, dcr_base_metrics *pinned_dst);

/* Overlapping mates (not a reference feature; the step that fgbio's
 * overlapping-bases consensus or ClipBam --clip-overlapping-reads do on the
 * written file: the rules below are the specification, fgbio was not run).
 * The two duplex records 2f and 2f + 1 of a family are mates on the same
 * reference (fam_tid[f]); where both have an aligned base on a reference
 * position the molecule is reported twice.  With a mode set,
 * dcr_submit_write[_ss] compares the two records of every family that does
 * not fail at each such position and rewrites their seq / qual in the slot,
 * after the QC tables are counted and before any filter, the formatters and
 * the compressor.  No other field changes (length, CIGAR, position, flag, mate
 * fields, TLEN, every tag with or without dcr_set_base_tags), and no
 * single-strand record does.
 *
 * The map of a record, from what is written of it: start pos, CIGAR, and len
 * clamped to [0, the record's region] (n_cig likewise).  The CIGAR is walked
 * with SAM semantics in 64-bit arithmetic: M, = and X give n bases on n
 * consecutive reference positions; I and S give n bases and no position; D
 * and N give n positions and no base; H and P (and the unused operation
 * codes) give neither.  A base index at or past len is not in the map.  This
 * is not reconstruct_alignment's layout, and the stored column maps of the
 * per-base filters are not used.
 *
 * For every reference position p in both maps, with base indices i0 / i1,
 * (x, qx) = (seq0[i0], qual0[i0]) and (y, qy) = (seq1[i1], qual1[i1]), bytes
 * compared as stored:
 *   x == 'N' or y == 'N'   nothing changes; the position is not compared
 *   x == y                 DCR_OVL_MASK: nothing changes
 *                          DCR_OVL_CONSENSUS: both qualities min(qx + qy, 93)
 *   x != y                 DCR_OVL_MASK: both bases 'N', each at min(its own
 *                          quality, 2)
 *                          DCR_OVL_CONSENSUS: qx > qy: both bases x at quality
 *                          qx - qy; qy > qx: both y at qy - qx; qx == qy: both
 *                          masked as DCR_OVL_MASK does
 * Every result comes from the values before the step; a base has at most one
 * reference position, so the pairs are independent.
 *
 * fam_ovl[3f .. 3f + 2]: compared (positions with both bases not 'N'),
 * disagree (the compared positions with x != y), changed (bases, over both
 * records, whose seq or qual byte changed); 0 0 0 for a failing family, which
 * is not touched.  k_metrics and k_base_metrics run before the step and
 * describe the consensus as called; k_base_filter and k_filter run after it,
 * see the records as it left them and count by their own definitions.  The
 * mode alone launches no filter and produces no fam_filt. */
#define DCR_OVL_MASK 1
#define DCR_OVL_CONSENSUS 2
/* mode 0: off (the default; nothing is launched, copied, zeroed or allocated
 * and no output byte changes); any value but 0, DCR_OVL_MASK and
 * DCR_OVL_CONSENSUS is DCR_EARG.  Holds for the batches submitted after the
 * call. */
int dcr_set_mate_overlap(dcr_ctx *ctx, int mode);
/* Where a slot's fam_ovl[3F] goes (pinned host memory, at least 3 * n_fam
 * int32 of every batch submitted on the slot while a mode is set): copied with
 * fam_fail, on the same stream and before the same event, so it is complete
 * when dcr_wait_write[_ss] returns.  NULL removes it. */
int dcr_slot_overlap_out(dcr_ctx *ctx, int slot, int32_t *fam_ovl);

/* Allele counts at given sites (not a reference feature; what a molecule-aware
 * pileup of the written file would count: the rules below are the
 * specification, no pileup tool was run).  With sites set,
 * dcr_submit_write[_ss] counts, for every site and over the families that are
 * written, which allele the molecule shows there.  A molecule is a family, not
 * a record: where both duplex records cover a site they give one count.
 *
 * Which records count: the two duplex records 2f and 2f + 1 of a family f with
 * fam_fail[f] == 0 that no filter rule dropped (fam_filt[f] & 0xff == 0 where a
 * filter is set), as they are written: after k_mate_overlap, k_base_filter and
 * k_filter, before the formatters.  No single-strand record counts.  A site
 * (tid, pos) matches a family only when tid == fam_tid[f].
 *
 * The map of a record is the one of dcr_set_mate_overlap above (pos, CIGAR,
 * len and n_cig clamped to the record's region, 64-bit arithmetic), with one
 * addition: a D run gives the call `del` on each of its positions.  N runs
 * give positions without a call; I and S give bases without a position; H and
 * P give neither.  The walk ends where that one ends: at the last operation,
 * or once the base index has reached len (an operation after the last base of
 * the map, a D run included, gives nothing).
 *
 * The call of a record at position p:
 *   none    the map has nothing at p
 *   5 del   p lies in a D run
 *   else from the base byte as stored: 'A' 'C' 'G' 'T' give 0 1 2 3, any other
 *           byte 4 (N); a base whose qual < min_base_quality gives 4 too
 * The molecule's call from the calls c0, c1 of its two records:
 *   one of them present            that call
 *   both present and equal         that call
 *   exactly one of them 4 (N)      the other (a del too)
 *   otherwise                      6 (discordant)
 * table[i][0..6] count the molecules by that call at site i (A C G T N del
 * discordant); table[i][7] (both) counts the molecules whose two records both
 * have a call there, whatever it is: how often a plain pileup would have
 * counted the molecule twice.  So every family adds exactly one to one of the
 * columns 0..6 of every site either record covers, and nothing elsewhere.
 *
 * keys[i] = (int64_t)tid << 32 | pos with pos 0-based, 0 <= tid, pos < 2^31,
 * strictly increasing, 0 < n <= DCR_ALLELE_MAX_SITES; anything else is
 * DCR_EARG and leaves the state as it was.  n == 0 or keys == NULL turns the
 * feature off and frees the table: the default, in which nothing is
 * allocated, launched, copied or zeroed and no output byte changes.  n > 0
 * waits for the batches in flight, uploads the keys and allocates and zeroes a
 * device table uint64[n][8] that lives on the context, not on a slot (a panel
 * can hold millions of sites; a copy per batch would cost more than the
 * kernel): every call gives a fresh table, also with the keys of the last one.
 * The table accumulates over every dcr_submit_write[_ss] after the call, from
 * any slot (k_allele_counts, after the filters and before k_fmt_size, on the
 * slot's stream; plain 64-bit atomics, so sums over batches, slots and
 * devices are order-free).  min_base_quality < 0 is DCR_EARG.  The option
 * changes no other output. */
#define DCR_ALLELE_MAX_SITES (1 << 24)
#define DCR_ALLELE_COLS 8
int dcr_set_allele_sites(dcr_ctx *ctx, const int64_t *keys, int64_t n, int min_base_quality);
/* The table so far into dst (host memory, uint64[n][DCR_ALLELE_COLS]): waits
 * for every batch submitted so far on any slot, then copies.  The table is not
 * reset and goes on accumulating.  DCR_EARG when no sites are set. */
int dcr_allele_counts_fetch(dcr_ctx *ctx, uint64_t *dst);

/* Errors against a genome (not a reference-script feature; "genome" is the
 * reference FASTA, because "reference" means the reference script here.  What a
 * mismatch counter run over the written files would count: the rules below are
 * the specification, no other tool was run).  With a genome set,
 * dcr_submit_write[_ss] compares every aligned base of the consensus records as
 * called with the genome's base on its position and counts.
 *
 * Which records count, over the families f of the batch with fam_fail[f] == 0:
 *   lv 0   the four single-strand records s = 4f + k, whether or not the
 *          single-strand stream is written; their read index is j = k >> 1
 *   lv 1   the two duplex records r = 2f + j
 * as called: before k_mate_overlap and before every filter, beside
 * k_base_metrics.
 *
 * The map of a record is the one of dcr_set_mate_overlap above (pos, CIGAR with
 * SAM semantics in 64-bit arithmetic, len and n_cig clamped to the record's
 * region; the walk ends at the last operation or once the base index has
 * reached len).  An M / = / X run of n gives min(n, len - base index) bases
 * with a position.  Of an I run the run counts once and min(n, len - base
 * index) bases; of a D run the run counts once and n positions.  S, N, H, P
 * and the unused codes count nothing.  An operation at or past len is not
 * reached and counts nothing.
 *
 * The genome: codes[] holds one byte per base, A C G T as 0 1 2 3 and anything
 * else 4, for n_ref sequences back to back; sequence t is
 * codes[ref_off[t] .. ref_off[t + 1]), of length 0 when the FASTA lacks it.
 *   code(t, p) = codes[ref_off[t] + p] when 0 <= t < n_ref and
 *                0 <= p < ref_off[t + 1] - ref_off[t]; otherwise 4
 * For base i of a record of family f on position p, with t = fam_tid[f]:
 *   g = code(t, p), g5 = code(t, p - 1), g3 = code(t, p + 1)
 *   x = the base's code: A a 0, C c 1, G g 2, T t 3, anything else 4 (the
 *       code of dcr_base_metrics.pair)
 *   q = the record's quality byte of the base
 *   i' = i for j = 0 and len - 1 - i for j = 1 (dcr_base_metrics.cyc's cycle
 *       from the sequencing 5' end), len the clamped one
 * Tables:
 *   n[lv][0]  records            [1] bases with a position
 *        [2]  of those g < 4 && x < 4 && g == x       [3] g < 4 && x < 4 && g != x
 *        [4]  g < 4 && x == 4    [5] g == 4 (past either end of the sequence,
 *             an absent sequence and a tid outside [0, n_ref) included)
 *        [6]  I runs   [7] I bases   [8] D runs   [9] D positions   [10] [11] 0
 *        so [1] == [2] + [3] + [4] + [5]
 *   sub[lv][j][g][x]        the bases with g < 4 && x < 4, in the genome's
 *        orientation (as SEQ is stored), the diagonal included; split by j so
 *        that the reverse read can be folded by complementing
 *   tri[lv][j][g5][g][g3][x]   where sub counts and g5 < 4 && g3 < 4 (so never
 *        at the first or the last position of a sequence)
 *   cyc[lv][j][what][min(i', 511)]   what 0: where sub counts; 1: of those g != x
 *   qual[lv][what][q]       what as in cyc
 * Every table is an integer sum: totals over batches or devices are sums of
 * the blocks in any order.  Mismatches at true variants are in the counts. */
#define DCR_GMET_CYC_BINS 512
#define DCR_GMET_QUAL_BINS 256
typedef struct dcr_genome_metrics {
    uint64_t n[2][12];
    uint64_t sub[2][2][4][4];
    uint64_t tri[2][2][4][4][4][4];
    uint64_t cyc[2][2][2][DCR_GMET_CYC_BINS];
    uint64_t qual[2][2][DCR_GMET_QUAL_BINS];
} dcr_genome_metrics;   /* 6,232 words, 49,856 bytes */
/* The genome onto the device.  codes / ref_off are host memory (pageable is
 * fine; copied in chunks), ref_off[0] == 0, non-decreasing, n_ref + 1 entries,
 * every code <= 4; anything else is DCR_EARG and leaves the state as it was.
 * Waits for the batches in flight, then uploads into device memory that lives
 * on the context and turns the counting on for the batches submitted afterwards
 * (k_genome_metrics, once per level, after k_base_metrics' place and before
 * k_mate_overlap, on the slot's stream).  n_ref == 0 or a NULL pointer frees the
 * memory and turns the counting off: the default, in which nothing is
 * allocated, uploaded, launched, copied or zeroed and no output byte changes.
 * With the counting on no output byte changes either. */
int dcr_set_genome(dcr_ctx *ctx, const uint8_t *codes, const int64_t *ref_off, int32_t n_ref);
/* Where a slot's block goes (pinned host memory, one dcr_genome_metrics,
 * written whole for every batch submitted on the slot while a genome is set:
 * the batch's own counts, not a running total): copied with fam_fail, on the
 * same stream and before the same event, so it is complete when
 * dcr_wait_write[_ss] returns.  NULL removes it. */
int dcr_slot_genome_metrics_out(dcr_ctx *ctx, int slot, dcr_genome_metrics *pinned_dst);

/* CPU restatement with the same contract (oracle/, test infrastructure):
   host pointers, single thread (or n_threads > 1) */
int dcr_oracle_run(const dcr_params *params, const dcr_batch *in, dcr_out *ss, dcr_out *ds,
                   dcr_read_info *info, int n_threads);

#ifdef __cplusplus
}
#endif
#endif /* DCR_H */
