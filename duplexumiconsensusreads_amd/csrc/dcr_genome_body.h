// The per-record body of k_genome_metrics (dcr_writer.hip; include/dcr.h
// dcr_genome_metrics states the rules).  It is written over a handful of wave
// primitives that the including file defines before the #include, so that the
// same text also compiles for the host, where the 64 lanes of a record run one
// after the other (exact, because the lanes share nothing but the tables):
//   GM_FN                      the function qualifiers
//   int gm_lane()              the lane, 0 .. 63
//   uint64 gm_pop(bool p)      how many lanes of the wave hold p (on the host: this lane's own p)
//   uint64 gm_once(uint64 v)   a value every lane holds alike, counted once per wave
//                              (the device: v, the wave's n[] are added by one lane; the host: v in lane 0)
//   gm_count(h, bin, act)      +1 into h[bin] for the lanes with act, the hot bin merged (bm_count)
//   gm_wave_add(p, pred)       the number of lanes with pred into *p, by one lane
//   gm_add(p)                  +1 into *p by this lane
//   int gm_code(uint8_t)       A a 0, C c 1, G g 2, T t 3, else 4
// Every lane of the wave calls gm_record with the same record; the walk of the
// CIGAR is the same in every lane, so every loop and branch but the ones on a
// lane's own base is wave-uniform.
#ifndef DCR_GENOME_BODY_H
#define DCR_GENOME_BODY_H

// a record's map (dcr_set_mate_overlap's): len and ncig clamped to the record's region
struct GmRec {
    const uint32_t *cig;
    const uint8_t *seq, *qual;
    int64_t len, ncig, pos;
};

// one level's tables as 32-bit bins: sub[2][4][4], tri[2][4][4][4][4], cyc[2][2][512], qual[2][256]
constexpr int kGmSub = 0;
constexpr int kGmTri = kGmSub + 2 * 16;
constexpr int kGmCyc = kGmTri + 2 * 256;
constexpr int kGmQual = kGmCyc + 2 * 2 * DCR_GMET_CYC_BINS;
constexpr int kGmBins = kGmQual + 2 * DCR_GMET_QUAL_BINS;      // 3,104 bins, 12,416 bytes

// the genome's code at p of a sequence of glen codes at g (outside: 4; a code above 4 reads as 4)
GM_FN int gm_at(const uint8_t *g, int64_t glen, int64_t p) {
    if (p < 0 || p >= glen) return 4;
    const int c = g[p];
    return c < 4 ? c : 4;
}

// record R of read index j on the sequence (g, glen): n[] is the wave's own, cnt the level's bins
GM_FN void gm_record(const GmRec &R, int j, const uint8_t *g, int64_t glen, unsigned long long (&n)[12], uint32_t *cnt) {
    const int64_t L = R.len;
    const int last_bin = DCR_GMET_CYC_BINS - 1;
    uint32_t *cyc = cnt + kGmCyc + j * 2 * DCR_GMET_CYC_BINS;
    n[0] += gm_once(1);
    int64_t rp = R.pos, bi = 0;
    for (int64_t k = 0; k < R.ncig && bi < L; ++k) {
        const uint32_t v = R.cig[k];
        const int64_t run = v >> 4;
        const uint32_t op = v & 15u;
        const int64_t here = run < L - bi ? run : L - bi;       // the run's bases inside the map
        if (op == 0u || op == 7u || op == 8u) {
            for (int64_t t0 = 0; t0 < here; t0 += 64) {
                const int64_t t = t0 + gm_lane();
                const bool act = t < here;
                const int64_t i = bi + t, p = rp + t;
                int gc = 4, x = 4;
                uint32_t q = 0;
                if (act) {
                    gc = gm_at(g, glen, p);
                    x = gm_code(R.seq[i]);
                    q = R.qual[i];
                }
                const bool both = act && gc < 4 && x < 4;       // what sub counts
                const bool mis = both && gc != x;
                n[1] += gm_pop(act);
                n[2] += gm_pop(both && !mis);
                n[3] += gm_pop(mis);
                n[4] += gm_pop(act && gc < 4 && x == 4);
                n[5] += gm_pop(act && gc == 4);
                gm_count(cnt + kGmSub, j * 16 + (gc & 3) * 4 + (x & 3), both);
                gm_count(cnt + kGmQual, (int)q, both);
                gm_count(cnt + kGmQual + DCR_GMET_QUAL_BINS, (int)q, mis);
                if (both) {
                    const int g5 = gm_at(g, glen, p - 1), g3 = gm_at(g, glen, p + 1);
                    if (g5 < 4 && g3 < 4) gm_add(cnt + kGmTri + j * 256 + ((g5 * 4 + gc) * 4 + g3) * 4 + x);
                }
                // the cycle i' from the sequencing 5' end; a whole step at or past the last bin is one add
                const int64_t t_last = t0 + 63 < here - 1 ? t0 + 63 : here - 1;
                const int64_t ip_min = j == 0 ? bi + t0 : L - 1 - (bi + t_last);
                if (ip_min >= last_bin) {
                    gm_wave_add(cyc + last_bin, both);
                    gm_wave_add(cyc + DCR_GMET_CYC_BINS + last_bin, mis);
                } else if (both) {
                    const int64_t ip = j == 0 ? i : L - 1 - i;
                    const int b = ip < last_bin ? (int)ip : last_bin;
                    gm_add(cyc + b);
                    if (mis) gm_add(cyc + DCR_GMET_CYC_BINS + b);
                }
            }
            rp += run;
            bi += run;
        } else if (op == 1u) {
            n[6] += gm_once(1);
            n[7] += gm_once((unsigned long long)here);
            bi += run;
        } else if (op == 4u) {
            bi += run;
        } else if (op == 2u) {
            n[8] += gm_once(1);
            n[9] += gm_once((unsigned long long)run);
            rp += run;
        } else if (op == 3u) {
            rp += run;
        }                       // H, P and the unused codes: neither
    }
}

#endif  // DCR_GENOME_BODY_H
