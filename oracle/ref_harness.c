/* oracle/ref_harness.c -- TEST INFRASTRUCTURE (fixture generator), our own source.
 *
 * Links against the reference's LandauVishkin.c + editdistance.c where they lie (see
 * oracle/Makefile target _ref/lvharness) and prints known-answer vectors for
 *   ed_mismatch            (Align_src/editdistance.c:88)
 *   ed_diff                (Align_src/editdistance.c:174)  -> computeEditDistance (LandauVishkin.c:19)
 *   ed_diff_withcigar      (Align_src/editdistance.c:234)  -> computeEditDistanceWithCigar (:176)
 * on a seeded synthetic 4-bit "mixRef".  Output format (text, one record per line):
 *   R <l> <hex words...>                      the mixRef (l bases, 8 per u32, LSB-first nibbles)
 *   V <pos> <L> <kmis> <kdiff> <read codes 0-4 as digits> <mis> <diff> <cigar_ret> <cigar|->
 * where mis = ed_mismatch(ref,pos,seq,L,kmis), diff = ed_diff(ref,l,pos,L+4,seq,L,kdiff) and
 * cigar_ret/cigar = ed_diff_withcigar(ref,pos,L+4,seq,L,diff,buf,128,1,COMPACT) when diff >= 0.
 *
 *   lvharness [N]               N vectors, most of them 100 bases long: tests/golden/lv_vectors.txt
 *   lvharness --shapes N SEED   N vectors shaped after the routes of the GPU's gapped pass (same line format, CIGAR buffer of 400):
 *                               lengths on both sides of every length at which the aligner changes route, bounds {L/10, 3, 12, 13, 30},
 *                               indel runs of 1..30 bases at both sides of the 8-base words of the packed windows, windows that
 *                               end at the reference's end -2 .. +1 or start at 0, reads with N, reference sites without any
 *                               allele.  The first 64 * N_GROUPED vectors come 64 to one (L, k), so that a kernel that takes one
 *                               candidate per lane can be given 64 different ones: tests/golden/lv_vectors_shapes.txt.gz
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "editdistance.h"

static uint64_t s_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    s_state ^= s_state << 13; s_state ^= s_state >> 7; s_state ^= s_state << 17;
    return (uint32_t)(s_state >> 11);
}
static uint32_t rndn(uint32_t n) { return rnd() % n; }

#define REFLEN 6000

/* ---- --shapes -------------------------------------------------------------------------------------------------------- */
static const int shape_len[] = { 40, 99, 100, 101, 119, 120, 128, 129, 130, 131, 139, 140, 160, 164, 165, 168, 170, 200, 300, 512,
                                 19, 36, 161, 235, 400 };
#define N_SHAPE_LEN ((int)(sizeof shape_len / sizeof shape_len[0]))
/* (L, k) of the groups of 64: every one within the lane kernel's limits (k <= 12, L + 4 <= 168); k = 0 stands for L / 10 */
static const int grouped[][2] = {
    { 19, 0 }, { 40, 0 }, { 99, 0 }, { 100, 0 }, { 101, 0 }, { 119, 0 }, { 120, 0 }, { 128, 0 }, { 129, 0 },
    { 100, 3 }, { 129, 3 }, { 130, 3 }, { 160, 3 }, { 161, 3 }, { 164, 3 },
    { 36, 12 }, { 40, 12 }, { 101, 12 }, { 130, 12 }, { 131, 12 }, { 139, 12 }, { 140, 12 }, { 160, 12 }, { 161, 12 }, { 164, 12 },
};
#define N_GROUPED ((int)(sizeof grouped / sizeof grouped[0]))

static int shape_pos(int L, int which)
{
    const int p[13] = { 0, 1, 2, 3, 7, 8, 9, L / 2, L - 9, L - 8, L - 3, L - 2, L - 1 };
    return p[which % 13] < 0 ? 0 : p[which % 13];
}

static void shapes(int n_cases, const uint32_t *ref, const uint8_t *base, uint32_t l)
{
    int t;
    for (t = 0; t < n_cases; ++t) {
        int L, kdiff;
        if (t < 64 * N_GROUPED) { L = grouped[t / 64][0]; kdiff = grouped[t / 64][1] ? grouped[t / 64][1] : L / 10; }
        else {
            const int ks[5] = { 0, 3, 12, 13, 30 };
            L = shape_len[rndn(N_SHAPE_LEN)];
            kdiff = ks[rndn(5)]; if (!kdiff) kdiff = L / 10;
        }
        /* the window's start: mostly anywhere, else its end L + 4 at the reference's end -2, -1, +0 (inside) or +1 (outside), or 0 */
        uint32_t pos, r = rndn(100);
        if (r < 12) pos = l - L - 4 - rndn(3);
        else if (r < 15) pos = l - L - 4 + 1;
        else if (r < 20) pos = 0;
        else pos = rndn(l - L - 64);
        /* the source: the reference from pos (a few bases in, now and then), any listed allele at a site, random past the end */
        uint8_t tmp[700], seq[520]; int n = 0, e; uint32_t p = pos, i;
        if (rndn(100) < 10) p += rndn(4);
        while (n < L + 80 && p < l) {
            uint32_t m = (ref[p >> 3] >> (4 * (p & 7))) & 15;
            uint8_t c = base[p];
            if (m && rndn(2)) {
                int tries = 0; uint32_t a;
                do { a = rndn(4); } while (!((m >> a) & 1) && ++tries < 32);
                if ((m >> a) & 1) c = (uint8_t)a;
            }
            tmp[n++] = c; ++p;
        }
        while (n < L + 80) tmp[n++] = (uint8_t)rndn(4);
        /* edits: none (1 in 8), one indel run, or a run and its opposite 20 bases on; runs of 1..3 (half) or 1..30 bases */
        int kind = (int)rndn(8), n_runs = kind == 0 ? 0 : (kind < 6 ? 1 : 2);
        int run = rndn(2) ? 1 + (int)rndn(3) : 1 + (int)rndn(30), q = shape_pos(L, (int)rndn(13)), ins = (int)rndn(2);
        if (run > L - 1) run = L - 1;
        for (e = 0; e < n_runs; ++e) {
            if (e == 1) { ins = !ins; q = q + 20 + run < L ? q + 20 : (q >= 20 ? q - 20 : q); }
            if (ins) { memmove(tmp + q + run, tmp + q, n - q - run); for (i = 0; i < (uint32_t)run; ++i) tmp[q + i] = (uint8_t)rndn(4); }
            else memmove(tmp + q, tmp + q + run, n - q - run);
        }
        int nsub = (int)rndn(4);
        for (e = 0; e < nsub; ++e) { int s = (int)rndn(L); tmp[s] = (uint8_t)((tmp[s] + 1 + rndn(3)) & 3); }
        memcpy(seq, tmp, L);
        if (rndn(100) < 15) seq[rndn(L)] = 4;                                    /* read N */
        if (rndn(100) < 3) { int s = (int)rndn(L - 5); for (e = 0; e < 5; ++e) seq[s + e] = 4; }
        int kmis = (int)rndn(4), mis = -9;
        if (pos + L <= l) mis = ed_mismatch(ref, pos, seq, L, kmis);
        int diff = ed_diff(ref, l, pos, L + 4, seq, L, kdiff);
        char cig[512]; memset(cig, 0, sizeof cig);
        int cret = -9;
        if (diff >= 0 && diff < 31)
            cret = ed_diff_withcigar(ref, pos, L + 4, seq, L, diff, cig, 400, 1, COMPACT_CIGAR_STRING);
        printf("V %u %d %d %d ", pos, L, kmis, kdiff);
        for (i = 0; i < (uint32_t)L; ++i) putchar('0' + seq[i]);
        printf(" %d %d %d %s\n", mis, diff, cret, cig[0] ? cig : "-");
    }
}

int main(int argc, char **argv)
{
    int shape_mode = argc > 3 && !strcmp(argv[1], "--shapes");
    if (shape_mode) { s_state ^= 0xD1B54A32D192ED03ull * (uint64_t)(atoi(argv[3]) + 1); if (!s_state) s_state = 1; argv += 1; }
    int n_cases = argc > 1 ? atoi(argv[1]) : 3000;
    uint32_t l = REFLEN;
    uint32_t nw = (l + 7) / 8;
    uint32_t *ref = calloc(nw + 4, 4);
    uint8_t *base = calloc(l, 1);
    uint32_t i;
    for (i = 0; i < l; ++i) {
        uint32_t c = rndn(4);
        uint32_t m = 1u << c;
        uint32_t r = rndn(100);
        if (r < 8) m |= 1u << rndn(4);           /* bi-allelic SNP site */
        else if (r < 10) m |= (1u << rndn(4)) | (1u << rndn(4));
        else if (r < 11) m = 0;                  /* reference N */
        base[i] = (uint8_t)c;
        ref[i >> 3] |= m << (4 * (i & 7));
    }
    printf("R %u", l);
    for (i = 0; i < nw; ++i) printf(" %08x", ref[i]);
    printf("\n");
    if (shape_mode) { shapes(n_cases, ref, base, l); return 0; }

    int t;
    for (t = 0; t < n_cases; ++t) {
        int L = (t % 7 == 0) ? 36 + (int)rndn(200) : 100;
        uint32_t pos;
        int mode = (int)rndn(10);
        if (mode == 0) pos = l - L - rndn(12);            /* at / over the end (LV window L+4) */
        else pos = rndn(l - L - 16);
        uint8_t *seq = calloc(L + 16, 1);
        /* derive the read from the reference with edits */
        int nsub = (int)rndn(100) < 50 ? (int)rndn(3) : (int)rndn(9);
        int nind = (int)rndn(100) < 55 ? 0 : 1 + (int)rndn(3);
        uint8_t tmp[600]; int n = 0; uint32_t p = pos;
        int shift = (int)rndn(100) < 15 ? (int)rndn(4) : 0; /* start a few bases in (leading D) */
        p += shift;
        while (n < L + 12 && p < l) {
            uint32_t m = (ref[p >> 3] >> (4 * (p & 7))) & 15;
            uint8_t c = base[p];
            if (m && rndn(2)) { /* pick any listed allele */
                int tries = 0; uint32_t a;
                do { a = rndn(4); } while (!((m >> a) & 1) && ++tries < 32);
                if ((m >> a) & 1) c = (uint8_t)a;
            }
            tmp[n++] = c; ++p;
        }
        while (n < L + 12) tmp[n++] = (uint8_t)rndn(4);
        int e;
        for (e = 0; e < nsub; ++e) { int q = (int)rndn(L); tmp[q] = (uint8_t)((tmp[q] + 1 + rndn(3)) & 3); }
        for (e = 0; e < nind; ++e) {
            int q = 2 + (int)rndn(L - 4);
            if (rndn(2)) { memmove(tmp + q, tmp + q + 1, n - q - 1); }
            else { memmove(tmp + q + 1, tmp + q, n - q - 1); tmp[q] = (uint8_t)rndn(4); }
        }
        memcpy(seq, tmp, L);
        if (rndn(100) < 6) seq[rndn(L)] = 4;           /* read N */
        int kmis = (int)rndn(4);
        int kdiff = (t % 5 == 0) ? (int)rndn(31) : L / 10;
        int mis = -9;
        if (pos + L <= l) mis = ed_mismatch(ref, pos, seq, L, kmis);
        int diff = ed_diff(ref, l, pos, L + 4, seq, L, kdiff);
        char cig[160]; memset(cig, 0, sizeof cig);
        int cret = -9;
        if (diff >= 0 && diff < 31)
            cret = ed_diff_withcigar(ref, pos, L + 4, seq, L, diff, cig, 128, 1, COMPACT_CIGAR_STRING);
        printf("V %u %d %d %d ", pos, L, kmis, kdiff);
        for (i = 0; i < (uint32_t)L; ++i) putchar('0' + seq[i]);
        printf(" %d %d %d %s\n", mis, diff, cret, cig[0] ? cig : "-");
        free(seq);
    }
    return 0;
}
