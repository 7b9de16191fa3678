/* oracle/ref_harness_ssw.c -- TEST INFRASTRUCTURE (fixture generator), our own source, linked against the
 * reference's ssw.c where it lies (oracle/Makefile target _ref/sswharness).  Prints known answers of
 *   ssw_init(read, L, mat, n, 1) + ssw_align(prof, ref, refLen, 3, 1, 2, 0, 20, L/2)     (Align_src/ssw.c:741-856)
 * exactly as snpaln_sw_snpaware / snpaln_sw call it (alnpe.c:261-393), for seeded random windows.
 * Line format:  S <aware 0|1> <ref symbols as hex digits> <read codes as digits 0-4>
 *                 <score1> <score2> <ref_begin1> <ref_end1> <read_begin1> <read_end1> <cigar text|->
 * aware=1: ref symbols are 4-bit allele masks and the read is encoded 1<<code with the 16x16 matrix score_mat2;
 * aware=0: ref symbols are 0..3 and the read 0..4 with the 5x5 matrix score_mat (both matrices: alnpe.c:52-73).
 *
 *   sswharness [N]               N short windows (default 600): tests/golden/ssw_vectors.txt
 *   sswharness --shapes N SEED   N windows shaped after the GPU kernels' code paths: reads of 16-512 bases (the stripe-variant
 *                                edges among them), windows up to ~3000 columns, indel runs up to 60 bases, band doubling, copies of
 *                                the target around the second-best mask, low-complexity windows, N runs, zero-mask runs, junk
 *                                reads and CIGARs of more than 64 operations: tests/golden/ssw_vectors_shapes.txt.gz */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "ssw.h"

#define MAX_L 512                         /* SALT_MAX_READ_LEN */
#define MAX_WIN 3200

static const int8_t score_mat[25] = { 1, -3, -3, -3, -1,  -3, 1, -3, -3, -1,  -3, -3, 1, -3, -1,  -3, -3, -3, 1, -1,  -1, -1, -1, -1, -1 };
static int8_t score_mat2[256 + 32];
static uint64_t st = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(void) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (uint32_t)(st >> 11); }

/* one known answer: ssw_align on ref[0..refLen) (symbols as the matrix wants them) and the read codes, printed as one line */
static void emit(int aware, const int8_t *ref, int refLen, const uint8_t *code, int L)
{
    int8_t *read = calloc(L + 8, 1);
    int i;
    for (i = 0; i < L; ++i) read[i] = aware ? (int8_t)(1 << code[i]) : (int8_t)code[i];
    s_profile *pr = ssw_init(read, L, aware ? score_mat2 : score_mat, aware ? 16 : 5, 1);
    s_align *a = ssw_align(pr, ref, refLen, 3, 1, 2, 0, 20, L / 2);
    printf("S %d ", aware);
    for (i = 0; i < refLen; ++i) printf("%x", ref[i] & 15);
    printf(" ");
    for (i = 0; i < L; ++i) printf("%d", code[i]);
    printf(" %d %d %d %d %d %d ", a->score1, a->score2, a->ref_begin1, a->ref_end1, a->read_begin1, a->read_end1);
    if (a->cigarLen == 0) printf("-");
    for (i = 0; i < a->cigarLen; ++i) printf("%u%c", a->cigar[i] >> 4, "MID"[a->cigar[i] & 15]);
    printf("\n");
    align_destroy(a); init_destroy(pr); free(read);
}

/* the window symbols of base[]: the bases themselves, or allele masks with a second allele now and then (aware) */
static void to_syms(int aware, const uint8_t *base, int8_t *ref, int refLen)
{
    int i;
    for (i = 0; i < refLen; ++i) {
        if (aware) { int m = 1 << base[i]; if (rnd() % 100 < 6) m |= 1 << (rnd() & 3); if (rnd() % 200 == 0) m = 0; ref[i] = (int8_t)m; }
        else ref[i] = (int8_t)base[i];
    }
}

static void short_vectors(int n_cases)
{
    int t;
    for (t = 0; t < n_cases; ++t) {
        int aware = t & 1, L = (t % 5 == 0) ? 40 + rnd() % 110 : 100, refLen = 120 + rnd() % 600, i;
        int8_t *ref = calloc(refLen + 8, 1);
        uint8_t *base = calloc(refLen, 1);
        for (i = 0; i < refLen; ++i) {
            base[i] = rnd() & 3;
            if (aware) { int m = 1 << base[i]; if (rnd() % 100 < 6) m |= 1 << (rnd() & 3); if (rnd() % 200 == 0) m = 0; ref[i] = m; }
            else ref[i] = base[i];
        }
        int kind = rnd() % 10, p = rnd() % (refLen - L > 1 ? refLen - L : 1);
        uint8_t code[MAX_L];
        if (refLen < L + 2) p = 0;
        for (i = 0; i < L; ++i) code[i] = (p + i < refLen) ? base[p + i] : (rnd() & 3);
        if (kind == 0) for (i = 0; i < L; ++i) code[i] = rnd() & 3;                      /* junk read */
        else {
            int ne = rnd() % 6, e;
            for (e = 0; e < ne; ++e) code[rnd() % L] = rnd() & 3;
            if (kind < 5) {                                                                 /* an indel */
                int q = 10 + rnd() % (L - 20), k = 1 + rnd() % 3;
                if (rnd() & 1) memmove(code + q, code + q + k, L - q - k);
                else { memmove(code + q + k, code + q, L - q - k); for (e = 0; e < k; ++e) code[q + e] = rnd() & 3; }
            }
            if (kind == 5) for (i = 0; i < 12; ++i) code[i] = rnd() & 3;                   /* clipped head */
            if (kind == 6) for (i = L - 15; i < L; ++i) code[i] = rnd() & 3;               /* clipped tail */
            if (rnd() % 10 == 0) code[rnd() % L] = 4;                                      /* N */
        }
        emit(aware, ref, refLen, code, L);
        free(ref); free(base);
    }
}

/* ---- --shapes ---------------------------------------------------------------------------------------------------------- */
/* an edit of the read against its source: at read position `at`, `len` inserted random bases (ins) or `len` skipped source bases */
typedef struct { int at, len, ins; } edit_t;

static int cmp_edit(const void *a, const void *b) { return ((const edit_t *)a)->at - ((const edit_t *)b)->at; }

/* the read: base[p..] with the edits applied (sorted by position); source bases past the window are random */
static void build_read(const uint8_t *base, int refLen, int p, int L, edit_t *ev, int nev, uint8_t *code)
{
    int i = 0, r = p, e = 0, k;
    qsort(ev, nev, sizeof *ev, cmp_edit);
    while (i < L) {
        if (e < nev && ev[e].at <= i) {
            if (ev[e].ins) for (k = 0; k < ev[e].len && i < L; ++k) code[i++] = rnd() & 3;
            else r += ev[e].len;
            ++e;
            continue;
        }
        code[i++] = (r >= 0 && r < refLen) ? base[r] : (rnd() & 3);
        ++r;
    }
}

/* the source span a read of L bases with these edits covers */
static int span_of(int L, const edit_t *ev, int nev)
{
    int s = L, e;
    for (e = 0; e < nev; ++e) s += ev[e].ins ? -ev[e].len : ev[e].len;
    return s > 1 ? s : 1;
}

static const int EDGE_L[] = { 104, 105, 152, 153, 256, 257, 512, 104, 152, 256 };

/* read lengths: the stripe-variant edges (13 / 19 / 32 stripes of 8, 512), 16-31 (maskLen on both sides of 15), the rest uniform */
static int pick_len(int lo)
{
    int L, c = rnd() % 100;
    if (c < 35) L = EDGE_L[rnd() % (sizeof EDGE_L / sizeof EDGE_L[0])];
    else if (c < 50) L = 16 + rnd() % 16;
    else L = 32 + rnd() % (MAX_L - 31);
    return L < lo ? lo + rnd() % (MAX_L - lo + 1) : L;
}

/* window length around a source span: mostly a few hundred columns more, now and then up to ~3000, now and then shorter than the read */
static int pick_win(int span, int L)
{
    int c = rnd() % 100, w;
    if (c < 8) w = L / 3 + 1 + rnd() % (L - L / 3);
    else if (c < 30) w = span + rnd() % (MAX_WIN - 200 - span > 1 ? MAX_WIN - 200 - span : 1);
    else w = span + rnd() % 400;
    return w < 1 ? 1 : w > MAX_WIN ? MAX_WIN : w;
}

enum { K_PLAIN, K_INDEL, K_DOUBLE, K_WIDE, K_TANDEM, K_LOWCX, K_NRUN, K_JUNK, K_CIGAR };
static const int KINDS[20] = { K_PLAIN, K_PLAIN, K_PLAIN, K_PLAIN, K_INDEL, K_INDEL, K_INDEL, K_DOUBLE, K_DOUBLE, K_WIDE,
                               K_WIDE, K_TANDEM, K_TANDEM, K_TANDEM, K_LOWCX, K_LOWCX, K_NRUN, K_NRUN, K_JUNK, K_PLAIN };

static void shape_vector(int t)
{
    static uint8_t base[MAX_WIN + 8], code[MAX_L];
    static int8_t ref[MAX_WIN + 8];
    edit_t ev[80];
    int aware = t & 1, kind = (t % 80 == 7) ? K_CIGAR : KINDS[t % 20], nev = 0, L, span, refLen, p, i, e;
    int sub_rate = 0, clip = 0;                                /* substitutions per 1000 read bases; a clipped head or tail */
    switch (kind) {
    case K_INDEL: {                                            /* one to four indel runs of 1-60 bases, at least 12 bases apart */
        L = pick_len(60);
        int n = 1 + rnd() % 4, at = 6 + rnd() % 20;
        for (e = 0; e < n && at < L - 6; ++e) {
            int lim = L / 4 < 60 ? L / 4 : 60, len = 1 + (rnd() % 3 ? rnd() % (lim < 12 ? lim : 12) : rnd() % lim);
            ev[nev].at = at; ev[nev].len = len; ev[nev].ins = rnd() & 1; ++nev;
            at += 12 + (ev[nev - 1].ins ? len : 0) + rnd() % (L / 2 > 1 ? L / 2 : 1);
        }
        sub_rate = rnd() % 20;
        break; }
    case K_DOUBLE: {                                           /* an insertion and a deletion of the same length far apart: the band starts at 1 */
        L = pick_len(80);
        int k = 2 + rnd() % (L / 8 < 40 ? L / 8 : 40), a1 = L / 8 + rnd() % (L / 4), a2 = L / 2 + k + rnd() % (L / 4);
        int first_ins = rnd() & 1;
        ev[0].at = a1; ev[0].len = k; ev[0].ins = first_ins; ev[1].at = a2; ev[1].len = k; ev[1].ins = !first_ins; nev = 2;
        sub_rate = rnd() % 10;
        break; }
    case K_WIDE: {                                             /* a short aligned core with a 14-40 base deletion in a longer read of junk */
        int k = 14 + rnd() % 27, c = 2 * k + 8 + rnd() % 40;
        L = pick_len(c + 4);
        ev[0].at = c / 2; ev[0].len = k; ev[0].ins = 0; nev = 1;
        sub_rate = rnd() % 8;
        span = span_of(c, ev, nev);
        refLen = pick_win(span + 2 * L, L); if (refLen < span + 2) refLen = span + 2;
        for (i = 0; i < refLen; ++i) base[i] = rnd() & 3;
        p = rnd() % (refLen - span + 1);
        build_read(base, refLen, p, c, ev, nev, code);
        {                                                      /* the core somewhere in the read, junk around it */
            int off = rnd() % (L - c + 1);
            memmove(code + off, code, c);
            for (i = 0; i < off; ++i) code[i] = rnd() & 3;
            for (i = off + c; i < L; ++i) code[i] = rnd() & 3;
        }
        goto finish; }
    case K_TANDEM: {                                           /* copies of the target around the second-best mask (maskLen = L/2) */
        L = pick_len(32);
        int mask = L / 2, d = mask - 2 + (int)(rnd() % 5), sub = rnd() % 4;
        if (sub == 0) {                                        /* the read's last d bases again right after the source: their end at end1 + d */
            span = L; refLen = pick_win(span + d, L); if (refLen < span + d + 1) refLen = span + d + 1;
            for (i = 0; i < refLen; ++i) base[i] = rnd() & 3;
            p = rnd() % (refLen - span - d + 1);
            for (i = 0; i < d; ++i) base[p + L + i] = base[p + L - d + i];
        } else if (sub == 1) {                                 /* a read of period d over d + L source bases: two full copies d apart, or one
                                                                  of them one base worse */
            span = L + d; refLen = pick_win(span, L); if (refLen < span + 1) refLen = span + 1;
            for (i = 0; i < refLen; ++i) base[i] = rnd() & 3;
            p = rnd() % (refLen - span + 1);
            for (i = d; i < span; ++i) base[p + i] = base[p + i - d];
            if (rnd() % 3) { int q = rnd() & 1 ? p + d / 2 : p + L + d / 2; base[q] = (base[q] + 1 + rnd() % 3) & 3; }
            if (rnd() & 1) p += d;                             /* the read from the later copy's phase: same bases */
        } else {                                               /* an exact second copy (score1 == score2) somewhere else in the window */
            span = L; refLen = pick_win(3 * L, L); if (refLen < 2 * L + 1) refLen = 2 * L + 1;
            for (i = 0; i < refLen; ++i) base[i] = rnd() & 3;
            p = rnd() % (refLen - 2 * L + 1);
            int q = rnd() % (refLen - L + 1);
            if (q + L > p && q < p + L) q = p + L + rnd() % (refLen - p - 2 * L + 1);
            memcpy(base + q, base + p, L);
        }
        build_read(base, refLen, p, L, ev, 0, code);
        if (sub == 3) for (e = 0; e < 3; ++e) code[rnd() % L] = rnd() & 3;
        goto finish; }
    case K_LOWCX: {                                            /* a window of period 1-6 around the source, indels inside it */
        L = pick_len(24);
        int per = 1 + rnd() % 6, n = rnd() % 4, at = 4 + rnd() % 10;
        uint8_t unit[6];
        for (i = 0; i < per; ++i) unit[i] = rnd() & 3;
        for (e = 0; e < n && at < L - 4; ++e) {
            ev[nev].at = at; ev[nev].len = 1 + rnd() % 10; ev[nev].ins = rnd() & 1; ++nev;
            at += 8 + rnd() % (L / 2 > 1 ? L / 2 : 1);
        }
        span = span_of(L, ev, nev);
        refLen = pick_win(span, L);
        for (i = 0; i < refLen; ++i) base[i] = rnd() & 3;
        p = refLen > span ? rnd() % (refLen - span + 1) : 0;
        {
            int a = p - (int)(rnd() % 40), b = p + span + (int)(rnd() % 40);
            for (i = a > 0 ? a : 0; i < b && i < refLen; ++i) base[i] = unit[i % per];
            if (rnd() & 1) for (e = 0; e < 3; ++e) { int q = a + (int)(rnd() % (b - a)); if (q >= 0 && q < refLen) base[q] = rnd() & 3; }
        }
        build_read(base, refLen, p, L, ev, nev, code);
        goto finish; }
    case K_JUNK:
        L = pick_len(16);
        refLen = pick_win(L, L);
        for (i = 0; i < refLen; ++i) base[i] = rnd() & 3;
        for (i = 0; i < L; ++i) code[i] = rnd() & 3;
        goto finish;
    case K_CIGAR: {                                            /* a 1-base indel every few bases: more operations than SALT_MAX_CIGAR_OPS */
        L = 200 + rnd() % (MAX_L - 199);
        int step = 5 + rnd() % 6, ins = rnd() % 3;
        for (i = step; i < L - 2 && nev < 80; i += step) { ev[nev].at = i; ev[nev].len = 1; ev[nev].ins = ins == 2 ? (nev & 1) : ins; ++nev; }
        break; }
    case K_NRUN:
    case K_PLAIN:
    default:
        L = pick_len(16);
        if (rnd() % 3 == 0 && L >= 30) { ev[0].at = 10 + rnd() % (L - 20); ev[0].len = 1 + rnd() % 3; ev[0].ins = rnd() & 1; nev = 1; }
        sub_rate = rnd() % 30;
        if (kind == K_PLAIN && rnd() % 4 == 0) clip = 1;   /* clipped head or tail */
        break;
    }
    span = span_of(L, ev, nev);
    refLen = pick_win(span, L);
    for (i = 0; i < refLen; ++i) base[i] = rnd() & 3;
    p = refLen > span ? rnd() % (refLen - span + 1) : (int)(rnd() % (refLen + 1)) - (int)(rnd() % (L / 2 + 1));
    build_read(base, refLen, p, L, ev, nev, code);
    for (i = 0; i < L; ++i) if (rnd() % 1000 < (uint32_t)sub_rate) code[i] = rnd() & 3;
    if (clip) {
        int k = 5 + rnd() % (L / 3 + 1);
        if (rnd() & 1) for (i = 0; i < k && i < L; ++i) code[i] = rnd() & 3;
        else for (i = L - k > 0 ? L - k : 0; i < L; ++i) code[i] = rnd() & 3;
    }
finish:
    if (kind == K_NRUN) {                                      /* runs of N in the read */
        int n = 1 + rnd() % 3;
        for (e = 0; e < n; ++e) { int a = rnd() % L, k = 1 + rnd() % 20; for (i = a; i < a + k && i < L; ++i) code[i] = 4; }
    } else if (rnd() % 10 == 0) code[rnd() % L] = 4;
    to_syms(aware, base, ref, refLen);
    if (aware && (kind == K_NRUN || rnd() % 8 == 0)) {         /* runs of zero masks (no allele) in SNP-aware windows */
        int n = 1 + rnd() % 3;
        for (e = 0; e < n; ++e) { int a = rnd() % refLen, k = 1 + rnd() % 30; for (i = a; i < a + k && i < refLen; ++i) ref[i] = 0; }
    }
    emit(aware, ref, refLen, code, L);
}

int main(int argc, char **argv)
{
    int r, c, t;
    for (r = 0; r < 16; ++r) for (c = 0; c < 16; ++c) {
        int v = -3;
        if (r == 1 && (c & 1)) v = 1;
        if (r == 2 && (c & 2)) v = 1;
        if (r == 4 && (c & 4)) v = 1;
        if (r == 8 && (c & 8)) v = 1;
        score_mat2[r * 16 + c] = v;
    }
    for (c = 0; c < 32; ++c) score_mat2[256 + c] = -3;
    if (argc > 1 && !strcmp(argv[1], "--shapes")) {
        int n = argc > 2 ? atoi(argv[2]) : 1000;
        uint64_t seed = argc > 3 ? strtoull(argv[3], NULL, 10) : 1;
        st ^= seed * 0x9E3779B97F4A7C15ull;
        if (!st) st = 1;
        for (t = 0; t < n; ++t) shape_vector(t);
        return 0;
    }
    short_vectors(argc > 1 ? atoi(argv[1]) : 600);
    return 0;
}
