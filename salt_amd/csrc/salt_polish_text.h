// salt_amd/csrc/salt_polish_text.h -- the per-record rules of `polish` over SAM text, written once for the device kernels
// (salt_polish.hip) and for the host (tools/polish_text_model.cc runs the same source on the CPU, under the sanitizers).
//
// What is here: the reference's strtok field splitting (samParser.c:84-190), its XA items, the offset sort and rm_repeat_hits, the
// window rule (the length that shrinks for good at the genome end and the stale bytes behind a clipped Landau-Vishkin window,
// polish.c:84-92, 466), the winners and the pairing walk (polish.c:155-188, 600-640, 718-737) and the record printer
// (polish_sam_se / polish_sam_pe, polish.c:251-445).  salt_amd/host/polish_main.cc states the same rules a second time over
// std::string and std::vector; the tests hold the two against each other and against the real program's output.
//
// Every function reads only [b, e) of the text it is given and only the spans it is handed: damaged input changes results, never
// addresses.
#ifndef SALT_POLISH_TEXT_H
#define SALT_POLISH_TEXT_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PL_HD __host__ __device__ inline
#else
#define PL_HD inline
#endif

namespace salt_pl {

static const int32_t PL_UNMAPPED = -100000, PL_MAX_DISTANCE = 13;           // polish.c:447, 150
static const uint32_t PL_MIN_ISIZE = 350, PL_MAX_ISIZE = 650;               // polish.c:148-149
static const uint32_t PL_MAX_READ = 512;                                    // SALT_MAX_READ_LEN
static const uint32_t PL_POOL_STRIDE = 512;                                 // bytes of one explicit window (>= any read)
static const uint32_t PL_MAX_CIGAR = 64;                                    // SALT_MAX_CIGAR_OPS

// status of a record (the smallest record index with a non-zero status is the one reported)
enum { PL_OK = 0, PL_E_FIELDS = 1, PL_E_CONTIG = 2, PL_E_LEN = 3, PL_E_RANGE = 4, PL_E_BAND = 5, PL_E_NOALN = 6, PL_E_CIGAR = 7, PL_E_WINDOW = 8 };

struct PlHit { uint32_t offset, pos, contig; int32_t score; };             // contig: index into the sorted table
// contig table sorted by name: name i = names[name_off[i] .. name_off[i + 1])
struct PlContigs { const int64_t *off; const uint32_t *name_off; const uint8_t *names; int32_t n; };
struct PlFields {
    uint32_t name_off, name_len, chrom_off, chrom_len, seq_off, l_seq, qual_off, qual_len, xa_off, xa_end;     // xa_off == xa_end: no XA field
    int32_t flag; uint32_t pos, has_primary;
};

// strtok(s, delim): skips leading delimiters, so empty fields vanish; false at the end of the text
PL_HD bool pl_tok(const uint8_t *s, uint32_t &p, uint32_t e, uint8_t delim, uint32_t &tb, uint32_t &te)
{
    while (p < e && s[p] == delim) ++p;
    if (p >= e) return false;
    tb = p;
    while (p < e && s[p] != delim) ++p;
    te = p;
    if (p < e) ++p;
    return true;
}
PL_HD bool pl_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
// strtoul(.., 10) cut to 32 bits: white space, one sign, digits; saturates at 2^64 - 1 as the C library does
PL_HD uint32_t pl_strtoul(const uint8_t *s, uint32_t b, uint32_t e)
{
    while (b < e && pl_space(s[b])) ++b;
    bool neg = false;
    if (b < e && (s[b] == '+' || s[b] == '-')) { neg = s[b] == '-'; ++b; }
    uint64_t v = 0; bool sat = false;
    for (; b < e && s[b] >= '0' && s[b] <= '9'; ++b) {
        const uint64_t d = (uint64_t)(s[b] - '0');
        if (v > (0xFFFFFFFFFFFFFFFFull - d) / 10) sat = true; else v = v * 10 + d;
    }
    if (sat) return 0xFFFFFFFFu;
    return (uint32_t)(neg ? (uint64_t)0 - v : v);
}
// atoi: the same through a signed long, cut to int
PL_HD int32_t pl_atoi(const uint8_t *s, uint32_t b, uint32_t e)
{
    while (b < e && pl_space(s[b])) ++b;
    bool neg = false;
    if (b < e && (s[b] == '+' || s[b] == '-')) { neg = s[b] == '-'; ++b; }
    uint64_t v = 0; bool sat = false;
    for (; b < e && s[b] >= '0' && s[b] <= '9'; ++b) {
        const uint64_t d = (uint64_t)(s[b] - '0');
        if (v > (0x7FFFFFFFFFFFFFFFull - d) / 10) sat = true; else v = v * 10 + d;
    }
    if (sat) return neg ? 0 : -1;                                // LONG_MIN / LONG_MAX cut to int
    return (int32_t)(uint32_t)(neg ? (uint64_t)0 - v : v);
}
PL_HD bool pl_has_xa(const uint8_t *s, uint32_t b, uint32_t e)
{
    for (uint32_t i = b; i + 1 < e; ++i) if (s[i] == 'X' && s[i + 1] == 'A') return true;
    return false;
}

// sam_readline (samParser.c:84-190) over the line s[b .. e) (no newline): false = fewer than 11 fields
PL_HD bool pl_parse(const uint8_t *s, uint32_t b, uint32_t e, PlFields &f)
{
    uint32_t p = b, tb = 0, te = 0;
    f.xa_off = f.xa_end = 0; f.has_primary = 0; f.l_seq = 0;
    if (!pl_tok(s, p, e, '\t', tb, te)) return false;
    f.name_off = tb; f.name_len = te - tb;
    if (!pl_tok(s, p, e, '\t', tb, te)) return false;
    f.flag = pl_atoi(s, tb, te);
    if (!pl_tok(s, p, e, '\t', tb, te)) return false;
    f.chrom_off = tb; f.chrom_len = te - tb;
    if (!pl_tok(s, p, e, '\t', tb, te)) return false;
    f.pos = pl_strtoul(s, tb, te);
    f.has_primary = (f.flag & 4) == 0 && !(f.chrom_len == 1 && s[f.chrom_off] == '*');
    for (int k = 0; k < 5; ++k) if (!pl_tok(s, p, e, '\t', tb, te)) return false;            // MAPQ CIGAR MRNM MPOS ISIZE
    if (!pl_tok(s, p, e, '\t', tb, te)) return false;
    f.seq_off = tb; f.l_seq = te - tb;
    if (!pl_tok(s, p, e, '\t', tb, te)) return false;
    f.qual_off = tb; f.qual_len = te - tb;
    while (pl_tok(s, p, e, '\t', tb, te))
        if (pl_has_xa(s, tb, te)) { f.xa_off = tb; f.xa_end = te; break; }                    // only the first field containing "XA" is read
    return true;
}

// the items of "XA:Z:chr,+pos,cigar,nd;..." as the reference's nested strtok sees them (samParser.c:143-186): the third ':' token,
// cut at ';', of each the first two ',' tokens
struct PlXa { uint32_t p, e; bool live; };
PL_HD PlXa pl_xa_begin(const uint8_t *s, const PlFields &f)
{
    PlXa x; x.p = x.e = 0; x.live = false;
    if (f.xa_off == f.xa_end) return x;
    uint32_t p = f.xa_off, tb = 0, te = 0;
    for (int k = 0; k < 3; ++k) if (!pl_tok(s, p, f.xa_end, ':', tb, te)) return x;
    x.p = tb; x.e = te; x.live = true;
    return x;
}
PL_HD bool pl_xa_next(const uint8_t *s, PlXa &x, uint32_t &chrom_b, uint32_t &chrom_e, uint32_t &strand, uint32_t &pos)
{
    if (!x.live || x.p >= x.e) return false;
    uint32_t semi = x.p;
    while (semi < x.e && s[semi] != ';') ++semi;
    if (semi == x.p) { x.live = false; return false; }
    uint32_t q = x.p, pb = 0, pe = 0;
    if (!pl_tok(s, q, semi, ',', chrom_b, chrom_e) || !pl_tok(s, q, semi, ',', pb, pe)) { x.live = false; return false; }
    if (s[pb] != '-') { strand = 0; pos = pl_strtoul(s, pb, pe); }
    else { strand = 1; pos = pl_strtoul(s, pb + 1, pe); }
    if (semi >= x.e) x.live = false; else x.p = semi + 1;
    return true;
}

// name -> index in the sorted table, -1 when it is not there
PL_HD int32_t pl_contig_find(const PlContigs &c, const uint8_t *s, uint32_t b, uint32_t e)
{
    int32_t lo = 0, hi = c.n - 1;
    const uint32_t n = e - b;
    while (lo <= hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        const uint32_t nb = c.name_off[mid], nl = c.name_off[mid + 1] - nb;
        int cmp = 0;
        for (uint32_t i = 0; i < n && i < nl && !cmp; ++i) cmp = (int)s[b + i] - (int)c.names[nb + i];
        if (!cmp) cmp = n < nl ? -1 : n > nl ? 1 : 0;
        if (!cmp) return mid;
        if (cmp < 0) hi = mid - 1; else lo = mid + 1;
    }
    return -1;
}

// hits per strand as parsed (primary first, then the XA items); `fill` false: counts only (h0 / h1 and the table are not touched).
// h0 / h1: the two strands' spans.
// false: a contig that is not in the table (bad_b / bad_e: its name)
PL_HD bool pl_hits(const uint8_t *s, const PlFields &f, const PlContigs &ct, bool fill, PlHit *h0, PlHit *h1, uint32_t nh[2], uint32_t &bad_b, uint32_t &bad_e)
{
    nh[0] = nh[1] = 0;
    PlHit *h[2] = { h0, h1 };
    if (f.has_primary) {
        const uint32_t st = (f.flag & 0x10) ? 1u : 0u;
        if (fill) {
            const int32_t c = pl_contig_find(ct, s, f.chrom_off, f.chrom_off + f.chrom_len);
            if (c < 0) { bad_b = f.chrom_off; bad_e = f.chrom_off + f.chrom_len; return false; }
            PlHit x; x.pos = f.pos; x.contig = (uint32_t)c; x.offset = (uint32_t)((uint64_t)ct.off[c] + f.pos - 1); x.score = 0;
            h[st][nh[st]] = x;
        }
        ++nh[st];
    }
    PlXa xa = pl_xa_begin(s, f);
    uint32_t cb = 0, ce = 0, st = 0, pos = 0;
    while (pl_xa_next(s, xa, cb, ce, st, pos)) {
        if (fill) {
            const int32_t c = pl_contig_find(ct, s, cb, ce);
            if (c < 0) { bad_b = cb; bad_e = ce; return false; }
            PlHit x; x.pos = pos; x.contig = (uint32_t)c; x.offset = (uint32_t)((uint64_t)ct.off[c] + pos - 1); x.score = 0;
            h[st][nh[st]] = x;
        }
        ++nh[st];
    }
    return true;
}

// ---- hits straight from a result row (salt --polish: no SAM line in between) ---------------------------------------------------
// bns_coor_pac2real's search (bntseq.c:269-289), the one the SAM writer names a position's contig by (seq_id_dev, salt_text.hip)
PL_HD int32_t pl_seq_id(const int64_t *c_off, int32_t n, int64_t coor)
{
    int32_t left = 0, mid = 0, right = n;
    while (left < right) {
        mid = (left + right) >> 1;
        if (coor >= c_off[mid]) {
            if (mid == n - 1) break;
            if (coor < c_off[mid + 1]) break;
            left = mid + 1;
        } else right = mid;
    }
    return mid;
}
static const uint32_t PL_ROW_HITS = 5 + 1;                                  // hits of one strand of a row at most: SALT_MAX_HITS and the primary
// The record-to-hits rule of the fused route: the hits pl_parse + pl_hits find in the line sam_head / sam_head_pe / sam_tags
// (salt_text.hip) write for row q, in the same order, without the line.  Row: salt_result_t (pos, strand, n_hits, hits).
//   primary   iff q.pos != 0xFFFFFFFF (single end: the line has flag 4 and RNAME "*" otherwise; paired end: flag 4, whatever RNAME
//             shows -- an unmapped mate is printed at its mate's place), on strand q.strand (paired end: 0x10 iff strand == 1)
//   XA items  hits[s][k], k < n_hits[s], strand 0 first, but those at the primary's position on either strand (sam_tags skips them);
//             a single-end unmapped read has no tags at all (sam.c:105-125), an unmapped mate of a pair has them
//   offset    the hit's position in the genome: the line says contig + (pos - c_off[contig] + 1) and pl_hits adds c_off[contig] - 1 back
//   contig    the index's own number of the contig the hit lies in (c_off / the names of the fused route's PlContigs are the index's table
//             as it stands: the tail only reads a hit's contig name and never searches the table, so no name-sorted copy is made)
// h0 / h1: PL_ROW_HITS entries each.
// pl_row_rev: bit 0x10 of the line's FLAG.  The printer needs it although QUAL is as sequenced on this route: polish_sam_se / _pe put a tab
// behind QUAL exactly when they print it the way the line had it (polish.c:289,292), and the line had it reversed under 0x10.
template <class Row> PL_HD bool pl_row_rev(const Row &q, bool paired) { return paired ? q.strand == 1 : (q.pos != 0xFFFFFFFFu && q.strand != 0); }
template <class Row>
PL_HD void pl_row_hits(const Row &q, bool paired, const int64_t *c_off, int32_t n_contigs, PlHit *h0, PlHit *h1, uint32_t nh[2])
{
    nh[0] = nh[1] = 0;
    PlHit *h[2] = { h0, h1 };
    const uint32_t primary = q.pos;
    const bool mapped = primary != 0xFFFFFFFFu;
    if (!mapped && !paired) return;
    for (int s = -1; s < 2; ++s) {
        const uint32_t n = s < 0 ? (mapped ? 1u : 0u) : (q.n_hits[s] < PL_ROW_HITS - 1 ? q.n_hits[s] : PL_ROW_HITS - 1);
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t at = s < 0 ? primary : q.hits[s][k].pos;
            if (s >= 0 && at == primary) continue;
            const uint32_t st = s >= 0 ? (uint32_t)s : (pl_row_rev(q, paired) ? 1u : 0u);
            const int32_t c = pl_seq_id(c_off, n_contigs, (int64_t)at);
            PlHit x; x.offset = at; x.pos = (uint32_t)((int64_t)at - c_off[c] + 1); x.contig = (uint32_t)c; x.score = 0;
            h[st][nh[st]++] = x;
        }
    }
}

// sort by offset (equal offsets are equal hits under one table: the order among them does not matter), then rm_repeat_hits
PL_HD void pl_sift(PlHit *h, uint32_t i, uint32_t n)
{
    const PlHit x = h[i];
    for (;;) {
        uint32_t c = 2 * i + 1;
        if (c >= n) break;
        if (c + 1 < n && h[c + 1].offset > h[c].offset) ++c;
        if (h[c].offset <= x.offset) break;
        h[i] = h[c]; i = c;
    }
    h[i] = x;
}
PL_HD uint32_t pl_sort_unique(PlHit *h, uint32_t n)
{
    if (n < 2) return n;
    if (n <= 16) {
        for (uint32_t i = 1; i < n; ++i) { const PlHit x = h[i]; uint32_t j = i; while (j > 0 && h[j - 1].offset > x.offset) { h[j] = h[j - 1]; --j; } h[j] = x; }
    } else {
        for (uint32_t i = n / 2; i-- > 0;) pl_sift(h, i, n);
        for (uint32_t m = n - 1; m > 0; --m) { const PlHit t = h[0]; h[0] = h[m]; h[m] = t; pl_sift(h, 0, m); }
    }
    uint32_t k = 1;
    for (uint32_t i = 1; i < n; ++i) if (h[i].offset != h[k - 1].offset) h[k++] = h[i];
    return k;
}

PL_HD uint8_t pl_code(uint8_t c) { switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; } }
// the read as sequenced: SEQ of a reverse-strand record is its reverse complement (samParser.c:131-141)
PL_HD void pl_codes(const uint8_t *s, const PlFields &f, uint8_t *d)
{
    const uint32_t L = f.l_seq;
    if (f.flag & 0x10) for (uint32_t j = 0; j < L; ++j) { const uint8_t c = pl_code(s[f.seq_off + L - 1 - j]); d[j] = c < 4 ? (uint8_t)(3 - c) : c; }
    else for (uint32_t j = 0; j < L; ++j) d[j] = pl_code(s[f.seq_off + j]);
}
PL_HD uint8_t pl_base(const uint8_t *pac, uint64_t l) { return (uint8_t)((pac[l >> 2] >> ((~l & 3) << 1)) & 3); }

// The window rule over the record's unique hits in order (forward strand first).  Pass 1 (item == null): checks and counts;
// pass 2: one item per hit into item[0 ..), clipped Landau-Vishkin windows into pool[pool_base ..).  n_clip: hits whose window is
// shorter than the read; those are the pool windows unless use_sw.  Returns PL_OK, PL_E_RANGE or PL_E_WINDOW.
template <class Item>
PL_HD int pl_windows(uint32_t read, uint32_t l_seq, uint64_t l_pac, bool use_sw, const PlHit *h0, uint32_t nu0, const PlHit *h1, uint32_t nu1,
                     const uint8_t *pac, Item *item, uint8_t *pool, uint32_t pool_base, uint32_t &n_clip)
{
    uint32_t l_ref = l_seq, prev_full = 0xFFFFFFFFu, k = 0;          // l_ref shrinks for good once a window is clipped (polish.c:466)
    n_clip = 0;
    for (uint32_t s = 0; s < 2; ++s) {
        const PlHit *h = s ? h1 : h0; const uint32_t nu = s ? nu1 : nu0;
        for (uint32_t j = 0; j < nu; ++j, ++k) {
            const uint32_t off = h[j].offset;
            if ((uint64_t)off > l_pac) return PL_E_RANGE;
            if ((uint64_t)off + l_ref > l_pac) l_ref = (uint32_t)(l_pac - off);
            if (use_sw && l_ref == 0) return PL_E_WINDOW;
            uint32_t pl = 0xFFFFFFFFu;
            if (l_ref < l_seq) {
                if (!use_sw) {
                    pl = pool_base + n_clip;
                    if (item) {
                        // the reference's buffer, written in place (polish.c:84-92): what the last window left, fresh bases up to the clip
                        uint8_t *w = pool + (uint64_t)pl * PL_POOL_STRIDE;
                        if (n_clip) { const uint8_t *v = w - PL_POOL_STRIDE; for (uint32_t i = l_ref; i < PL_POOL_STRIDE; ++i) w[i] = v[i]; }
                        else for (uint32_t i = l_ref; i < PL_POOL_STRIDE; ++i) w[i] = (prev_full != 0xFFFFFFFFu && i < l_seq) ? pl_base(pac, (uint64_t)prev_full + i) : (uint8_t)0;
                        for (uint32_t i = 0; i < l_ref; ++i) w[i] = pl_base(pac, (uint64_t)off + i);
                    }
                }
                ++n_clip;
            } else prev_full = off;
            if (item) { Item x; x.read = read; x.offset = off; x.pool = pl; x.tlen = (uint16_t)l_ref; x.strand = (uint8_t)s; x.k = (uint8_t)PL_MAX_DISTANCE; item[k] = x; }
        }
    }
    return PL_OK;
}

// ---- winners -----------------------------------------------------------------------------------------------------------
struct PlWin { int32_t strand, primary, b0, b1; };                         // strand / primary -1: unmapped
PL_HD void pl_pick(const PlHit *h0, uint32_t nu0, const PlHit *h1, uint32_t nu1, PlWin &w)        // polish.c:718-737
{
    int32_t best0 = PL_UNMAPPED, best1 = PL_UNMAPPED;
    w.strand = w.primary = -1;
    for (uint32_t s = 0; s < 2; ++s) {
        const PlHit *h = s ? h1 : h0; const uint32_t nu = s ? nu1 : nu0;
        for (uint32_t j = 0; j < nu; ++j) {
            const int32_t sc = h[j].score;
            if (sc == PL_UNMAPPED) continue;
            if (sc > best1) { best1 = sc; if (best1 > best0) { const int32_t t = best0; best0 = best1; best1 = t; w.strand = (int32_t)s; w.primary = (int32_t)j; } }
        }
    }
    w.b0 = best0; w.b1 = best1;
}
PL_HD uint32_t pl_pairing(PlHit *fw, uint32_t nf, PlHit *bw, uint32_t nb)  // __pairing (polish.c:155-188): swaps in place
{
    uint32_t k = 0, i = 0, j = 0;
    while (i < nf && j < nb) {
        const uint32_t a = fw[i].offset, b = bw[j].offset, d = a > b ? a - b : b - a;
        if (a > b || d < PL_MIN_ISIZE) ++j;
        else if (d > PL_MAX_ISIZE) ++i;
        else { PlHit t = fw[k]; fw[k] = fw[i]; fw[i] = t; t = bw[k]; bw[k] = bw[j]; bw[j] = t; ++i; ++j; ++k; }
    }
    return k;
}
// a pair (polish.c:600-640): a's hits ah0 / ah1, b's bh0 / bh1; true = a proper pair was chosen
PL_HD bool pl_pick_pair(PlHit *ah0, uint32_t an0, PlHit *ah1, uint32_t an1, PlHit *bh0, uint32_t bn0, PlHit *bh1, uint32_t bn1, PlWin &a, PlWin &b)
{
    const uint32_t n0 = pl_pairing(ah0, an0, bh1, bn1), n1 = pl_pairing(bh0, bn0, ah1, an1);
    if (n0 + n1 == 0) { pl_pick(ah0, an0, ah1, an1, a); pl_pick(bh0, bn0, bh1, bn1, b); return false; }
    int32_t best0 = PL_UNMAPPED, best1 = PL_UNMAPPED;
    a.strand = b.strand = a.primary = b.primary = -1;
    for (uint32_t k = 0; k < n0; ++k) {
        const int32_t sc = ah0[k].score + bh1[k].score;
        if (sc == PL_UNMAPPED) continue;
        if (sc > best1) { best1 = sc; if (best1 > best0) { const int32_t t = best0; best0 = best1; best1 = t; a.strand = 0; b.strand = 1; a.primary = b.primary = (int32_t)k; } }
    }
    for (uint32_t k = 0; k < n1; ++k) {
        const int32_t sc = ah1[k].score + bh0[k].score;
        if (sc == PL_UNMAPPED) continue;
        if (sc > best1) { best1 = sc; if (best1 > best0) { const int32_t t = best0; best0 = best1; best1 = t; a.strand = 1; b.strand = 0; a.primary = b.primary = (int32_t)k; } }
    }
    a.b0 = b.b0 = best0; a.b1 = b.b1 = best1;
    return true;
}

// ---- records -----------------------------------------------------------------------------------------------------------
// E: put(char), span(const uint8_t *, n).  PlCount measures, PlWrite writes.
struct PlCount { uint32_t n = 0; PL_HD void put(char) { ++n; } PL_HD void span(const uint8_t *, uint32_t k) { n += k; } };
struct PlWrite { char *o; PL_HD void put(char c) { *o++ = c; } PL_HD void span(const uint8_t *s, uint32_t k) { for (uint32_t i = 0; i < k; ++i) *o++ = (char)s[i]; } };
template <class E> PL_HD void pl_put_u32(E &o, uint32_t v)
{
    char t[10]; int n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) o.put(t[--n]);
}
template <class E> PL_HD void pl_put_str(E &o, const char *s) { while (*s) o.put(*s++); }

// what the printer needs of one record and its winner
struct PlOut {
    const uint8_t *name; uint32_t name_len; const uint8_t *qual; uint32_t qual_len; const uint8_t *codes; uint32_t l_seq; int32_t flag;
    int32_t qual_seq;                                                    // QUAL is as sequenced whatever flag says (the fused route); 0: as the SAM line had it
    PlWin w; uint32_t pos; const uint8_t *chrom; uint32_t chrom_len;     // of the winning hit
    int32_t star; const uint16_t *cigar; uint32_t n_cigar; int32_t clip_front, clip_back;       // star: the LV "*" rule at distance 13
};
template <class E> PL_HD void pl_put_cigar(E &o, const PlOut &r)
{
    if (r.star) { o.put('*'); return; }
    if (r.clip_front > 0) { pl_put_u32(o, (uint32_t)r.clip_front); o.put('S'); }
    for (uint32_t j = 0; j < r.n_cigar; ++j) { pl_put_u32(o, (uint32_t)(r.cigar[j] >> 4)); o.put("MID"[r.cigar[j] & 3]); }
    if (r.clip_back > 0) { pl_put_u32(o, (uint32_t)r.clip_back); o.put('S'); }
}
template <class E> PL_HD void pl_put_seq_qual(E &o, const PlOut &r)
{
    const uint8_t *d = r.codes; const uint32_t L = r.l_seq;
    // the winner's strand (an unmapped read prints its reverse complement: strand == -1 takes the `else` of polish.c:283)
    if (r.w.strand == 0) for (uint32_t j = 0; j < L; ++j) o.put("ACGTN"[d[j] > 4 ? 4 : d[j]]);
    else for (uint32_t j = L; j-- > 0;) { const uint8_t c = d[j]; o.put("ACGTN"[c < 4 ? 3 - c : 4]); }
    o.put('\t');
    const bool rev_in = (r.flag & 0x10) != 0;
    const bool flip = (rev_in && r.w.strand == 0) || (!rev_in && r.w.strand != 0);      // against the line's QUAL
    if (r.qual_seq ? r.w.strand != 0 : flip) for (uint32_t j = r.qual_len; j-- > 0;) o.put((char)r.qual[j]);
    else o.span(r.qual, r.qual_len);
    if (!flip) o.put('\t');                                      // the tab of printf("%s\t", s) (polish.c:289,292)
    o.put('\n');
}
template <class E> PL_HD void pl_print_se(E &o, const PlOut &r)           // polish_sam_se
{
    const bool mapped = r.w.strand != -1;
    o.span(r.name, r.name_len); o.put('\t');
    pl_put_u32(o, 0x40u | (r.w.strand == 1 ? 0x10u : 0u) | (mapped ? 0u : 4u)); o.put('\t');
    if (!mapped) pl_put_str(o, "*\t0\t"); else { o.span(r.chrom, r.chrom_len); o.put('\t'); pl_put_u32(o, r.pos); o.put('\t'); }
    pl_put_str(o, (r.w.b1 == PL_UNMAPPED && r.w.b0 != PL_UNMAPPED) ? "60\t" : "0\t");
    if (mapped) { pl_put_cigar(o, r); o.put('\t'); } else pl_put_str(o, "*\t");
    pl_put_str(o, "*\t0\t0\t");
    pl_put_seq_qual(o, r);
}
PL_HD bool pl_same(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb)
{
    if (na != nb) return false;
    for (uint32_t i = 0; i < na; ++i) if (a[i] != b[i]) return false;
    return true;
}
// record k (0 / 1) of a pair: me, its mate, the first mate's name (polish_sam_pe)
template <class E> PL_HD void pl_print_pe(E &o, const PlOut &me, const PlOut &mate, const PlOut &first, int k, bool proper)
{
    const bool m0 = me.w.strand != -1, m1 = mate.w.strand != -1;
    uint32_t flag = 1u | (proper ? 2u : 0u) | (me.w.strand == 1 ? 0x10u : 0u) | (mate.w.strand == 1 ? 0x20u : 0u) | (k == 0 ? 0x40u : 0x80u) | (m0 ? 0u : 4u);
    if (!m1) flag |= k == 0 ? 8u : 4u;                            // the second record marks itself unmapped when EITHER mate is (polish.c:383-384)
    o.span(first.name, first.name_len); o.put('\t');              // both records print the first mate's name (polish.c:378)
    pl_put_u32(o, flag & 0xFFu); o.put('\t');
    if (!m0) pl_put_str(o, "*\t0\t"); else { o.span(me.chrom, me.chrom_len); o.put('\t'); pl_put_u32(o, me.pos); o.put('\t'); }
    pl_put_str(o, (me.w.b1 == PL_UNMAPPED && me.w.b0 != PL_UNMAPPED) ? "60\t" : "0\t");
    if (m0) { pl_put_cigar(o, me); o.put('\t'); } else pl_put_str(o, "*\t");
    if (!m1) pl_put_str(o, "*\t0\t");
    else if (!m0 || !pl_same(me.chrom, me.chrom_len, mate.chrom, mate.chrom_len)) { o.span(mate.chrom, mate.chrom_len); o.put('\t'); pl_put_u32(o, mate.pos); o.put('\t'); }
    else { pl_put_str(o, "=\t"); pl_put_u32(o, mate.pos); o.put('\t'); }
    if (m0 && m1) {
        const int32_t a = (int32_t)(me.pos < mate.pos ? mate.pos - me.pos : me.pos - mate.pos);
        const int32_t v = me.w.strand == 0 ? a : -a;
        if (v < 0) { o.put('-'); pl_put_u32(o, (uint32_t)0 - (uint32_t)v); } else pl_put_u32(o, (uint32_t)v);
        o.put('\t');
    } else pl_put_str(o, "0\t");
    pl_put_seq_qual(o, me);
}

} // namespace salt_pl
#endif
