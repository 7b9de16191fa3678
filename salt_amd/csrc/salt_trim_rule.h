// salt_amd/csrc/salt_trim_rule.h -- the trimming rule of DESIGN.md 4.3, for the device's k_fq_trim and k_fq_trim_pair (salt_trim.hip), the
// host twins (salt_trim_span, salt_trim_pair_span, host/salt_host.cc) and the stand-alone model programs (tools/trim_model.cc,
// tools/trim_pair_model.cc): all compile this one header, as salt_vcf_line.h and salt_bgzf_block.h are shared.  The independent statements
// of the rule are the Python models in tests/trim_check.py and tests/trim_pair_check.py.
//
// A read of L >= 1 bases and L quality bytes becomes the span [beg, end), 0 <= beg < end <= L.  The steps, each on the span the one before left:
//   1. clips      beg += front, end -= tail, both saturating (trim_clip)
//   2. quality    the partial-sum rule of `bwa aln -q`: s = best = 0, cut = end; for i = end - 1 down to beg: s += Q - q(i); stop when
//                 s < 0; when s > best: best = s, cut = i.  end = cut.  q(i) = byte - 33, a byte below 33 counts as 0 (trim_q)
//   2p. pair     (pairs only, when switched on) the adapter found from the mates' overlap: see trim_pair_span below
//   3. adapter    every start p from beg upward, ov = min(A, end - p); the search ends at the first p with ov < M; mm = the j < ov where
//                 the read's letter p + j is not the adapter's letter j (case ignored; a read letter outside ACGTacgt always differs);
//                 the leftmost p with 100 mm <= E ov wins: end = p (trim_accept)
//   4. floor      end <= beg: beg = min(beg, L - 1), end = beg + 1 (trim_floor)
// Integers only.  The pieces are what both sides are made of: trim_span below walks them one position at a time on one thread; k_fq_trim
// gives every start position and every quality a lane, and calls the same pieces.  Both keep the read as three bit planes.
//
// Bit planes: a stretch of up to 64 letters is three 64-bit words, bit j for letter j: lo and hi hold the two bits of the code (A 0, C 1,
// G 2, T 3), nn is set where the letter is none of ACGTacgt.  The adapter has no nn plane (its letters are checked when it is set).
#ifndef SALT_TRIM_RULE_H
#define SALT_TRIM_RULE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SALT_TRIM_HD __host__ __device__ __forceinline__
#else
#define SALT_TRIM_HD inline
#endif

namespace salt {

static const uint32_t TRIM_MAX_ADAPTER = 64, TRIM_MAX_CLIP = 511, TRIM_MAX_QUAL = 93, TRIM_MAX_ERROR_PCT = 50;
// the counters of one mate (salt_gpu_ws_trim_counts: eight for mate 1, then eight for mate 2)
enum { TRIM_READS = 0, TRIM_BASES_IN = 1, TRIM_BASES_OUT = 2, TRIM_READS_QUAL = 3, TRIM_BASES_QUAL = 4, TRIM_READS_ADAPTER = 5, TRIM_BASES_ADAPTER = 6,
       TRIM_READS_FLOORED = 7, TRIM_N_COUNTS = 8 };

// The options as the rule reads them: by value into the kernel.  Adapter m is the one mate m is searched with (a_len 0: none).
struct TrimRule {
    uint64_t a_lo[2], a_hi[2];
    uint32_t a_len[2];
    uint32_t front, tail, qual, min_overlap, error_pct;
};
SALT_TRIM_HD bool trim_rule_on(const TrimRule &r) { return (r.front | r.tail | r.qual | r.a_len[0] | r.a_len[1]) != 0; }

// code of a letter: 0 .. 3, or 4 for anything that is not ACGTacgt
SALT_TRIM_HD uint32_t trim_code(uint8_t c)
{
    c |= 0x20;
    return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : c == 't' ? 3u : 4u;
}
SALT_TRIM_HD int32_t trim_q(uint8_t c) { return c < 33 ? 0 : (int32_t)c - 33; }
SALT_TRIM_HD uint64_t trim_low_bits(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }

// step 1
SALT_TRIM_HD void trim_clip(const TrimRule &r, uint32_t L, uint32_t *beg, uint32_t *end)
{
    const uint32_t b = r.front < L ? r.front : L;
    const uint32_t e = L - b > r.tail ? L - r.tail : b;
    *beg = b; *end = e;
}
// step 3: the mismatches of a window of ov letters (its planes start at bit 0) against the adapter's first ov letters, and the verdict
SALT_TRIM_HD uint32_t trim_window_mm(uint64_t lo, uint64_t hi, uint64_t nn, uint64_t a_lo, uint64_t a_hi, uint32_t ov)
{
    const uint64_t m = ((lo ^ a_lo) | (hi ^ a_hi) | nn) & trim_low_bits(ov);
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(m);
#else
    return (uint32_t)__builtin_popcountll(m);
#endif
}
SALT_TRIM_HD bool trim_accept(const TrimRule &r, uint32_t mm, uint32_t ov) { return ov >= r.min_overlap && 100u * mm <= r.error_pct * ov; }
// the 64 bits from bit k on of (w1 : w0): the window of the start that lies k letters into the tile w0
SALT_TRIM_HD uint64_t trim_window(uint64_t w0, uint64_t w1, uint32_t k) { return k ? (w0 >> k) | (w1 << (64u - k)) : w0; }
// letters [at, at + 64) of a span of n letters as planes, one letter after the other (the kernel takes a lane a letter and ballots); behind the span: 0
struct TrimPlanes { uint64_t lo, hi, nn; };
SALT_TRIM_HD TrimPlanes trim_pack_tile(const uint8_t *s, uint32_t n, uint32_t at)
{
    TrimPlanes p = { 0, 0, 0 };
    for (uint32_t j = 0; j < 64u && at < n && j < n - at; ++j) {
        const uint32_t c = trim_code(s[at + j]);
        p.lo |= (uint64_t)(c & 1u) << j; p.hi |= (uint64_t)((c >> 1) & 1u) << j; p.nn |= (uint64_t)(c >> 2) << j;
    }
    return p;
}
// step 4; true: the floor applied
SALT_TRIM_HD bool trim_floor(uint32_t L, uint32_t *beg, uint32_t *end)
{
    if (*end > *beg) return false;
    if (*beg > L - 1u) *beg = L - 1u;
    *end = *beg + 1u;
    return true;
}
// what one read adds to its mate's counters: e1, e2, e3 = the span's end behind steps 1, 2 and 3
SALT_TRIM_HD void trim_count(uint64_t *c, uint32_t L, uint32_t beg, uint32_t end, uint32_t e1, uint32_t e2, uint32_t e3, bool floored)
{
    c[TRIM_READS] += 1; c[TRIM_BASES_IN] += L; c[TRIM_BASES_OUT] += end - beg;
    c[TRIM_READS_QUAL] += e2 < e1; c[TRIM_BASES_QUAL] += e1 - e2;
    c[TRIM_READS_ADAPTER] += e3 < e2; c[TRIM_BASES_ADAPTER] += e2 - e3;
    c[TRIM_READS_FLOORED] += floored;
}

// The adapter's planes from its letters; false: a letter outside ACGTacgt, or more than 64 of them.
SALT_TRIM_HD bool trim_pack_adapter(const char *s, uint32_t n, uint64_t *lo, uint64_t *hi)
{
    *lo = 0; *hi = 0;
    if (n > TRIM_MAX_ADAPTER) return false;
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t c = trim_code((uint8_t)s[j]);
        if (c > 3u) return false;
        *lo |= (uint64_t)(c & 1u) << j; *hi |= (uint64_t)(c >> 1) << j;
    }
    return true;
}

// The options as a caller gives them -> the rule.  Null, or what is wrong: the message names the field and its range.  All zero: a rule that is off.
inline const char *trim_rule_make(const char *adapter, uint32_t n1, const char *adapter2, uint32_t n2, uint32_t front, uint32_t tail, uint32_t qual,
                                  uint32_t min_overlap, uint32_t error_pct, TrimRule *out)
{
    TrimRule r = TrimRule();
    if (!adapter) n1 = 0;
    if (!adapter2) n2 = 0;
    if (front > TRIM_MAX_CLIP) return "trim: front outside 0 .. 511";
    if (tail > TRIM_MAX_CLIP) return "trim: tail outside 0 .. 511";
    if (qual > TRIM_MAX_QUAL) return "trim: qual outside 1 .. 93 (0: off)";
    if (n1 > TRIM_MAX_ADAPTER) return "trim: adapter longer than 64 letters";
    if (n2 > TRIM_MAX_ADAPTER) return "trim: adapter2 longer than 64 letters";
    if (n2 && !n1) return "trim: adapter2 without adapter";
    if (!n1 && min_overlap) return "trim: min_overlap without an adapter";
    if (!n1 && error_pct) return "trim: error_pct without an adapter";
    if (n1) {
        if (min_overlap < 1 || min_overlap > TRIM_MAX_ADAPTER) return "trim: min_overlap outside 1 .. 64";
        if (error_pct > TRIM_MAX_ERROR_PCT) return "trim: error_pct outside 0 .. 50";
        if (!trim_pack_adapter(adapter, n1, &r.a_lo[0], &r.a_hi[0])) return "trim: adapter holds a letter outside ACGTacgt";
        r.a_len[0] = n1;
        if (n2) {
            if (!trim_pack_adapter(adapter2, n2, &r.a_lo[1], &r.a_hi[1])) return "trim: adapter2 holds a letter outside ACGTacgt";
            r.a_len[1] = n2;
        } else { r.a_lo[1] = r.a_lo[0]; r.a_hi[1] = r.a_hi[0]; r.a_len[1] = n1; }
    }
    r.front = front; r.tail = tail; r.qual = qual; r.min_overlap = min_overlap; r.error_pct = error_pct;
    *out = r;
    return nullptr;
}

// Steps 1 and 2 on one thread: the span they leave; *e1_out = the end behind the clips.
SALT_TRIM_HD void trim_span_clip_qual(const TrimRule &r, const uint8_t *qual, uint32_t L, uint32_t *beg_out, uint32_t *end_out, uint32_t *e1_out)
{
    uint32_t beg, end;
    trim_clip(r, L, &beg, &end);
    *e1_out = end;
    if (r.qual) {
        int64_t s = 0, best = 0;
        uint32_t cut = end;
        for (uint32_t i = end; i-- > beg;) {
            s += (int64_t)r.qual - trim_q(qual[i]);
            if (s < 0) break;
            if (s > best) { best = s; cut = i; }
        }
        end = cut;
    }
    *beg_out = beg; *end_out = end;
}
// Step 3 on one thread: the end it leaves of the span [beg, end) (end <= beg: nothing to search).
SALT_TRIM_HD uint32_t trim_span_adapter(const TrimRule &r, uint32_t mate, const uint8_t *seq, uint32_t beg, uint32_t end)
{
    const uint32_t A = r.a_len[mate & 1u];
    if (A && end > beg) {
        const uint64_t a_lo = r.a_lo[mate & 1u], a_hi = r.a_hi[mate & 1u];
        // tiles of 64 starts: the span's letters packed once, 64 to a word a plane; a start's window is two words of it shifted together
        const uint8_t *sp = seq + beg;
        const uint32_t n = end - beg;
        TrimPlanes w0 = trim_pack_tile(sp, n, 0);
        for (uint32_t at = 0, found = 0; at < n && !found; at += 64) {
            const TrimPlanes w1 = trim_pack_tile(sp, n, at + 64u);
            for (uint32_t k = 0; k < 64u && at + k < n; ++k) {
                const uint32_t ov = n - (at + k) < A ? n - (at + k) : A;
                if (ov < r.min_overlap) { found = 1; break; }                 // every later overlap is shorter still
                const uint32_t mm = trim_window_mm(trim_window(w0.lo, w1.lo, k), trim_window(w0.hi, w1.hi, k), trim_window(w0.nn, w1.nn, k), a_lo, a_hi, ov);
                if (trim_accept(r, mm, ov)) { end = beg + at + k; found = 1; break; }
            }
            w0 = w1;
        }
    }
    return end;
}

// The whole rule on one thread.  seq, qual: the read's L >= 1 letters and quality bytes; mate: 0 or 1; counts: the mate's eight counters, or null.
SALT_TRIM_HD void trim_span(const TrimRule &r, uint32_t mate, const uint8_t *seq, const uint8_t *qual, uint32_t L, uint32_t *beg_out, uint32_t *end_out, uint64_t *counts)
{
    uint32_t beg, end, e1;
    trim_span_clip_qual(r, qual, L, &beg, &end, &e1);
    const uint32_t e2 = end;
    end = trim_span_adapter(r, mate, seq, beg, end);
    const uint32_t e3 = end;
    const bool floored = trim_floor(L, &beg, &end);
    if (counts) trim_count(counts, L, beg, end, e1, e2, e3, floored);
    *beg_out = beg; *end_out = end;
}

// ---- step 2p: the adapter found from the mates' overlap (pairs only, and only when switched on) ------------------------------------------
// All positions are in the mates' untrimmed reads of L1 and L2 letters; [b1, e1) and [b2, e2) are what steps 1 and 2 left.  For a candidate
// insert length I >= 1, column j of mate 1 faces letter I - 1 - j of mate 2, complemented: with R the reverse complement of mate 2's L2
// letters, r1[j] faces R[j + L2 - I] (the shift L2 - I may be negative).  Compared are the columns max(b1, I - e2) <= j < min(e1, I - b2):
// ov(I) of them, mm(I) of those where the letters are no complementary pair (case ignored, a letter outside ACGTacgt always differs).
// I is accepted when ov >= P and 100 mm <= Ep ov; the LARGEST accepted I in 1 .. e1 + e2 - P wins: e1 = min(e1, I), e2 = min(e2, I).
// A pair with a mate of more than TRIM_PAIR_MAX_LEN letters skips the step (it is counted in TRIM_PAIR_SKIPPED_LONG).
static const uint32_t TRIM_PAIR_MAX_LEN = 512, TRIM_PAIR_WORDS = 8, TRIM_PAIR_MAX_OVERLAP = 512;
enum { TRIM_PAIR_PAIRS = 0, TRIM_PAIR_OVERLAPPING = 1, TRIM_PAIR_TRIMMED = 2, TRIM_PAIR_READS1 = 3, TRIM_PAIR_BASES1 = 4, TRIM_PAIR_READS2 = 5, TRIM_PAIR_BASES2 = 6,
       TRIM_PAIR_SKIPPED_LONG = 7, TRIM_PAIR_N_COUNTS = 8 };
struct TrimPairRule { uint32_t min_overlap, error_pct; };          // min_overlap 0: off
SALT_TRIM_HD bool trim_pair_on(const TrimPairRule &p) { return p.min_overlap != 0; }
inline const char *trim_pair_rule_make(uint32_t min_overlap, uint32_t error_pct, TrimPairRule *out)
{
    TrimPairRule p = { 0, 0 };
    if (min_overlap || error_pct) {
        if (min_overlap < 1 || min_overlap > TRIM_PAIR_MAX_OVERLAP) return "trim pair: min_overlap outside 1 .. 512";
        if (error_pct > TRIM_MAX_ERROR_PCT) return "trim pair: error_pct outside 0 .. 50";
        p.min_overlap = min_overlap; p.error_pct = error_pct;
    }
    *out = p;
    return nullptr;
}
// 64 columns of a read, a word a plane: the three planes of the letters and va, set where the column lies in the read's span.  A read is
// TRIM_PAIR_WORDS of them: mate 1 as it is, mate 2 as R (letter k of R = the complement of letter L2 - 1 - k, va over [L2 - e2, L2 - b2)).
struct TrimPairWord { uint64_t lo, hi, nn, va; };
SALT_TRIM_HD uint32_t trim_code_rc(uint32_t c) { return c < 4u ? 3u - c : 4u; }
SALT_TRIM_HD void trim_pair_pack(const uint8_t *seq, uint32_t L, uint32_t beg, uint32_t end, bool rc, TrimPairWord *w /* [TRIM_PAIR_WORDS] */)
{
    for (uint32_t t = 0; t < TRIM_PAIR_WORDS; ++t) { w[t].lo = 0; w[t].hi = 0; w[t].nn = 0; w[t].va = 0; }
    const uint32_t vb = rc ? L - end : beg, ve = rc ? L - beg : end;
    for (uint32_t k = 0; k < L; ++k) {
        const uint32_t c = rc ? trim_code_rc(trim_code(seq[L - 1u - k])) : trim_code(seq[k]);
        TrimPairWord &x = w[k >> 6];
        const uint32_t j = k & 63u;
        x.lo |= (uint64_t)(c & 1u) << j; x.hi |= (uint64_t)((c >> 1) & 1u) << j; x.nn |= (uint64_t)(c >> 2) << j;
        x.va |= (uint64_t)(k >= vb && k < ve) << j;
    }
}
SALT_TRIM_HD uint32_t trim_popc(uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(m);
#else
    return (uint32_t)__builtin_popcountll(m);
#endif
}
// mm(I) and ov(I): for every word of mate 1 (n1 of them hold its span's end), R's 64 columns from bit 64 w + L2 - I on -- two neighbouring
// words joined as trim_window joins them, nothing outside R's words
SALT_TRIM_HD void trim_pair_eval(const TrimPairWord *m1, const TrimPairWord *R, uint32_t n1, uint32_t L2, uint32_t I, uint32_t *mm_out, uint32_t *ov_out)
{
    const int32_t shift = (int32_t)L2 - (int32_t)I;
    uint32_t mm = 0, ov = 0;
    for (uint32_t w = 0; w < n1; ++w) {
        const int32_t p = (int32_t)(64u * w) + shift, q = p >> 6;            // (an arithmetic shift: the floor, also of a negative p)
        const uint32_t k = (uint32_t)p & 63u;
        TrimPairWord r0 = { 0, 0, 0, 0 }, r1 = { 0, 0, 0, 0 };
        if ((uint32_t)q < TRIM_PAIR_WORDS) r0 = R[q];
        if ((uint32_t)(q + 1) < TRIM_PAIR_WORDS) r1 = R[q + 1];
        const uint64_t mask = m1[w].va & trim_window(r0.va, r1.va, k);
        mm += trim_popc(((m1[w].lo ^ trim_window(r0.lo, r1.lo, k)) | (m1[w].hi ^ trim_window(r0.hi, r1.hi, k)) | m1[w].nn | trim_window(r0.nn, r1.nn, k)) & mask);
        ov += trim_popc(mask);
    }
    *mm_out = mm; *ov_out = ov;
}
SALT_TRIM_HD bool trim_pair_accept(const TrimPairRule &p, uint32_t mm, uint32_t ov) { return ov >= p.min_overlap && 100u * mm <= p.error_pct * ov; }
// the largest candidate, and how many words of mate 1 its columns can lie in
SALT_TRIM_HD uint32_t trim_pair_first(const TrimPairRule &p, uint32_t e1, uint32_t e2) { return e1 + e2 > p.min_overlap ? e1 + e2 - p.min_overlap : 0u; }
SALT_TRIM_HD uint32_t trim_pair_words(uint32_t e1) { return (e1 + 63u) >> 6; }
// what one pair adds to the eight pair counters: I = the accepted layout (0: none), e1, e2 the ends step 2 left; skipped: a mate too long
SALT_TRIM_HD void trim_pair_count(uint64_t *c, uint32_t I, uint32_t e1, uint32_t e2, bool skipped)
{
    const uint32_t t1 = I && I < e1 ? e1 - I : 0u, t2 = I && I < e2 ? e2 - I : 0u;
    c[TRIM_PAIR_PAIRS] += 1; c[TRIM_PAIR_OVERLAPPING] += I != 0; c[TRIM_PAIR_TRIMMED] += (t1 | t2) != 0;
    c[TRIM_PAIR_READS1] += t1 != 0; c[TRIM_PAIR_BASES1] += t1; c[TRIM_PAIR_READS2] += t2 != 0; c[TRIM_PAIR_BASES2] += t2;
    c[TRIM_PAIR_SKIPPED_LONG] += skipped;
}
// a mate's counters where step 2p stands between steps 2 and 3: the adapter's are what step 3 took from what step 2p left (e2p)
SALT_TRIM_HD void trim_count_pair(uint64_t *c, uint32_t L, uint32_t beg, uint32_t end, uint32_t e1, uint32_t e2, uint32_t e2p, uint32_t e3, bool floored)
{
    trim_count(c, L, beg, end, e1, e2, e2, floored);
    c[TRIM_READS_ADAPTER] += e3 < e2p; c[TRIM_BASES_ADAPTER] += e2p - e3;
}

// Step 2p on one thread: the accepted layout I*, or 0.
SALT_TRIM_HD uint32_t trim_pair_find(const TrimPairRule &p, const uint8_t *seq1, uint32_t L1, uint32_t b1, uint32_t e1, const uint8_t *seq2, uint32_t L2, uint32_t b2, uint32_t e2)
{
    TrimPairWord m1[TRIM_PAIR_WORDS], R[TRIM_PAIR_WORDS];
    trim_pair_pack(seq1, L1, b1, e1, false, m1);
    trim_pair_pack(seq2, L2, b2, e2, true, R);
    const uint32_t n1 = trim_pair_words(e1);
    for (uint32_t I = trim_pair_first(p, e1, e2); I >= 1u; --I) {
        uint32_t mm, ov;
        trim_pair_eval(m1, R, n1, L2, I, &mm, &ov);
        if (trim_pair_accept(p, mm, ov)) return I;
    }
    return 0;
}

// The whole rule on one pair, one thread.  span: b1, e1, b2, e2; counts: the sixteen per-mate counters or null; pair_counts: the eight or null.
// With the pair rule off, each mate's span and counters are trim_span's.
SALT_TRIM_HD void trim_pair_span(const TrimRule &r, const TrimPairRule &p, const uint8_t *seq1, const uint8_t *qual1, uint32_t L1, const uint8_t *seq2, const uint8_t *qual2,
                                 uint32_t L2, uint32_t *span, uint64_t *counts, uint64_t *pair_counts)
{
    const uint8_t *seq[2] = { seq1, seq2 }, *qual[2] = { qual1, qual2 };
    const uint32_t L[2] = { L1, L2 };
    uint32_t beg[2], end[2], e1[2], e2[2], e2p[2];
    for (uint32_t m = 0; m < 2; ++m) { trim_span_clip_qual(r, qual[m], L[m], &beg[m], &end[m], &e1[m]); e2[m] = end[m]; }
    if (trim_pair_on(p)) {
        const bool skipped = L1 > TRIM_PAIR_MAX_LEN || L2 > TRIM_PAIR_MAX_LEN;
        const uint32_t I = skipped ? 0u : trim_pair_find(p, seq1, L1, beg[0], end[0], seq2, L2, beg[1], end[1]);
        if (pair_counts) trim_pair_count(pair_counts, I, end[0], end[1], skipped);
        if (I) for (uint32_t m = 0; m < 2; ++m) end[m] = end[m] < I ? end[m] : I;
    }
    for (uint32_t m = 0; m < 2; ++m) {
        e2p[m] = end[m];
        end[m] = trim_span_adapter(r, m, seq[m], beg[m], end[m]);
        const uint32_t e3 = end[m];
        const bool floored = trim_floor(L[m], &beg[m], &end[m]);
        if (counts) trim_count_pair(counts + TRIM_N_COUNTS * m, L[m], beg[m], end[m], e1[m], e2[m], e2p[m], e3, floored);
        span[2 * m] = beg[m]; span[2 * m + 1] = end[m];
    }
}

} // namespace salt
#endif
