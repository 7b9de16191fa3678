// salt_amd/csrc/salt_trim_rule.h -- the trimming rule of DESIGN.md 4.3, for the device's k_fq_trim (salt_trim.hip), the host twin
// (salt_trim_span, host/salt_host.cc) and the stand-alone model program (tools/trim_model.cc): all three compile this one header, as
// salt_vcf_line.h and salt_bgzf_block.h are shared.  The independent statement of the rule is the Python model in tests/trim_check.py.
//
// A read of L >= 1 bases and L quality bytes becomes the span [beg, end), 0 <= beg < end <= L.  The steps, each on the span the one before left:
//   1. clips      beg += front, end -= tail, both saturating (trim_clip)
//   2. quality    the partial-sum rule of `bwa aln -q`: s = best = 0, cut = end; for i = end - 1 down to beg: s += Q - q(i); stop when
//                 s < 0; when s > best: best = s, cut = i.  end = cut.  q(i) = byte - 33, a byte below 33 counts as 0 (trim_q)
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

// The whole rule on one thread.  seq, qual: the read's L >= 1 letters and quality bytes; mate: 0 or 1; counts: the mate's eight counters, or null.
SALT_TRIM_HD void trim_span(const TrimRule &r, uint32_t mate, const uint8_t *seq, const uint8_t *qual, uint32_t L, uint32_t *beg_out, uint32_t *end_out, uint64_t *counts)
{
    uint32_t beg, end;
    trim_clip(r, L, &beg, &end);
    const uint32_t e1 = end;
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
    const uint32_t e2 = end, A = r.a_len[mate & 1u];
    if (A) {
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
    const uint32_t e3 = end;
    const bool floored = trim_floor(L, &beg, &end);
    if (counts) trim_count(counts, L, beg, end, e1, e2, e3, floored);
    *beg_out = beg; *end_out = end;
}

} // namespace salt
#endif
