// salt_amd/csrc/salt_ctx_record.h -- the context record of a suffix-array row (c_ctx / r_ctx, salt_device.h): its geometry, how it is
// built from the 2-bit text and the allele masks, which read base each of its positions faces, and the lower bound on a candidate
// window's mismatches that it gives.  One source for the device (salt_index.hip builds, salt_align.hip reads) and for the host
// (tools/ctx_model.cc, plain C++: tests/test_ctx_record_model.py runs the same functions against the oracle's masked Hamming count).
//
// Geometry.  A record holds CTX_BASES = 46 genome bases around the suffix start s:
//   side B, CTX_N_B = CTX_N_FRONT bases in front of the suffix:  s - 1, s - 2, ... s - CTX_N_B               (plane bit CTX_N_A + u)
//   side A, CTX_N_A = 46 - CTX_N_FRONT bases behind it:          s + a_start, ... s + a_start + CTX_N_A - 1   (plane bit t)
// with a_start = CTX_A_SEEDS * k + CTX_A_EXTRA for seed length k (ctx_a_start): the seed extension of alnse_seed_overlap moves a seed
// left by whole seed strides, so "beyond the usual extension" is a number of seed lengths, not a literal.  The geometry is a set of
// compile-time constants: ctx_reject runs once per located row in k_heavy's locate loop and its two side masks and the widths of the
// two special-site counts stay immediates; a_start only enters ctx_face (once per seed interval) and the attach-time builder.
// A/B builds: make EXTRA="-DCTX_N_FRONT=23 -DCTX_A_SEEDS=1 -DCTX_NS_BITS_A=2" TAG=_g23 (the symmetric record this one replaced).
//
// Why 9 in front and 37 behind, from 2 k on: DESIGN.md 3 and 5.0, tools/ctx_geometry_model.py.  In short: most located rows of a
// repeat read come from a seed at read offset 0 (nothing in front of it to compare) or from one extended to near offset 0 (side A at
// [k, k + 23) lies inside what already matched).  CTX_N_FRONT stays >= 9: seed_resolve_unique (salt_align.hip) finishes a one-row C
// search of up to CTX_N_FRONT remaining bases from side B, and with k = 21 the W-mer table (W = 12 .. 16) leaves 5 .. 9.
#ifndef SALT_CTX_RECORD_H
#define SALT_CTX_RECORD_H
#include <stdint.h>

#if defined(__HIPCC__)
#define CTX_FN __device__ __forceinline__
#define CTX_POPC64(x) ((uint32_t)__popcll(x))
typedef uint4 CtxRec;
#define CTX_MAKE_REC(x, y, z, w) make_uint4((x), (y), (z), (w))
#else
#define CTX_FN static inline
#define CTX_POPC64(x) ((uint32_t)__builtin_popcountll(x))
struct CtxRec { uint32_t x, y, z, w; };
#define CTX_MAKE_REC(x, y, z, w) CtxRec{ (x), (y), (z), (w) }
#endif

#ifndef CTX_N_FRONT
#define CTX_N_FRONT 9
#endif
#ifndef CTX_A_SEEDS
#define CTX_A_SEEDS 2
#endif
#ifndef CTX_A_EXTRA
#define CTX_A_EXTRA 0
#endif
// Special-site counts: 4 bits in all, CTX_NS_BITS_A of them for side A.  A count at its maximum means "that many or more, or the side
// runs off the genome": the side bounds nothing.  2 + 2 (each side gives up at 3 sites); 3 + 1 lets the long side go on to 6 sites but
// the short one gives up at its first, and rejected no more rows of either bench leg (profiles/r05/ab_ctx_geometry.log).
#ifndef CTX_NS_BITS_A
#define CTX_NS_BITS_A 2
#endif

namespace salt {

static const uint32_t CTX_BASES = 46;
static const uint32_t CTX_N_B = CTX_N_FRONT, CTX_N_A = CTX_BASES - CTX_N_FRONT;
static const uint32_t CTX_NS_BITS_B = 4 - CTX_NS_BITS_A;
static const uint32_t CTX_NS_SAT_A = (1u << CTX_NS_BITS_A) - 1u, CTX_NS_SAT_B = (1u << CTX_NS_BITS_B) - 1u;
static const uint64_t CTX_MASK_A = (1ull << CTX_N_A) - 1ull, CTX_MASK_B = ((1ull << CTX_N_B) - 1ull) << CTX_N_A;
static_assert(CTX_N_FRONT >= 9 && CTX_N_FRONT <= 32 && CTX_N_FRONT < CTX_BASES, "side B: 9 .. 32 bases (seed_resolve_unique reads it as one word)");
static_assert(CTX_NS_BITS_A >= 1 && CTX_NS_BITS_A <= 3, "each side needs a special-site count");
static_assert(CTX_A_SEEDS >= 1, "side A starts behind the seed");

CTX_FN uint32_t ctx_a_start(uint32_t k) { return (uint32_t)CTX_A_SEEDS * k + (uint32_t)CTX_A_EXTRA; }

// 96 bits behind .x: low plane (46), high plane (46), special-site count of A (CTX_NS_BITS_A), of B (the rest of 4)
CTX_FN CtxRec ctx_pack(uint32_t sa, uint64_t lo, uint64_t hi, uint32_t ns_a, uint32_t ns_b)
{
    return CTX_MAKE_REC(sa, (uint32_t)lo, (uint32_t)(lo >> 32) | ((uint32_t)hi << 14), (uint32_t)(hi >> 18) | (ns_a << 28) | (ns_b << (28 + CTX_NS_BITS_A)));
}
CTX_FN uint64_t ctx_plane_lo(const CtxRec rec) { return (uint64_t)rec.y | ((uint64_t)(rec.z & 0x3FFFu) << 32); }
CTX_FN uint64_t ctx_plane_hi(const CtxRec rec) { return (uint64_t)(rec.z >> 14) | ((uint64_t)(rec.w & 0x0FFFFFFFu) << 18); }
// side B alone: bit u = genome base s - 1 - u.  Complete iff CTX_N_FRONT <= s <= len (ctx_build), whatever its special-site count says.
CTX_FN uint32_t ctx_front_lo(const CtxRec rec) { return (uint32_t)(ctx_plane_lo(rec) >> CTX_N_A); }
CTX_FN uint32_t ctx_front_hi(const CtxRec rec) { return (uint32_t)(ctx_plane_hi(rec) >> CTX_N_A); }

// The record of the suffix that starts at genome position s (`first` goes to .x: the suffix-array value or r_pos of the row).
// text: 2 bits per base, 16 per word, first base in the high bits; ref: the allele masks, 4 bits per base, 8 per word, first base in
// the low bits; len: the positions both hold.  A side that does not lie inside [0, len) whole bounds nothing.
CTX_FN CtxRec ctx_build(const uint32_t *text, const uint32_t *ref, uint64_t len, uint32_t first, uint64_t s, uint32_t a_start)
{
    uint64_t lo = 0, hi = 0;
    uint32_t ns[2] = { 0, 0 };
    const bool whole[2] = { s + a_start + CTX_N_A <= len, s >= CTX_N_B && s <= len };
    for (int side = 0; side < 2; ++side) {
        const uint32_t n = side == 0 ? CTX_N_A : CTX_N_B, sat = side == 0 ? CTX_NS_SAT_A : CTX_NS_SAT_B;
        if (!whole[side]) { ns[side] = sat; continue; }
        for (uint32_t t = 0; t < n; ++t) {
            const uint64_t p = side == 0 ? s + a_start + t : s - 1 - t;
            const uint32_t b = (text[p >> 4] >> (30 - 2 * (uint32_t)(p & 15u))) & 3u;
            const uint32_t mask = (ref[p >> 3] >> (4 * (uint32_t)(p & 7u))) & 15u;
            const uint32_t bit = (side == 0 ? 0u : CTX_N_A) + t;
            lo |= (uint64_t)(b & 1u) << bit; hi |= (uint64_t)(b >> 1) << bit;
            ns[side] += mask != (1u << b);
        }
        if (ns[side] > sat) ns[side] = sat;
    }
    return ctx_pack(first, lo, hi, ns[0], ns[1]);
}

// The read's side of the comparison, the same for every row of one seed interval: planes of the read bases facing the record's
// positions, and `use` = the positions that face a base of the read which is not N.
struct CtxRead { uint64_t lo, hi, use; };
// The read base that plane bit t faces for a seed at read offset `off` (the suffix start s faces read base off); negative or >= L: none.
CTX_FN int ctx_face(uint32_t t, uint32_t off, uint32_t a_start)
{
    return t < CTX_N_A ? (int)(off + a_start + t) : t < CTX_BASES ? (int)off - 1 - (int)(t - CTX_N_A) : -1;
}
// A read base as its one-hot nibble 1 << code (N: 15, matches everything and is not counted): its bit in each plane, and whether it counts
CTX_FN bool ctx_nib_lo(uint32_t nib) { return (nib & 0xAu) != 0; }          // code bit 0 is set for 2 and 8
CTX_FN bool ctx_nib_hi(uint32_t nib) { return (nib & 0xCu) != 0; }          // code bit 1 for 4 and 8
CTX_FN bool ctx_nib_use(uint32_t nib) { return nib == 1u || nib == 2u || nib == 4u || nib == 8u; }

// true: the window of this row has more than `bound` mismatches for certain (so ed_mismatch(..., bound) would return -1).
// Mismatches between the 2-bit genome and the read are counted over the usable positions; every special site among them may be a
// match after all (the mask holds more than the genome base), so each side's count is lowered by its special-site count.
CTX_FN bool ctx_reject(const CtxRec rec, const CtxRead rd, uint32_t bound)
{
    const uint64_t m = ((ctx_plane_lo(rec) ^ rd.lo) | (ctx_plane_hi(rec) ^ rd.hi)) & rd.use;
    const uint32_t ns_a = (rec.w >> 28) & CTX_NS_SAT_A, ns_b = rec.w >> (28 + CTX_NS_BITS_A);
    const uint32_t ca = CTX_POPC64(m & CTX_MASK_A), cb = CTX_POPC64(m & CTX_MASK_B);
    const uint32_t la = (ns_a == CTX_NS_SAT_A || ca < ns_a) ? 0u : ca - ns_a, lb = (ns_b == CTX_NS_SAT_B || cb < ns_b) ? 0u : cb - ns_b;
    return la + lb > bound;
}

} // namespace salt
#endif
