// salt_amd/csrc/salt_bgzf_block.h -- one BGZF block (RFC 1952 member with the 'BC' extra field around one dynamic-Huffman deflate block,
// RFC 1951) made by one workgroup from at most BGZF_CUT bytes of text held in LDS.  k_bgzf_deflate (salt_bgzf.hip) is the caller.
//
// The block's work is a fixed list of PHASES.  Inside a phase every thread works on its own (LDS / global atomics apart); what one
// phase writes the next one reads; on the device a phase ends in __syncthreads().  No barrier and no cross-lane operation sits inside
// divergent control flow: every phase is entered by all threads, and every loop around a phase has a trip count that depends on the
// block's length alone.  Compiled without hipcc the same source runs the phases one thread after the other (tools/bgzf_model.cc,
// tests/test_bgzf_model.py): the phase list is checked on a machine without a GPU, against zlib's inflate.
//
//   stage      text -> LDS (bytes behind the text read 0), tables cleared
//   crc        table-driven CRC-32 (four bytes per step) of every 128-byte piece; pieces combined by a tree of "advance by 128 * 2^k bytes" operators
//              (32 x 32 bit matrices, tabulated at compile time); the last n % 128 bytes by one thread
//   match      LZ77 candidates in rounds of BGZF_THREADS positions: a round READS the hash table (4-byte hash -> latest position of an
//              EARLIER round) and, after a barrier, enters its own positions with an LDS atomicMax -- the table never depends on wave
//              scheduling.  Only the candidate's distance is kept per position
//   parse      greedy, per lane over BGZF_SEG-byte segments: where the parse comes to a position, the candidate's match is measured
//              against the block's own text (matches reach back over segment borders, and end with the segment); histograms by LDS
//              atomics.  The later passes walk the same parse from the lengths this one leaves
//   codes      length-limited Huffman codes (15 bits; 7 for the code-length code): symbols ranked by count, the tree by the two-queue
//              method, depths by walking up, overlong codes folded back until the Kraft sum fits, canonical codes
//   bits       per-lane bit counts and their prefix sums (two levels: groups of 16, then the groups); the block is assembled in LDS,
//              where the candidates' distances lay (a match keeps its own in the two bytes behind its length): every lane writes its
//              symbols at its own bit offset, whole words by plain stores, the first and last word of its range by atomic OR into words
//              cleared beforehand; the block header's code lengths go out the same way, one per thread.  The image leaves for the
//              block's slot in one coalesced copy
//   stored     when the deflated payload would not be smaller than the text: a stored block (BTYPE 0)
#ifndef SALT_BGZF_BLOCK_H
#define SALT_BGZF_BLOCK_H
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BGZF_FN __device__ __forceinline__
#define BGZF_MFN __device__ __forceinline__
#define BGZF_CONST __constant__
#define BGZF_TID const uint32_t tid = tid0;
#define BGZF_PHASE {
#define BGZF_END } __syncthreads();
#define BGZF_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define BGZF_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define BGZF_ATOMIC_OR(p, v) atomicOr((p), (v))
#else
#define BGZF_FN static inline
#define BGZF_MFN inline
#define BGZF_CONST static
#define BGZF_TID (void)tid0;
#define BGZF_PHASE for (uint32_t tid = 0; tid < BGZF_THREADS; ++tid) {
#define BGZF_END }
#define BGZF_ATOMIC_MAX(p, v) do { if (*(p) < (v)) *(p) = (v); } while (0)
#define BGZF_ATOMIC_ADD(p, v) (*(p) += (v))
#define BGZF_ATOMIC_OR(p, v) (*(p) |= (v))
#endif

namespace salt {
namespace bgzf {

// The block cut: 32 640 = 0xff00 / 2 text bytes per block.  htslib's 65 280 would need 64 KiB of text + 192 KiB of match records in LDS;
// at 32 640 the text (32 KiB), one match record per position (1 + 2 bytes: 96 KiB) and the hash table (16 KiB) fit the 160 KiB of a CU
// together, and a 32-MiB FASTQ chunk (about 41 MB of SAM) gives 1 280 blocks for the 256 CUs instead of 640.  DESIGN.md 4.3.
constexpr uint32_t BGZF_CUT = 32640;
constexpr uint32_t BGZF_SLOT = 32768;                        // stride of the blocks' slots before compaction: a block is at most BGZF_CUT + 31 bytes
constexpr uint32_t BGZF_THREADS = 512;
constexpr uint32_t BGZF_SEG = 64, BGZF_NSEG = BGZF_CUT / BGZF_SEG;          // parse segments: 510 lanes
constexpr uint32_t BGZF_CSEG = 128, BGZF_NCSEG = BGZF_CUT / BGZF_CSEG, BGZF_CRC_LEVELS = 8;      // CRC pieces: 255, combined in 8 levels
constexpr uint32_t BGZF_HBITS = 12;
constexpr uint32_t BGZF_MIN_MATCH = 4;                                     // the hash is over 4 bytes; a match ends with its segment at the latest
constexpr uint32_t BGZF_NLL = 286, BGZF_ND = 30, BGZF_NCL = 19;
static_assert(BGZF_NSEG + 2 <= BGZF_THREADS && BGZF_NCSEG <= BGZF_THREADS && BGZF_NLL <= BGZF_THREADS, "lanes");
static_assert(BGZF_CUT + 31 <= BGZF_SLOT && BGZF_CUT % 16 == 0, "slot");

struct CrcTables { uint32_t tab[4][256]; uint32_t mat[BGZF_CRC_LEVELS][32]; };      // tab[k][b]: byte b, then k zero bytes (slicing by 4)
constexpr CrcTables make_crc_tables()
{
    CrcTables t{};
    for (uint32_t i = 0; i < 256; ++i) { uint32_t c = i; for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1; t.tab[0][i] = c; }
    for (uint32_t k = 1; k < 4; ++k) for (uint32_t i = 0; i < 256; ++i) t.tab[k][i] = t.tab[0][t.tab[k - 1][i] & 0xff] ^ (t.tab[k - 1][i] >> 8);
    for (uint32_t j = 0; j < 32; ++j) {                     // column j of "the CRC state BGZF_CSEG zero bytes later"
        uint32_t c = 1u << j;
        for (uint32_t b = 0; b < BGZF_CSEG; ++b) c = t.tab[0][c & 0xff] ^ (c >> 8);
        t.mat[0][j] = c;
    }
    for (uint32_t k = 1; k < BGZF_CRC_LEVELS; ++k)           // squared: twice as far
        for (uint32_t j = 0; j < 32; ++j) {
            const uint32_t v = t.mat[k - 1][j]; uint32_t r = 0;
            for (uint32_t i = 0; i < 32; ++i) if ((v >> i) & 1) r ^= t.mat[k - 1][i];
            t.mat[k][j] = r;
        }
    return t;
}
BGZF_CONST const CrcTables k_crc = make_crc_tables();
BGZF_CONST const uint8_t k_cl_order[BGZF_NCL] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

struct HuffScratch {                                         // one code under construction (lies over the hash table, which is done by then)
    uint32_t nfreq[2 * 288];                                 // counts of the leaves in rank order, then of the inner nodes in the order they are made
    uint16_t parent[2 * 288];
    uint16_t sorted[288];                                    // symbol of rank r (ascending count, ties by symbol)
    uint32_t bl_count[16], first_rank[17], next_code[16];
    uint32_t n_used;
};

struct BlockLds {
    uint32_t text32[(BGZF_CUT + 16) / 4];                    // the text; bytes behind it are 0
    uint8_t  mlen[BGZF_CUT];                                 // per position the parse came to: 0 = literal, else the length - 2 of its match, and its distance in the two bytes behind
    union {
        uint16_t mdist[BGZF_CUT];                            // per position: distance to its candidate, 0 = none; until the first parse has been
        uint32_t out[BGZF_CUT / 2];                          // then the block is assembled here
    } v;
    union { uint32_t htab[1u << BGZF_HBITS]; HuffScratch hs; } u;      // 4-byte hash -> position + 1 (0 = none)
    uint32_t crc_tab[4][256], crc_mat[BGZF_CRC_LEVELS][32];
    uint32_t hist_ll[288], hist_d[32], hist_cl[20];
    uint16_t code_ll[288], code_d[32], code_cl[20];
    uint8_t  len_ll[288], len_d[32], len_cl[20];
    uint8_t  hdr_len[320]; uint16_t hdr_off[320];            // the code lengths as the block header sends them: bits of each, and where it starts
    uint32_t lane_a[BGZF_THREADS], lane_b[BGZF_THREADS];     // CRC pieces (ping-pong); then lane_a = bits per lane, lane_b = their prefix sums inside groups of 16
    uint32_t grp[32], hgrp[32];                              // bits in front of a group of 16 lanes / of 16 header code lengths
    uint32_t crc, hlit, hdist, hclen, hdr_bits, hdr_sym_bits, sym_bits, payload_bytes, stored, block_size;
};
static_assert(sizeof(BlockLds) <= 160 * 1024, "one CU's LDS");

BGZF_FN uint32_t load32u(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

// ---- symbols of RFC 1951 3.2.5 ----
BGZF_FN void len_symbol(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev)         // len 3 .. 258
{
    const uint32_t l = len - 3;
    if (l < 8) { sym = 257 + l; eb = 0; ev = 0; return; }
    const uint32_t msb = 31u - (uint32_t)__builtin_clz(l);
    eb = msb - 2; sym = 257 + 4 * (eb + 1) + ((l >> eb) & 3); ev = l & ((1u << eb) - 1);
}
BGZF_FN void dist_symbol(uint32_t dist, uint32_t &sym, uint32_t &eb, uint32_t &ev)       // dist 1 .. 32768
{
    const uint32_t d = dist - 1;
    if (d < 4) { sym = d; eb = 0; ev = 0; return; }
    const uint32_t msb = 31u - (uint32_t)__builtin_clz(d);
    eb = msb - 1; sym = 2 * msb + ((d >> eb) & 1); ev = d & ((1u << eb) - 1);
}

// The greedy parse of segment `lane`, first pass: at every position it comes to, the candidate's match is measured against the block's
// own text -- up to the segment's end, where the next lane starts -- and kept in mlen[] for the passes that follow.  Positions inside a
// match are never looked at: the compare work is what the parse uses, not one compare per byte of text.
template <class Lit, class Match>
BGZF_FN void parse_segment(BlockLds &s, uint32_t lane, uint32_t n, Lit lit, Match match)
{
    const uint8_t *tx = reinterpret_cast<const uint8_t *>(s.text32);
    uint32_t p = lane * BGZF_SEG;
    const uint32_t end = p + BGZF_SEG < n ? p + BGZF_SEG : n;
    while (p < end) {
        const uint32_t dist = s.v.mdist[p], maxl = end - p;
        uint32_t len = 0;
        if (dist && maxl >= BGZF_MIN_MATCH) {
            while (len < maxl) {
                const uint32_t x = load32u(tx + p + len) ^ load32u(tx + p - dist + len);
                if (x) { len += (uint32_t)__builtin_ctz(x) >> 3; break; }
                len += 4;
            }
            if (len > maxl) len = maxl;
        }
        if (len >= BGZF_MIN_MATCH) { s.mlen[p] = (uint8_t)(len - 2); s.mlen[p + 1] = (uint8_t)dist; s.mlen[p + 2] = (uint8_t)(dist >> 8); match(len, dist); p += len; }
        else { s.mlen[p] = 0; lit((uint32_t)tx[p]); ++p; }
    }
}

// The same parse again (bit count, emit): lit(byte) / match(len, dist) in text order, from the records the first pass left.
template <class Lit, class Match>
BGZF_FN void walk_segment(const BlockLds &s, uint32_t lane, uint32_t n, Lit lit, Match match)
{
    const uint8_t *tx = reinterpret_cast<const uint8_t *>(s.text32);
    uint32_t p = lane * BGZF_SEG;
    const uint32_t end = p + BGZF_SEG < n ? p + BGZF_SEG : n;
    while (p < end) {
        const uint32_t len = s.mlen[p] ? (uint32_t)s.mlen[p] + 2u : 0u;
        if (len) { match(len, (uint32_t)s.mlen[p + 1] | (uint32_t)s.mlen[p + 2] << 8); p += len; }
        else { lit((uint32_t)tx[p]); ++p; }
    }
}

// Bits into the block's image in LDS from an arbitrary bit position on.  Words that lie wholly inside what this writer puts are stored; its
// first and last word, shared with the neighbours, are OR-ed into the (cleared) image.
struct BitWriter {
    uint32_t *w; uint64_t acc; uint32_t n_acc, pos; bool shared;
    BGZF_MFN void open(uint32_t *words, uint32_t bit) { w = words; acc = 0; pos = bit >> 5; n_acc = bit & 31; shared = n_acc != 0; }
    BGZF_MFN void put(uint32_t v, uint32_t nb)                 // nb <= 32; bits of v above nb are 0
    {
        acc |= (uint64_t)v << n_acc; n_acc += nb;
        if (n_acc >= 32) {
            if (shared) { BGZF_ATOMIC_OR(&w[pos], (uint32_t)acc); shared = false; } else w[pos] = (uint32_t)acc;
            acc >>= 32; n_acc -= 32; ++pos;
        }
    }
    BGZF_MFN void close() { if (n_acc) BGZF_ATOMIC_OR(&w[pos], (uint32_t)acc); }
};

// Length-limited canonical Huffman code of hist[0 .. nsym): len[] (0 = unused) and the codes as the bit stream wants them (first bit lowest).
BGZF_FN void build_code(BlockLds &s, uint32_t *hist, uint32_t nsym, uint32_t maxbits, uint8_t *len, uint16_t *code, uint32_t tid0)
{
    BGZF_TID
    HuffScratch &h = s.u.hs;
    BGZF_PHASE
        if (tid == 0) {
            uint32_t used = 0;
            for (uint32_t i = 0; i < nsym; ++i) used += hist[i] != 0;
            // at least two codes, so that a lone symbol still costs one bit and the decoder sees a complete code (as zlib's build_tree does)
            for (uint32_t i = 0; used < 2; ++i) if (!hist[i]) { hist[i] = 1; ++used; }
            h.n_used = used;
            for (uint32_t i = 0; i < 16; ++i) h.bl_count[i] = 0;
        }
    BGZF_END
    BGZF_PHASE
        if (tid < nsym) {
            len[tid] = 0; code[tid] = 0;
            const uint32_t f = hist[tid];
            if (f) {
                uint32_t rank = 0;
                for (uint32_t t = 0; t < nsym; ++t) { const uint32_t g = hist[t]; rank += g && (g < f || (g == f && t < tid)); }
                h.sorted[rank] = (uint16_t)tid; h.nfreq[rank] = f;
            }
        }
    BGZF_END
    BGZF_PHASE
        if (tid == 0) {                                      // leaves 0 .. m - 1 in ascending count, inner nodes m .. 2m - 2 in the order made: both queues are sorted
            const uint32_t m = h.n_used;
            const uint32_t none = 0xFFFFFFFFu;               // (counts are at most BGZF_CUT + 1)
            uint32_t li = 0, ii = m, fl = h.nfreq[0], fi = none;      // heads of the two queues and their counts, kept in registers
            for (uint32_t nx = m; nx < 2 * m - 1; ++nx) {
                uint32_t sum = 0;
                for (int k = 0; k < 2; ++k) {
                    if (fl <= fi) { sum += fl; h.parent[li] = (uint16_t)nx; ++li; fl = li < m ? h.nfreq[li] : none; }
                    else {
                        sum += fi; h.parent[ii] = (uint16_t)nx; ++ii;
                        fi = ii < nx ? h.nfreq[ii] : none;
                    }
                }
                h.nfreq[nx] = sum;
                if (fi == none && ii == nx) fi = sum;         // the node just made is the inner queue's head
            }
        }
    BGZF_END
    BGZF_PHASE
        if (tid < h.n_used) {
            const uint32_t root = 2 * h.n_used - 2;
            uint32_t d = 0;
            for (uint32_t x = tid; x != root; x = h.parent[x]) ++d;
            BGZF_ATOMIC_ADD(&h.bl_count[d < maxbits ? d : maxbits], 1u);
        }
    BGZF_END
    BGZF_PHASE
        if (tid == 0) {
            // codes deeper than maxbits were counted at maxbits: while the Kraft sum is over, one code of the last level pairs up with a
            // code moved one level down from the deepest level above that has one (every step takes exactly one unit off the sum)
            uint32_t total = 0;
            for (uint32_t i = 1; i <= maxbits; ++i) total += h.bl_count[i] << (maxbits - i);
            while (total > (1u << maxbits)) {
                --h.bl_count[maxbits];
                for (uint32_t i = maxbits - 1; i >= 1; --i) if (h.bl_count[i]) { --h.bl_count[i]; h.bl_count[i + 1] += 2; break; }
                --total;
            }
            uint32_t c = 0, r = 0;
            h.bl_count[0] = 0;
            for (uint32_t b = 1; b <= maxbits; ++b) { c = (c + h.bl_count[b - 1]) << 1; h.next_code[b] = c; }
            for (uint32_t b = maxbits; b >= 1; --b) { h.first_rank[b] = r; r += h.bl_count[b]; }      // the rarest symbols get the longest codes
            h.first_rank[0] = r;
        }
    BGZF_END
    BGZF_PHASE
        if (tid < h.n_used) {
            uint32_t b = maxbits;
            while (b > 1 && tid >= h.first_rank[b] + h.bl_count[b]) --b;
            len[h.sorted[tid]] = (uint8_t)b;
        }
    BGZF_END
    BGZF_PHASE
        if (tid < nsym && len[tid]) {
            const uint32_t b = len[tid];
            uint32_t c = h.next_code[b];
            for (uint32_t t = 0; t < tid; ++t) c += len[t] == b;
            uint32_t rev = 0;
            for (uint32_t i = 0; i < b; ++i) rev |= ((c >> i) & 1u) << (b - 1 - i);
            code[tid] = (uint16_t)rev;
        }
    BGZF_END
}

// One block: text[0 .. n), 1 <= n <= BGZF_CUT (readable up to the next multiple of 4), into slot[0 .. BGZF_SLOT / 4) words; *size = its bytes.
BGZF_FN void deflate_block(BlockLds &s, const uint8_t *text, uint32_t n, uint32_t *slot, uint32_t *size, uint32_t tid0)
{
    BGZF_TID
    const uint8_t *tx = reinterpret_cast<const uint8_t *>(s.text32);
    uint8_t *slot8 = reinterpret_cast<uint8_t *>(slot);
    const uint32_t n_full = n / BGZF_CSEG;                    // whole CRC pieces

    // ---- stage ----
    BGZF_PHASE
        for (uint32_t w = tid; w < (BGZF_CUT + 16) / 4; w += BGZF_THREADS) {
            uint32_t v = 0;
            if (4 * w < n) { v = load32u(text + 4 * w); if (4 * w + 4 > n) v &= (1u << (8 * (n - 4 * w))) - 1u; }
            s.text32[w] = v;
        }
        for (uint32_t i = tid; i < (1u << BGZF_HBITS); i += BGZF_THREADS) s.u.htab[i] = 0;
        for (uint32_t i = tid; i < 4 * 256; i += BGZF_THREADS) s.crc_tab[i >> 8][i & 255] = k_crc.tab[i >> 8][i & 255];
        for (uint32_t i = tid; i < BGZF_CRC_LEVELS * 32; i += BGZF_THREADS) s.crc_mat[i >> 5][i & 31] = k_crc.mat[i >> 5][i & 31];
        for (uint32_t i = tid; i < 288; i += BGZF_THREADS) s.hist_ll[i] = i == 256 ? 1u : 0u;       // the end-of-block symbol
        if (tid < 32) s.hist_d[tid] = 0;
        if (tid < 20) s.hist_cl[tid] = 0;
        if (tid == 0) s.hdr_sym_bits = 0;
    BGZF_END

    // ---- CRC-32 ----
    BGZF_PHASE
        if (tid < n_full) {                                  // piece tid; stored by its distance from the last whole piece
            uint32_t c = tid == 0 ? 0xFFFFFFFFu : 0u;
            for (uint32_t w = 0; w < BGZF_CSEG / 4; ++w) {
                c ^= s.text32[tid * (BGZF_CSEG / 4) + w];
                c = s.crc_tab[3][c & 0xff] ^ s.crc_tab[2][(c >> 8) & 0xff] ^ s.crc_tab[1][(c >> 16) & 0xff] ^ s.crc_tab[0][c >> 24];
            }
            s.lane_a[n_full - 1 - tid] = c;
        }
    BGZF_END
    {
        uint32_t count = n_full, level = 0;
        uint32_t *a = s.lane_a, *b = s.lane_b;
        while (count > 1) {                                  // entry e must still advance e pieces of this level: the odd ones advance one piece and join the even ones
            const uint32_t half = (count + 1) / 2;
            BGZF_PHASE
                if (tid < half) {
                    uint32_t v = a[2 * tid];
                    if (2 * tid + 1 < count) {
                        const uint32_t x = a[2 * tid + 1]; uint32_t r = 0;
                        for (uint32_t i = 0; i < 32; ++i) r ^= ((x >> i) & 1u) ? s.crc_mat[level][i] : 0u;
                        v ^= r;
                    }
                    b[tid] = v;
                }
            BGZF_END
            uint32_t *t = a; a = b; b = t;
            count = half; ++level;
        }
        BGZF_PHASE
            if (tid == 0) {
                uint32_t c = n_full ? a[0] : 0xFFFFFFFFu;
                for (uint32_t i = n_full * BGZF_CSEG; i < n; ++i) c = s.crc_tab[0][(c ^ tx[i]) & 0xff] ^ (c >> 8);
                s.crc = ~c;
            }
        BGZF_END
    }

    // ---- match: candidates ----
    for (uint32_t base = 0; base < n; base += BGZF_THREADS) {
        BGZF_PHASE
            const uint32_t p = base + tid;
            if (p < n) {
                uint32_t dist = 0;
                if (p + BGZF_MIN_MATCH <= n) {
                    const uint32_t c = s.u.htab[(load32u(tx + p) * 2654435761u) >> (32 - BGZF_HBITS)];
                    if (c) dist = p + 1 - c;
                }
                s.v.mdist[p] = (uint16_t)dist;
            }
        BGZF_END
        BGZF_PHASE
            const uint32_t p = base + tid;
            if (p + BGZF_MIN_MATCH <= n) BGZF_ATOMIC_MAX(&s.u.htab[(load32u(tx + p) * 2654435761u) >> (32 - BGZF_HBITS)], p + 1);
        BGZF_END
    }

    // ---- parse: histograms ----
    BGZF_PHASE
        if (tid < BGZF_NSEG)
            parse_segment(s, tid, n,
                [&](uint32_t b) { BGZF_ATOMIC_ADD(&s.hist_ll[b], 1u); },
                [&](uint32_t len, uint32_t dist) {
                    uint32_t sym, eb, ev;
                    len_symbol(len, sym, eb, ev); BGZF_ATOMIC_ADD(&s.hist_ll[sym], 1u);
                    dist_symbol(dist, sym, eb, ev); BGZF_ATOMIC_ADD(&s.hist_d[sym], 1u);
                });
    BGZF_END

    // ---- codes ----
    build_code(s, s.hist_ll, BGZF_NLL, 15, s.len_ll, s.code_ll, tid0);
    build_code(s, s.hist_d, BGZF_ND, 15, s.len_d, s.code_d, tid0);
    BGZF_PHASE
        if (tid == 0) {
            uint32_t hl = BGZF_NLL, hd = BGZF_ND;
            while (hl > 257 && !s.len_ll[hl - 1]) --hl;
            while (hd > 1 && !s.len_d[hd - 1]) --hd;
            s.hlit = hl; s.hdist = hd;
        }
    BGZF_END
    BGZF_PHASE                                               // the code lengths go out one by one (no repeat codes 16 - 18)
        if (tid < s.hlit + s.hdist) BGZF_ATOMIC_ADD(&s.hist_cl[tid < s.hlit ? s.len_ll[tid] : s.len_d[tid - s.hlit]], 1u);
    BGZF_END
    build_code(s, s.hist_cl, BGZF_NCL, 7, s.len_cl, s.code_cl, tid0);

    // ---- bit counts ----
    BGZF_PHASE
        if (tid < s.hlit + s.hdist) {
            const uint32_t hb = s.len_cl[tid < s.hlit ? s.len_ll[tid] : s.len_d[tid - s.hlit]];
            s.hdr_len[tid] = (uint8_t)hb;
            BGZF_ATOMIC_ADD(&s.hdr_sym_bits, hb);
        }
        uint32_t bits = 0;
        if (tid < BGZF_NSEG)
            walk_segment(s, tid, n,
                [&](uint32_t b) { bits += s.len_ll[b]; },
                [&](uint32_t len, uint32_t dist) {
                    uint32_t sym, eb, ev;
                    len_symbol(len, sym, eb, ev); bits += s.len_ll[sym] + eb;
                    dist_symbol(dist, sym, eb, ev); bits += s.len_d[sym] + eb;
                });
        s.lane_a[tid] = bits;
    BGZF_END
    BGZF_PHASE                                               // prefix sums in two levels: inside groups of 16 (one thread per group) ...
        if (tid < 32) {
            uint32_t sum = 0;
            for (uint32_t l = 16 * tid; l < 16 * tid + 16 && l < BGZF_NSEG; ++l) { s.lane_b[l] = sum; sum += s.lane_a[l]; }
            s.grp[tid] = sum;
        } else if (tid >= 64 && tid < 96) {                  // (another wave than the lanes' groups)
            const uint32_t g = tid - 64;
            uint32_t sum = 0;
            for (uint32_t i = 16 * g; i < 16 * g + 16 && i < s.hlit + s.hdist; ++i) { s.hdr_off[i] = (uint16_t)sum; sum += s.hdr_len[i]; }
            s.hgrp[g] = sum;
        }
    BGZF_END
    BGZF_PHASE                                               // ... and over the groups
        if (tid == 0) {
            uint32_t hc = BGZF_NCL;
            while (hc > 4 && !s.len_cl[k_cl_order[hc - 1]]) --hc;
            s.hclen = hc;
            s.hdr_bits = 3 + 5 + 5 + 4 + 3 * hc + s.hdr_sym_bits;
            uint32_t sum = 0;
            for (uint32_t g = 0; g < 32; ++g) { const uint32_t v = s.grp[g]; s.grp[g] = sum; sum += v; }
            s.sym_bits = sum;
            const uint32_t bytes = (s.hdr_bits + sum + s.len_ll[256] + 7) / 8;
            s.stored = bytes >= n;                           // not smaller than the text: stored, 5 bytes of block header in front
            s.payload_bytes = s.stored ? n + 5 : bytes;
            s.block_size = 18 + s.payload_bytes + 8;
            *size = s.block_size;
        }
        if (tid == 64) {
            uint32_t sum = 0;
            for (uint32_t g = 0; g < 32; ++g) { const uint32_t v = s.hgrp[g]; s.hgrp[g] = sum; sum += v; }
        }
    BGZF_END
    BGZF_PHASE                                               // (the candidates' distances are no longer needed: the image takes their place)
        for (uint32_t w = tid; w < (s.block_size + 3) / 4; w += BGZF_THREADS) s.v.out[w] = 0;
    BGZF_END

    // ---- emit ----
    BGZF_PHASE
        const uint32_t bsize = s.block_size - 1;
        if (s.stored) {
            for (uint32_t i = tid; i < n; i += BGZF_THREADS) slot8[23 + i] = tx[i];
            if (tid == BGZF_THREADS - 1) {
                const uint8_t hd[23] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8),
                                         1, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)(~n >> 8) };
                for (uint32_t i = 0; i < 23; ++i) slot8[i] = hd[i];
                uint8_t *t = slot8 + 23 + n;
                for (uint32_t i = 0; i < 4; ++i) { t[i] = (uint8_t)(s.crc >> (8 * i)); t[4 + i] = (uint8_t)(n >> (8 * i)); }
            }
        } else {
            const uint32_t body = 18 * 8 + s.hdr_bits;
            uint32_t *const img = s.v.out;
            BitWriter bw;
            if (tid < BGZF_NSEG) {
                bw.open(img, body + s.grp[tid >> 4] + s.lane_b[tid]);
                walk_segment(s, tid, n,
                    [&](uint32_t b) { bw.put(s.code_ll[b], s.len_ll[b]); },
                    [&](uint32_t len, uint32_t dist) {
                        uint32_t sym, eb, ev;
                        len_symbol(len, sym, eb, ev); bw.put(s.code_ll[sym], s.len_ll[sym]); if (eb) bw.put(ev, eb);
                        dist_symbol(dist, sym, eb, ev); bw.put(s.code_d[sym], s.len_d[sym]); if (eb) bw.put(ev, eb);
                    });
                bw.close();
            }
            if (tid < s.hlit + s.hdist) {                    // the block header's code lengths, one per thread
                const uint32_t l = tid < s.hlit ? s.len_ll[tid] : s.len_d[tid - s.hlit];
                bw.open(img, 18 * 8 + 17 + 3 * s.hclen + s.hgrp[tid >> 4] + s.hdr_off[tid]);
                bw.put(s.code_cl[l], s.len_cl[l]);
                bw.close();
            }
            if (tid == BGZF_THREADS - 1) {                   // the member's header and the fixed part of the deflate block's
                bw.open(img, 0);
                bw.put(0x04088b1fu, 32); bw.put(0, 32); bw.put(0x0006ff00u, 32); bw.put(0x00024342u, 32); bw.put(bsize, 16);
                bw.put(1, 1); bw.put(2, 2); bw.put(s.hlit - 257, 5); bw.put(s.hdist - 1, 5); bw.put(s.hclen - 4, 4);
                for (uint32_t i = 0; i < s.hclen; ++i) bw.put(s.len_cl[k_cl_order[i]], 3);
                bw.close();
            } else if (tid == BGZF_THREADS - 2) {            // end of block, then the trailer on the next byte boundary
                bw.open(img, body + s.sym_bits);
                bw.put(s.code_ll[256], s.len_ll[256]);
                bw.close();
                bw.open(img, (18 + s.payload_bytes) * 8);
                bw.put(s.crc, 32); bw.put(n, 32);
                bw.close();
            }
        }
    BGZF_END
    BGZF_PHASE
        if (!s.stored) for (uint32_t w = tid; w < (s.block_size + 3) / 4; w += BGZF_THREADS) slot[w] = s.v.out[w];
    BGZF_END
}

} // namespace bgzf
} // namespace salt
#endif
