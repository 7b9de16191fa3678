// salt_amd/csrc/salt_inflate_block.h -- one BGZF member (RFC 1952 header with the 'BC' extra field, an RFC 1951 payload of any number of
// stored / fixed / dynamic blocks, CRC-32 and ISIZE) inflated by one workgroup, compressed bytes and text both held in LDS.
// k_bgzf_inflate (salt_inflate.hip) is the caller; the deflate side's header (salt_bgzf_block.h) gives the CRC tables and the phase macros.
//
// As there, the member's work is a fixed list of PHASES: every phase is entered by all threads, on the device it ends in __syncthreads(),
// and no barrier or cross-lane operation sits inside divergent control flow -- the only loop around phases (the CRC tree) has a constant
// trip count.  Compiled without hipcc the same source runs the phases one thread after the other (tools/inflate_model.cc,
// tests/test_inflate_model.py): the bounds rules below are proven there, under AddressSanitizer, before the kernel sees a damaged file.
//
//   stage      the member's bytes -> LDS (global reads stay inside the member; the words behind it read 0), the CRC tables -> LDS
//   decode     ONE lane: header, then block after block.  A deflate stream is serial -- where a symbol starts is known only when the one
//              before it has been decoded -- so the other lanes wait at the barrier.  Bits come from LDS through a 64-bit window, symbols
//              from a table of the code's first 10 (distances: 8) bits, longer codes from the canonical counts; matches copy inside the
//              text in LDS, which is why a distance can never reach a neighbour's bytes
//   crc        as the deflate side: 128-byte pieces, four bytes a step, combined by the tabulated "advance by 128 * 2^k bytes" operators
//   check      CRC-32 and ISIZE against the trailer and against the bytes produced; the member's status word
//   copy-out   only a good member: text -> its [uoff[b], uoff[b + 1]) of the output, whole words where the output is aligned
//
// What damaged input can do: nothing but set a status.  Every read of the compressed bytes is an LDS read at an index bounded by the
// member's size + 16 (the array is larger and zero behind the member); every write of text is checked against the member's text size, which
// is at most INFL_MAX; every loop iteration consumes at least one input bit or writes at least one output byte, and running out of either
// ends the decode with a reason.  No trap, no assert, no loop that waits for data to become good.
#ifndef SALT_INFLATE_BLOCK_H
#define SALT_INFLATE_BLOCK_H
#include "salt_bgzf_block.h"

namespace salt {
namespace bgzf {

constexpr uint32_t INFL_MAX = 65536;                         // most text in a member (ISIZE) and most bytes of a member (BSIZE + 1)
constexpr uint32_t INFL_THREADS = BGZF_THREADS;              // the phase macros count this many threads
constexpr uint32_t INFL_NCSEG = INFL_MAX / BGZF_CSEG;        // 512 CRC pieces at most: nine tree levels
constexpr uint32_t INFL_CRC_LEVELS = 9;
constexpr uint32_t INFL_LL_BITS = 10, INFL_D_BITS = 8, INFL_CL_BITS = 7;      // bits looked up at once
static_assert(INFL_NCSEG <= INFL_THREADS && (1u << INFL_CRC_LEVELS) >= INFL_NCSEG, "one CRC piece per thread");

// a member's status word: 0 = its text is in place, else why it is not (nothing of it has been written then)
enum : uint32_t {
    INFL_OK = 0, INFL_E_SIZE, INFL_E_HEADER, INFL_E_BSIZE, INFL_E_BTYPE, INFL_E_STORED, INFL_E_HLIT, INFL_E_CL_CODE, INFL_E_CL_REPEAT,
    INFL_E_LL_CODE, INFL_E_D_CODE, INFL_E_NO_EOB, INFL_E_SYMBOL, INFL_E_DISTANCE, INFL_E_OUTPUT, INFL_E_INPUT, INFL_E_ISIZE, INFL_E_CRC, INFL_N_REASONS
};
static inline const char *inflate_reason(uint32_t r)
{
    static const char *const text[INFL_N_REASONS] = {
        "ok", "member or text larger than 64 KiB (or no room for header and trailer)", "not a gzip header with the BC extra field", "BSIZE does not match the member's bytes",
        "reserved block type", "stored block whose LEN and NLEN disagree or which passes the payload's end", "more than 286 literal/length or 30 distance codes",
        "code-length code over-subscribed or incomplete", "bad repeat in the code lengths", "literal/length code over-subscribed or incomplete",
        "distance code over-subscribed or incomplete", "no end-of-block code", "bit pattern that is no code, or an invalid symbol", "distance reaches in front of the block's first byte",
        "more text than ISIZE", "payload ends inside a block", "ISIZE differs from the bytes produced", "CRC-32 mismatch" };
    return r < INFL_N_REASONS ? text[r] : "unknown";
}

// RFC 1951 3.2.5: base and extra bits of the length symbols 257 .. 285 and of the distance symbols
BGZF_CONST const uint16_t k_len_base[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258 };
BGZF_CONST const uint8_t k_len_extra[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0 };
BGZF_CONST const uint16_t k_dist_base[30] = { 1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577 };
BGZF_CONST const uint8_t k_dist_extra[30] = { 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13 };

struct InflCode {                                            // one canonical code
    uint16_t count[16];                                      // codes of each length
    uint16_t sym[288];                                       // symbols in code order
    uint16_t fast[1u << INFL_LL_BITS];                       // low bits of the window -> symbol << 4 | length, 0 = longer than the table (or no code)
    uint32_t offs[16], next[16];                             // while it is built: per length, where its next symbol goes and its next code
};

struct InflateLds {
    uint32_t out32[INFL_MAX / 4];                            // the text
    uint32_t in32[INFL_MAX / 4 + 8];                         // the member; zero behind it
    InflCode ll, d;                                          // (the code-length code lies in d until the lengths are read)
    uint8_t  lens[320];
    uint32_t crc_tab[4][256], crc_mat[BGZF_CRC_LEVELS][32];
    uint32_t lane_a[INFL_THREADS], lane_b[INFL_THREADS];
    uint32_t status, produced, crc;
};
static_assert(sizeof(InflateLds) <= 160 * 1024, "one CU's LDS");

// The stream's next bits, lowest first.  `ip` counts the payload bytes taken into the window, so 8 * (ip - lo) - nb bits have been consumed;
// the window may run up to 8 bytes past the payload (into the trailer and the zeros behind it, all in LDS): over() says so before anything
// is made of such bits.
struct InflBits {
    const uint32_t *w; uint64_t acc; uint32_t nb, ip, lo, hi;
    BGZF_MFN void open(const uint32_t *words, uint32_t from, uint32_t to) { w = words; acc = 0; nb = 0; ip = lo = from; hi = to; }
    BGZF_MFN uint32_t word_at(uint32_t byte) const
    {
        const uint32_t i = byte >> 2, sh = (byte & 3) * 8;
        const uint32_t a = w[i], b = w[i + 1];
        return sh ? (a >> sh) | (b << (32 - sh)) : a;
    }
    BGZF_MFN void fill() { if (nb <= 32) { acc |= (uint64_t)word_at(ip) << nb; nb += 32; ip += 4; } }      // at least 32 bits afterwards
    BGZF_MFN uint32_t peek(uint32_t n) const { return (uint32_t)acc & ((1u << n) - 1u); }
    BGZF_MFN void drop(uint32_t n) { acc >>= n; nb -= n; }
    BGZF_MFN uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
    BGZF_MFN bool over() const { return 8u * (ip - lo) - nb > 8u * (hi - lo); }
    BGZF_MFN uint32_t to_byte() { drop(nb & 7); ip -= nb >> 3; acc = 0; nb = 0; return ip; }             // the next whole byte; the window is emptied
};

// lens[0 .. n) -> code.  0 = usable; 1 = over-subscribed; 2 = incomplete (the caller knows which incomplete codes RFC 1951 allows).
BGZF_FN uint32_t infl_build(InflCode &c, const uint8_t *lens, uint32_t n, uint32_t fast_bits)
{
    uint32_t *const offs = c.offs, *const next = c.next;
    for (uint32_t l = 0; l < 16; ++l) c.count[l] = 0;
    for (uint32_t i = 0; i < n; ++i) ++c.count[lens[i]];
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; ++l) { left = left * 2 - (int32_t)c.count[l]; if (left < 0) return 1; }
    offs[1] = 0; next[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) { offs[l + 1] = offs[l] + c.count[l]; next[l + 1] = (next[l] + c.count[l]) << 1; }
    for (uint32_t i = 0; i < (1u << fast_bits); ++i) c.fast[i] = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t l = lens[i];
        if (!l) continue;
        c.sym[offs[l]++] = (uint16_t)i;
        const uint32_t code = next[l]++;
        if (l <= fast_bits) {                                // the stream sends a code's first bit first: the table is indexed by the reversed code
            uint32_t rev = 0;
            for (uint32_t b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
            for (uint32_t k = rev; k < (1u << fast_bits); k += 1u << l) c.fast[k] = (uint16_t)(i << 4 | l);
        }
    }
    return left > 0 ? 2u : 0u;
}

// The next symbol (the window holds at least 15 bits), or 0xFFFF when the bits are no code of c.
BGZF_FN uint32_t infl_symbol(const InflCode &c, InflBits &br, uint32_t fast_bits)
{
    const uint32_t e = c.fast[br.peek(fast_bits)];
    if (e) { br.drop(e & 15); return e >> 4; }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        code |= ((uint32_t)(br.acc >> (l - 1))) & 1u;
        const uint32_t cnt = c.count[l];
        if (code < first + cnt) { br.drop(l); return c.sym[index + (code - first)]; }
        index += cnt; first = (first + cnt) << 1; code <<= 1;
    }
    return 0xFFFFu;
}

// The payload in[pay_lo .. pay_hi) -> out[0 .. usize) exactly; one thread.  Returns a reason; *produced = bytes written.
BGZF_FN uint32_t infl_payload(InflateLds &s, uint32_t pay_lo, uint32_t pay_hi, uint32_t usize, uint32_t *produced)
{
    uint8_t *out = reinterpret_cast<uint8_t *>(s.out32);
    const uint8_t *in = reinterpret_cast<const uint8_t *>(s.in32);
    InflBits br; br.open(s.in32, pay_lo, pay_hi);
    uint32_t op = 0, last = 0;
    *produced = 0;
    while (!last) {                                          // a block: its header alone is three bits of input
        br.fill();
        last = br.take(1);
        const uint32_t type = br.take(2);
        if (br.over()) return INFL_E_INPUT;
        if (type == 3) return INFL_E_BTYPE;
        if (type == 0) {
            br.drop(br.nb & 7); br.fill();
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (br.over()) return INFL_E_INPUT;
            if ((len ^ nlen) != 0xFFFFu) return INFL_E_STORED;
            uint32_t p = br.to_byte();
            if (len > pay_hi - p) return INFL_E_STORED;
            if (len > usize - op) return INFL_E_OUTPUT;
            const uint32_t end = op + len;
            while (op < end && (op & 3)) out[op++] = in[p++];
            for (; op + 4 <= end; op += 4, p += 4) s.out32[op >> 2] = br.word_at(p);
            while (op < end) out[op++] = in[p++];
            br.ip = p;
            continue;
        }
        if (type == 1) {
            for (uint32_t i = 0; i < 288; ++i) s.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
            infl_build(s.ll, s.lens, 288, INFL_LL_BITS);
            for (uint32_t i = 0; i < 32; ++i) s.lens[i] = 5;
            infl_build(s.d, s.lens, 32, INFL_D_BITS);         // (symbols 286, 287 and 30, 31 have codes; using one is the error)
        } else {
            const uint32_t hlit = br.take(5) + 257, hdist = br.take(5) + 1, hclen = br.take(4) + 4;
            if (br.over()) return INFL_E_INPUT;
            if (hlit > BGZF_NLL || hdist > BGZF_ND) return INFL_E_HLIT;
            for (uint32_t i = 0; i < BGZF_NCL; ++i) s.lens[i] = 0;
            for (uint32_t i = 0; i < hclen; ++i) { br.fill(); s.lens[k_cl_order[i]] = (uint8_t)br.take(3); }
            if (br.over()) return INFL_E_INPUT;
            if (infl_build(s.d, s.lens, BGZF_NCL, INFL_CL_BITS)) return INFL_E_CL_CODE;
            uint32_t n = 0;
            while (n < hlit + hdist) {                       // a code-length symbol: at least one bit of input
                br.fill();
                const uint32_t sym = infl_symbol(s.d, br, INFL_CL_BITS);
                if (sym == 0xFFFFu) return br.over() ? INFL_E_INPUT : INFL_E_SYMBOL;
                uint32_t rep = 1, val = sym;
                if (sym == 16) { if (n == 0) return INFL_E_CL_REPEAT; val = s.lens[n - 1]; rep = 3 + br.take(2); }
                else if (sym == 17) { val = 0; rep = 3 + br.take(3); }
                else if (sym == 18) { val = 0; rep = 11 + br.take(7); }
                if (br.over()) return INFL_E_INPUT;
                if (rep > hlit + hdist - n) return INFL_E_CL_REPEAT;
                while (rep--) s.lens[n++] = (uint8_t)val;
            }
            if (!s.lens[256]) return INFL_E_NO_EOB;
            if (infl_build(s.ll, s.lens, hlit, INFL_LL_BITS)) return INFL_E_LL_CODE;
            // the distance code may be incomplete in one way: a single code of one bit (RFC 1951 3.2.7); none at all means literals only
            const uint32_t rd = infl_build(s.d, s.lens + hlit, hdist, INFL_D_BITS);
            if (rd == 1 || (rd == 2 && s.d.count[0] + s.d.count[1] != hdist)) return INFL_E_D_CODE;
        }
        for (;;) {                                           // a symbol: at least one bit of input, or the decode ends
            br.fill();
            uint32_t sym = infl_symbol(s.ll, br, INFL_LL_BITS);
            if (sym < 256) {
                if (br.over()) return INFL_E_INPUT;
                if (op >= usize) return INFL_E_OUTPUT;
                out[op++] = (uint8_t)sym;
                continue;
            }
            if (sym == 256) { if (br.over()) return INFL_E_INPUT; break; }
            if (sym >= 286) return br.over() ? INFL_E_INPUT : INFL_E_SYMBOL;          // (0xFFFF: no code)
            sym -= 257;
            const uint32_t len = k_len_base[sym] + br.take(k_len_extra[sym]);
            br.fill();
            const uint32_t ds = infl_symbol(s.d, br, INFL_D_BITS);
            if (ds >= 30) return br.over() ? INFL_E_INPUT : INFL_E_SYMBOL;
            const uint32_t dist = k_dist_base[ds] + br.take(k_dist_extra[ds]);
            if (br.over()) return INFL_E_INPUT;
            if (dist > op) return INFL_E_DISTANCE;
            if (len > usize - op) return INFL_E_OUTPUT;
            for (uint32_t i = 0; i < len; ++i, ++op) out[op] = out[op - dist];         // byte after byte: a copy may overlap what it writes
        }
    }
    *produced = op;
    return INFL_OK;
}

// One member: member[0 .. csize) -> out[0 .. usize) (the member's range of the output), *status = 0 or the reason nothing was written.
BGZF_FN void inflate_block(InflateLds &s, const uint8_t *member, uint32_t csize, uint8_t *out, uint32_t usize, uint32_t *status, uint32_t tid0)
{
    BGZF_TID
    if (csize < 26 || csize > INFL_MAX || usize > INFL_MAX) {                            // (the same for every thread)
        BGZF_PHASE
            if (tid == 0) *status = INFL_E_SIZE;
        BGZF_END
        return;
    }
    const uint8_t *tx = reinterpret_cast<const uint8_t *>(s.out32);
    const uint8_t *in = reinterpret_cast<const uint8_t *>(s.in32);

    // ---- stage ----
    BGZF_PHASE
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(member) & 3u);
        for (uint32_t w = tid; w < INFL_MAX / 4 + 8; w += INFL_THREADS) {
            const uint32_t i = 4 * w;
            uint32_t v = 0;
            if (i >= mis && i - mis + 8 <= csize) {          // both aligned words around member[i .. i + 4) lie inside the member
                const uint8_t *p = member + i - mis;
                const uint32_t a = load32u(static_cast<const uint8_t *>(__builtin_assume_aligned(p, 4)));
                if (mis) { const uint32_t b = load32u(static_cast<const uint8_t *>(__builtin_assume_aligned(p + 4, 4))); v = (a >> (8 * mis)) | (b << (32 - 8 * mis)); }
                else v = a;
            } else
                for (uint32_t k = 0; k < 4 && i + k < csize; ++k) v |= (uint32_t)member[i + k] << (8 * k);
            s.in32[w] = v;
        }
        for (uint32_t i = tid; i < 4 * 256; i += INFL_THREADS) s.crc_tab[i >> 8][i & 255] = k_crc.tab[i >> 8][i & 255];
        for (uint32_t i = tid; i < BGZF_CRC_LEVELS * 32; i += INFL_THREADS) s.crc_mat[i >> 5][i & 31] = k_crc.mat[i >> 5][i & 31];
    BGZF_END

    // ---- decode ----
    BGZF_PHASE
        if (tid == 0) {
            uint32_t st = INFL_OK, produced = 0;
            const uint32_t xlen = (uint32_t)in[10] | (uint32_t)in[11] << 8;
            if (in[0] != 0x1f || in[1] != 0x8b || in[2] != 8 || in[3] != 4 || 12 + xlen + 8 > csize) st = INFL_E_HEADER;
            else {
                uint32_t bsize = 0;
                for (uint32_t p = 12; p + 4 <= 12 + xlen; ) {                            // extra subfields: SI1 SI2 SLEN data (at least 4 bytes a turn)
                    const uint32_t slen = (uint32_t)in[p + 2] | (uint32_t)in[p + 3] << 8;
                    if (in[p] == 'B' && in[p + 1] == 'C' && slen == 2 && p + 6 <= 12 + xlen) { bsize = ((uint32_t)in[p + 4] | (uint32_t)in[p + 5] << 8) + 1u; break; }
                    p += 4 + slen;
                }
                if (!bsize) st = INFL_E_HEADER;
                else if (bsize != csize) st = INFL_E_BSIZE;
                else st = infl_payload(s, 12 + xlen, csize - 8, usize, &produced);
            }
            if (st == INFL_OK) {
                const uint32_t isize = (uint32_t)in[csize - 4] | (uint32_t)in[csize - 3] << 8 | (uint32_t)in[csize - 2] << 16 | (uint32_t)in[csize - 1] << 24;
                if (isize != produced || produced != usize) st = INFL_E_ISIZE;
            }
            s.status = st; s.produced = st == INFL_OK ? produced : 0;
        }
    BGZF_END

    // ---- CRC-32 ----
    BGZF_PHASE
        const uint32_t n_full = s.produced / BGZF_CSEG;
        if (tid < n_full) {                                  // piece tid; stored by its distance from the last whole piece
            uint32_t c = tid == 0 ? 0xFFFFFFFFu : 0u;
            for (uint32_t w = 0; w < BGZF_CSEG / 4; ++w) {
                c ^= s.out32[tid * (BGZF_CSEG / 4) + w];
                c = s.crc_tab[3][c & 0xff] ^ s.crc_tab[2][(c >> 8) & 0xff] ^ s.crc_tab[1][(c >> 16) & 0xff] ^ s.crc_tab[0][c >> 24];
            }
            s.lane_a[n_full - 1 - tid] = c;
        }
    BGZF_END
    for (uint32_t level = 0; level < INFL_CRC_LEVELS; ++level) {                         // count entries -> (count + 1) / 2, nine times whatever the text's length
        BGZF_PHASE
            const uint32_t count = ((s.produced / BGZF_CSEG) + (1u << level) - 1u) >> level;
            const uint32_t *a = level & 1 ? s.lane_b : s.lane_a;
            uint32_t *b = level & 1 ? s.lane_a : s.lane_b;
            if (tid < (count + 1) / 2) {
                uint32_t v = a[2 * tid];
                if (2 * tid + 1 < count) {                   // entry 2 tid + 1 advances one piece of this level (the ninth level's piece is two of the eighth's)
                    uint32_t x = a[2 * tid + 1];
                    const uint32_t m = level < BGZF_CRC_LEVELS ? level : BGZF_CRC_LEVELS - 1;
                    for (uint32_t rep = 0; rep < (1u << (level - m)); ++rep) {
                        uint32_t r = 0;
                        for (uint32_t i = 0; i < 32; ++i) r ^= ((x >> i) & 1u) ? s.crc_mat[m][i] : 0u;
                        x = r;
                    }
                    v ^= x;
                }
                b[tid] = v;
            }
        BGZF_END
    }

    // ---- check ----
    BGZF_PHASE
        if (tid == 0) {
            const uint32_t n = s.produced, n_full = n / BGZF_CSEG;
            uint32_t c = n_full ? s.lane_b[0] : 0xFFFFFFFFu;                             // (nine levels: the last one wrote lane_b)
            for (uint32_t i = n_full * BGZF_CSEG; i < n; ++i) c = s.crc_tab[0][(c ^ tx[i]) & 0xff] ^ (c >> 8);
            const uint32_t want = (uint32_t)in[csize - 8] | (uint32_t)in[csize - 7] << 8 | (uint32_t)in[csize - 6] << 16 | (uint32_t)in[csize - 5] << 24;
            if (s.status == INFL_OK && ~c != want) s.status = INFL_E_CRC;
            *status = s.status;
        }
    BGZF_END

    // ---- copy-out ----
    BGZF_PHASE
        if (s.status == INFL_OK) {
            // bytes up to the output's next word boundary, whole output words (each from two words of the text), the bytes left
            uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 3u)) & 3u;
            if (head > usize) head = usize;
            const uint32_t n_words = (usize - head) / 4;
            if (tid < head) out[tid] = tx[tid];
            for (uint32_t w = tid; w < n_words; w += INFL_THREADS) {
                const uint32_t j = head + 4 * w, sh = (j & 3) * 8;
                const uint32_t a = s.out32[j >> 2];
                const uint32_t v = sh ? (a >> sh) | (s.out32[(j >> 2) + 1] << (32 - sh)) : a;
                memcpy(__builtin_assume_aligned(out + j, 4), &v, 4);
            }
            const uint32_t done = head + 4 * n_words;
            if (done + tid < usize) out[done + tid] = tx[done + tid];
        }
    BGZF_END
}

} // namespace bgzf
} // namespace salt
#endif
