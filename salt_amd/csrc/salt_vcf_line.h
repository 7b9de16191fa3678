// salt_amd/csrc/salt_vcf_line.h -- one VCF line under the rule of DESIGN.md 2.2, for the device's k_vcf_parse (salt_vcf.hip) and the host
// twin (salt_vcf_snps, host/salt_idx.cc): both compile this one function, as salt_bgzf_block.h is shared.  The independent statement of
// the rule is the Python model in tests/vcf_check.py.
//
// A line is t[b, e) without its '\n'.  The first condition that holds decides, in this order:
//   one trailing '\r' is dropped; empty or '#'            VCF_SKIP      (not counted as a line)
//   fewer than 5 TAB-separated fields, POS not 1-10 digits VCF_MALFORMED
//   CHROM not among the keys                               VCF_UNKNOWN
//   POS outside 1 .. contig length (64-bit, never wraps)   VCF_RANGE
//   REF not one byte of ACGTacgt; no contributing ALT      VCF_NOT_SNV
//   folded REF != folded genome base at POS (N: never)     VCF_REF
//   pass_only and FILTER (field 7) neither PASS nor .      VCF_FILTERED
//   else                                                   VCF_KEPT: *gpos = contig start + POS - 1, *mask = bit(REF) | bits(ALT)
// Nothing behind ALT is read (behind FILTER with pass_only); a long ALT is walked, never stored.
#ifndef SALT_VCF_LINE_H
#define SALT_VCF_LINE_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SALT_VCF_HD __host__ __device__ __forceinline__
#else
#define SALT_VCF_HD inline
#endif

namespace salt {

enum { VCF_SKIP = 0, VCF_KEPT = 1, VCF_UNKNOWN = 2, VCF_RANGE = 3, VCF_NOT_SNV = 4, VCF_REF = 5, VCF_FILTERED = 6, VCF_MALFORMED = 7 };

// The contig names a CHROM may carry (FASTA names and what the rename map sends to them) in an open-addressing table: slots[h] = key + 1, 0 = free,
// linear probing, at most half full (so a probe always ends).  Key k is names[key_off[k], key_off[k + 1]) and stands for contig key_contig[k].
struct VcfTable {
    const uint8_t  *names;
    const uint32_t *key_off;
    const int32_t  *key_contig;
    const uint32_t *slots;
    uint32_t        slot_mask;       // slots - 1, slots a power of two
    uint32_t        pass_only;
    const uint64_t *start;           // n_contigs + 1: offsets in the concatenated genome
    const uint8_t *const *seq;       // n_contigs: the base LETTERS of every contig, as the FASTA holds them
};

SALT_VCF_HD uint32_t vcf_hash(const uint8_t *s, uint64_t n)            // FNV-1a
{
    uint32_t h = 2166136261u;
    for (uint64_t i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
    return h;
}
SALT_VCF_HD uint32_t vcf_base(uint8_t c)
{
    c |= 0x20;
    return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : c == 't' ? 3u : 4u;
}
SALT_VCF_HD int32_t vcf_lookup(const VcfTable &T, const uint8_t *s, uint64_t n)
{
    for (uint32_t h = vcf_hash(s, n) & T.slot_mask;; h = (h + 1) & T.slot_mask) {
        const uint32_t v = T.slots[h];
        if (v == 0) return -1;
        const uint32_t o = T.key_off[v - 1];
        if ((uint64_t)(T.key_off[v] - o) != n) continue;
        uint64_t i = 0;
        while (i < n && T.names[o + i] == s[i]) ++i;
        if (i == n) return T.key_contig[v - 1];
    }
}

SALT_VCF_HD int vcf_line(const uint8_t *t, uint64_t b, uint64_t e, const VcfTable &T, uint64_t *gpos, uint32_t *mask)
{
    if (e > b && t[e - 1] == '\r') --e;
    if (e == b || t[b] == '#') return VCF_SKIP;
    uint64_t f[5];                                           // f[i]: start of field i; field i ends at f[i + 1] - 1
    uint64_t p = b;
    f[0] = b;
    for (int i = 1; i < 5; ++i) {
        while (p < e && t[p] != '\t') ++p;
        if (p == e) return VCF_MALFORMED;
        f[i] = ++p;
    }
    const uint64_t n_pos = f[2] - 1 - f[1];
    if (n_pos < 1 || n_pos > 10) return VCF_MALFORMED;
    uint64_t v = 0;
    for (uint64_t i = f[1]; i < f[2] - 1; ++i) {
        const uint32_t d = (uint32_t)t[i] - '0';
        if (d > 9) return VCF_MALFORMED;
        v = v * 10 + d;
    }
    const int32_t c = vcf_lookup(T, t + f[0], f[1] - 1 - f[0]);
    if (c < 0) return VCF_UNKNOWN;
    if (v < 1 || v > T.start[c + 1] - T.start[c]) return VCF_RANGE;
    if (f[4] - 1 - f[3] != 1) return VCF_NOT_SNV;
    const uint32_t r = vcf_base(t[f[3]]);
    if (r > 3) return VCF_NOT_SNV;
    uint32_t m = 0;
    p = f[4];
    for (;;) {                                               // the alleles of ALT, cut at commas
        uint64_t q = p;
        while (q < e && t[q] != ',' && t[q] != '\t') ++q;
        if (q - p == 1) { const uint32_t a = vcf_base(t[p]); if (a < 4 && a != r) m |= 1u << a; }
        p = q;
        if (p == e || t[p] == '\t') break;
        ++p;
    }
    if (m == 0) return VCF_NOT_SNV;
    const uint64_t g = T.start[c] + v - 1;
    if (vcf_base(T.seq[c][v - 1]) != r) return VCF_REF;
    if (T.pass_only && p < e) {                              // p: the TAB behind ALT.  QUAL, then FILTER; without a field 7 the line passes
        ++p;
        while (p < e && t[p] != '\t') ++p;
        if (p < e) {
            const uint64_t s = ++p;
            while (p < e && t[p] != '\t') ++p;
            const bool pass = (p - s == 1 && t[s] == '.') || (p - s == 4 && t[s] == 'P' && t[s + 1] == 'A' && t[s + 2] == 'S' && t[s + 3] == 'S');
            if (!pass) return VCF_FILTERED;
        }
    }
    *gpos = g;
    *mask = m | 1u << r;
    return VCF_KEPT;
}

} // namespace salt
#endif
