// tools/ctx_model.cc -- the context record (salt_amd/csrc/salt_ctx_record.h) on the host: builds the record of a suffix, the read's side
// of the comparison and the verdict of ctx_reject with the very functions the kernels use, for every seed offset of every window it is
// given.  tests/test_ctx_record_model.py sets the verdicts against the oracle's masked Hamming count of the whole window.
//
//   g++ -O2 -std=c++17 -Wall -Wextra -Werror [-DCTX_N_FRONT=.. -DCTX_A_SEEDS=.. -DCTX_A_EXTRA=.. -DCTX_NS_BITS_A=..] -o ctx_model tools/ctx_model.cc
//
// stdin:  u32 G, n_win, L, k;  G bytes genome codes 0..3;  G bytes allele masks (bit c: base c is listed);
//         n_win windows: u32 pos, L bytes read codes 0..3, 4 = N.  Every window lies inside the genome (pos + L <= G).
// stdout: first line "n_front a_start n_behind ns_bits_a"; then per window L - k + 1 bytes: byte `off` is 1 when the record of the
//         suffix at pos + off rejects the window for a seed at read offset off (bound 3), else 0.
// exit 2: a record's side B does not hold the genome in front of its suffix (what seed_resolve_unique relies on).
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../salt_amd/csrc/salt_ctx_record.h"

using namespace salt;

static bool get(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }

int main()
{
    uint32_t hd[4];
    if (!get(hd, sizeof hd)) return 1;
    const uint32_t G = hd[0], n_win = hd[1], L = hd[2], k = hd[3];
    std::vector<uint8_t> genome(G), mask(G), read(L);
    if (!get(genome.data(), G) || !get(mask.data(), G) || L < k) return 1;
    std::vector<uint32_t> text(G / 16 + 2, 0), ref(G / 8 + 2, 0);             // packed as the device image packs them
    for (uint32_t i = 0; i < G; ++i) {
        text[i >> 4] |= (uint32_t)(genome[i] & 3u) << (30 - 2 * (i & 15u));
        ref[i >> 3] |= (uint32_t)(mask[i] & 15u) << (4 * (i & 7u));
    }
    const uint32_t a_start = ctx_a_start(k);
    printf("%u %u %u %u\n", (unsigned)CTX_N_B, (unsigned)a_start, (unsigned)CTX_N_A, (unsigned)CTX_NS_BITS_A);
    std::vector<uint8_t> out(L - k + 1);
    for (uint32_t w = 0; w < n_win; ++w) {
        uint32_t pos;
        if (!get(&pos, 4) || !get(read.data(), L) || (uint64_t)pos + L > G) return 1;
        for (uint32_t off = 0; off + k <= L; ++off) {
            const uint64_t s = (uint64_t)pos + off;
            const CtxRec rec = ctx_build(text.data(), ref.data(), G, (uint32_t)s, s, a_start);
            if (s >= CTX_N_B && s <= G)
                for (uint32_t u = 0; u < CTX_N_B; ++u) {
                    const uint32_t b = ((ctx_front_lo(rec) >> u) & 1u) | (((ctx_front_hi(rec) >> u) & 1u) << 1);
                    if (b != genome[s - 1 - u]) return 2;
                }
            CtxRead rd = { 0, 0, 0 };
            for (uint32_t t = 0; t < 64; ++t) {                                // the device: one lane per plane bit, three ballots
                const int p = ctx_face(t, off, a_start);
                if (p < 0 || p >= (int)L) continue;
                const uint32_t nib = read[p] > 3 ? 15u : 1u << read[p];
                rd.lo |= (uint64_t)ctx_nib_lo(nib) << t; rd.hi |= (uint64_t)ctx_nib_hi(nib) << t; rd.use |= (uint64_t)ctx_nib_use(nib) << t;
            }
            out[off] = ctx_reject(rec, rd, 3u) ? 1 : 0;
        }
        fwrite(out.data(), 1, out.size(), stdout);
    }
    return 0;
}
