// salt_amd/csrc/salt_tally.h -- what the row tallies share on the device (k_snp_count, k_depth_mark, k_errprof; DESIGN.md, in front of 4.6).
//
// A tally is a per-index table that every align call adds into behind the kernels that finish a batch's result rows.  Its kernel reads a
// row's head the way the SAM / BAM writers lay the record out; that decode is here once.
//
// The CIGAR op is `word & 3`: 0 M, 1 I, 2 D.  Nothing else is ever written into cigar[]: lv_cigar (k_heavy's gapped hits, k_cigar) writes
// M runs and `a == 'I' ? 1 : 2`; tb_walk (the Smith-Waterman traceback, whose words k_pe_final copies) writes 0, 1 and 2; k_pe_final's
// ungapped mates and the light kernels write `L << 4 | 0`.  So `& 3` and `& 15` agree on every row; `& 3` is what the SAM and BAM writers
// print, and a 3 (which they would print as '?') moves neither in the read nor in the genome.
#pragma once
#include <hip/hip_runtime.h>
#include "salt_device.h"

namespace salt {

// blocks of 256 threads for a grid-stride loop over n items
static inline uint32_t tally_grid(uint64_t n) { uint64_t b = (n + 255) / 256; if (b > (1u << 16)) b = 1u << 16; return b ? (uint32_t)b : 1u; }

enum TallyFate : uint32_t { TALLY_COUNTED, TALLY_SKIPPED, TALLY_UNMAPPED, TALLY_BELOW };      // in this order of precedence (R of the error profile)

struct TallyRow {
    uint32_t pos, mapq, s_lead, seq_end, n_ops;      // s_lead: the leading soft clip of a paired-end row (0 single end); n_ops <= SALT_MAX_CIGAR_OPS
    bool rev;                                        // printed reverse-complemented: paired end iff strand == 1, single end iff strand != 0
    TallyFate fate;
};

// Two loads: the row's first 16 bytes and the 8 bytes behind them.
__device__ __forceinline__ TallyRow tally_row(const salt_result_t *q, int pe, uint32_t min_mapq)
{
    const uint4 h0 = *reinterpret_cast<const uint4 *>(q);                          // pos | strand n_diff is_gap mapq | b0 | b1
    const uint2 h1 = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint8_t *>(q) + 16);      // seq_start seq_end | n_hits[2] n_cigar skipped
    const uint32_t strand = h0.y & 0xFFu, n_cigar = (h1.y >> 16) & 0xFFu, skipped = h1.y >> 24;
    TallyRow r;
    r.pos = h0.x; r.mapq = h0.y >> 24;
    r.rev = pe ? strand == 1u : strand != 0u;
    r.s_lead = pe ? (h1.x & 0xFFFFu) : 0u; r.seq_end = h1.x >> 16;
    r.n_ops = n_cigar < SALT_MAX_CIGAR_OPS ? n_cigar : SALT_MAX_CIGAR_OPS;
    r.fate = skipped ? TALLY_SKIPPED : r.pos == 0xFFFFFFFFu ? TALLY_UNMAPPED : r.mapq < min_mapq ? TALLY_BELOW : TALLY_COUNTED;
    return r;
}

// f(g, s, len) for every M run of the row: genome positions [g, g + len), bases [s, s + len) of SEQ as printed.  The CIGAR words are loaded
// one at a time (most rows have one).
template <class F> __device__ __forceinline__ void tally_m_runs(const salt_result_t *q, const TallyRow &r, F f)
{
    uint64_t g = r.pos;
    uint32_t s = r.s_lead;
    for (uint32_t k = 0; k < r.n_ops; ++k) {
        const uint32_t op = q->cigar[k], len = op >> 4, what = op & 3u;
        if (what == 1u) { s += len; continue; }
        if (what == 2u) { g += len; continue; }
        if (what != 0u) continue;
        f(g, s, len);
        g += len; s += len;
    }
}

// The same walk for a tally that also reads the gaps (k_indel_add): fm(g, s, len) for every M run as above, and fgap(what, len, g, s, prev,
// next) for every I (what 1) and D (what 2) op met at genome position g and base s of SEQ as printed, with the CIGAR words of the ops in
// front of it and behind it; TALLY_NO_OP where the row has none (its `& 3` is 3: no M).
static constexpr uint32_t TALLY_NO_OP = 0xFFFFFFFFu;
template <class FM, class FG> __device__ __forceinline__ void tally_ops(const salt_result_t *q, const TallyRow &r, FM fm, FG fgap)
{
    uint64_t g = r.pos;
    uint32_t s = r.s_lead, prev = TALLY_NO_OP, op = r.n_ops ? q->cigar[0] : TALLY_NO_OP;
    for (uint32_t k = 0; k < r.n_ops; ++k) {
        const uint32_t next = k + 1 < r.n_ops ? q->cigar[k + 1] : TALLY_NO_OP, len = op >> 4, what = op & 3u;
        if (what == 0u) { fm(g, s, len); g += len; s += len; }
        else if (what != 3u) {
            fgap(what, len, g, s, prev, next);
            if (what == 1u) s += len; else g += len;
        }
        prev = op; op = next;
    }
}

// An M run [g, g + len) into a difference array of ref_len + 1 words (DESIGN.md 4.7's rule; k_depth_mark and k_disc_add): delta at g, taken
// again at the run's end, the run cut at the genome's end.  Returns that end (<= g: nothing of the run lies in the genome, nothing marked).
__device__ __forceinline__ uint64_t tally_diff_mark(uint32_t *diff, uint32_t ref_len, uint64_t g, uint32_t len, uint32_t delta)
{
    const uint64_t end = g + len < ref_len ? g + len : (uint64_t)ref_len;
    if (g < end) { atomicAdd(diff + g, delta); atomicAdd(diff + end, 0u - delta); }
    return end;
}

} // namespace salt
