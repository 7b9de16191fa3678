// salt_amd/csrc/salt_stats.hip -- the run's summary: mapping counts, histograms and per-contig counts (salt --stats).
//
// k_stats_add runs behind the kernels that finish a batch's result rows, beside the other row tallies.  Every table but CT is hot: a
// lambda batch puts all its reads into a handful of cells.  So no cell receives a global atomic per record:
//   - a workgroup of ST_THREADS lanes owns a chunk of SALT_STATS_CHUNK records, a lane a record a round.  Its LDS holds the fixed tables
//     (SALT_STATS_CELLS cells) and the CT rows of the first SALT_STATS_CT_LDS contigs as uint32 partial counts: 6 536 words, 25.5 KB, so
//     that six workgroups fit the 160 KB of a CU and the loads of one hide behind those of the others;
//   - the eleven counters of SN that are predicates (cells 0 .. 10) are taken wave-wide: one ballot and one LDS atomic per wave, mate and
//     cell.  The sums and the histograms are one LDS atomic per event;
//   - behind its last round the workgroup sweeps the table (16-byte LDS reads) and sends every non-zero partial on as ONE 64-bit global
//     atomic of count * delta.  CT rows of contigs beyond SALT_STATS_CT_LDS go to global memory directly, one atomic per event.
// No 32-bit partial can overflow, whatever the batch size: a partial is a workgroup's, a workgroup owns SALT_STATS_CHUNK = 2 048 records
// however many the batch has, and one record adds to one partial at most the sum of its CIGAR lengths, 64 ops of at most 4 095 (SN 12, 14
// and CT 5; SN 11, 13 and 15 grow by up to 512 per record, every other partial by up to 64): 2 048 * 64 * 4 095 < 2^29.1.
// Per record a lane reads the row head (tally_row: 24 bytes), its two offsets, the first CIGAR word -- the other words only when the row
// is not one M op --, the hits only when the head lists some, the mate's head for a pair, and the read's bases for GC in the aligned
// 16-byte pieces that hold a byte of the read's own (no byte of another allocation is touched).
// Bounds: L from the offsets, capped at 512; a mate index that exists (i ^ 1 < n_rec); a contig from a search that cannot leave
// [0, n_contigs) (the SAM writer's, seq_id_dev); n_hits capped at 5 per strand, n_ops at 64, the clips at L; every table index is cut to
// its table.  A row the align kernels got wrong cannot make this kernel fault.
#include <hip/hip_runtime.h>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_tally.h"

namespace salt {

static constexpr uint32_t ST_THREADS = 256, ST_CT0 = SALT_STATS_CELLS, ST_USED = SALT_STATS_CELLS + SALT_STATS_CT_LDS * 8u, ST_WORDS = (ST_USED + 3u) & ~3u;
static_assert(SALT_STATS_CHUNK % ST_THREADS == 0 && ST_THREADS % 64 == 0, "whole rounds of whole waves, and an even chunk: a pair never straddles two workgroups' parities");
static_assert((uint64_t)SALT_STATS_CHUNK * SALT_MAX_CIGAR_OPS * 4095u < (1ull << 32), "a uint32 partial holds a chunk's largest sum");
static_assert(ST_WORDS * 4u * 2u <= 160u * 1024u, "more than one workgroup per CU");
static_assert(SALT_STATS_ID + 2u * 65u == SALT_STATS_CELLS, "the tables tile the cells");

// bns_coor_pac2real's search (bntseq.c:269-289), the one the SAM writer names a position's contig by: the result lies in [0, n - 1]
__device__ __forceinline__ uint32_t st_contig(const int64_t *c_off, int32_t n, int64_t coor)
{
    int left = 0, mid = 0, right = n;
    while (left < right) {
        mid = (left + right) >> 1;
        if (coor >= c_off[mid]) {
            if (mid == n - 1) break;
            if (coor < c_off[mid + 1]) break;
            left = mid + 1;
        } else right = mid;
    }
    return (uint32_t)mid;
}

// (gc, n) of the L codes at p: gc those that are 1 or 2, n those that are 0 .. 3; only the aligned 16-byte pieces that hold one of them are loaded
__device__ __forceinline__ void st_gc(const uint8_t *p, uint32_t L, uint32_t &gc, uint32_t &n)
{
    gc = 0; n = 0;
    if (!L) return;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t sh = (uint32_t)(a & 15u), end = sh + L;                             // the read is bytes [sh, end) of the pieces from a - sh on
    for (uint32_t b0 = 0; b0 < end; b0 += 16u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a - sh + b0);
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t lo = b0 + 4u * k;                                           // the word is bytes [lo, lo + 4)
            if (lo + 4u <= sh || lo >= end) continue;
            uint32_t own = 0x80808080u;                                                // bit 7 of every byte that is the read's
            if (lo < sh) own &= 0xFFFFFFFFu << (8u * (sh - lo));
            if (lo + 4u > end) own &= 0xFFFFFFFFu >> (8u * (lo + 4u - end));
            const uint32_t t = w[k] & 0xFCFCFCFCu;                                     // a byte of t is 0 iff the code is 0 .. 3
            const uint32_t acgt = ~(t | ((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & own;
            n += (uint32_t)__popc(acgt);
            gc += (uint32_t)__popc((((w[k] ^ (w[k] >> 1)) & 0x01010101u) << 7) & acgt);
        }
    }
}

// One record into the workgroup's table; returns its SN predicates, bit b = cell b (0 .. 10), which the caller counts wave-wide.
__device__ __forceinline__ uint32_t st_record(const StatsAdd &c, uint32_t *tab, uint64_t i, uint32_t mate)
{
    const salt_result_t *row = c.res + i;
    const TallyRow h = tally_row(row, c.pe, c.min_mapq);
    uint32_t bits = 1u;
    if (h.fate == TALLY_SKIPPED) return bits | 2u;
    const uint32_t o0 = c.offs[i], l_read = c.offs[i + 1] - o0, L = l_read < SALT_MAX_READ_LEN ? l_read : SALT_MAX_READ_LEN;
    uint32_t gc, n;
    st_gc(c.seqs + o0, L, gc, n);
    atomicAdd(&tab[SALT_STATS_RL + mate * 513u + L], 1u);
    atomicAdd(&tab[SALT_STATS_GC + mate * 102u + (n ? (200u * gc + n) / (2u * n) : 101u)], 1u);
    if (L) atomicAdd(&tab[SALT_STATS_SN + mate * 16u + 11u], L);
    if (h.fate == TALLY_UNMAPPED) return bits | 4u;

    // ---- mapped ----
    const uint32_t rid = st_contig(c.c_off, c.n_contigs, (int64_t)h.pos);
    auto ct_add = [&](uint32_t col, uint32_t v) {
        if (rid < SALT_STATS_CT_LDS) atomicAdd(&tab[ST_CT0 + rid * 8u + col], v);
        else atomicAdd(c.ct + (uint64_t)rid * 8u + col, (unsigned long long)v * c.delta);
    };
    atomicAdd(&tab[SALT_STATS_MQ + mate * 256u + (h.mapq & 255u)], 1u);
    ct_add(mate, 1u);
    if (h.fate == TALLY_BELOW) return bits | 8u;

    // ---- counted ----
    bits |= 16u;
    ct_add(2u + mate, 1u);
    if (h.rev) { bits |= 32u; ct_add(4u, 1u); }
    // the CIGAR: M columns cut at the genome's end as the coverage cuts them, I and D ops by length
    uint32_t m_cols = 0, n_i = 0, n_d = 0;
    {
        uint64_t g = h.pos;
        for (uint32_t k = 0; k < h.n_ops; ++k) {                                       // (one pass, one word, for a row of one M op)
            const uint32_t op = row->cigar[k], len = op >> 4, what = op & 3u;
            if (what == 0u) {
                const uint64_t end = g + len < c.ref_len ? g + len : (uint64_t)c.ref_len;
                if (g < end) m_cols += (uint32_t)(end - g);
                g += len;
            } else if (what == 1u) { n_i += len; atomicAdd(&tab[SALT_STATS_ID + (len < 64u ? len : 64u)], 1u); }
            else if (what == 2u) { n_d += len; g += len; atomicAdd(&tab[SALT_STATS_ID + 65u + (len < 64u ? len : 64u)], 1u); }
        }
    }
    uint32_t n_s = 0;                                                                  // the soft clips the SAM / BAM writers print
    if (c.pe) {
        const uint32_t lead = h.s_lead < L ? h.s_lead : L, trail = L && h.seq_end < L - 1u ? L - 1u - h.seq_end : 0u;
        n_s = lead + trail < L ? lead + trail : L;
    }
    if (m_cols) { atomicAdd(&tab[SALT_STATS_SN + mate * 16u + 12u], m_cols); ct_add(5u, m_cols); }
    if (n_i) atomicAdd(&tab[SALT_STATS_SN + mate * 16u + 13u], n_i);
    if (n_d) atomicAdd(&tab[SALT_STATS_SN + mate * 16u + 14u], n_d);
    if (n_s) atomicAdd(&tab[SALT_STATS_SN + mate * 16u + 15u], n_s);
    if (n_i | n_d | n_s) bits |= 64u;
    // the XA entries the writers print: every listed hit whose position is not the row's
    {
        const uint32_t nh0 = row->n_hits[0] < SALT_MAX_HITS ? row->n_hits[0] : SALT_MAX_HITS, nh1 = row->n_hits[1] < SALT_MAX_HITS ? row->n_hits[1] : SALT_MAX_HITS;
        uint32_t n_xa = 0;
        for (uint32_t k = 0; k < nh0; ++k) n_xa += row->hits[0][k].pos != h.pos;
        for (uint32_t k = 0; k < nh1; ++k) n_xa += row->hits[1][k].pos != h.pos;
        if (n_xa) bits |= 128u;
        atomicAdd(&tab[SALT_STATS_XA + mate * 8u + (n_xa < 7u ? n_xa : 7u)], 1u);
    }
    if (!c.pe) return bits;

    // ---- the pair: what alnpe_sam prints of the mate (sam.c:350-358; sam_head_pe, k_bam_write) ----
    const uint64_t j = i ^ 1ull;
    TallyRow ho{};
    bool map_ot = false;
    if (j < c.n_rec) { ho = tally_row(c.res + j, 1, 0u); map_ot = ho.pos != 0xFFFFFFFFu; }
    if (!map_ot) return bits | 512u;
    const uint32_t rid_ot = st_contig(c.c_off, c.n_contigs, (int64_t)ho.pos);
    if (rid_ot != rid) return bits | 1024u;
    const uint32_t pos_me = h.pos - (uint32_t)c.c_off[rid] + 1u, pos_ot = ho.pos - (uint32_t)c.c_off[rid] + 1u;
    // the template, on (mate 0, mate 1) whichever record this is; mate 1's seq_start stands in both arms, as in the reference
    const uint32_t p0 = mate ? pos_ot : pos_me, p1 = mate ? pos_me : pos_ot;
    const uint32_t se0 = mate ? ho.seq_end : h.seq_end, se1 = mate ? h.seq_end : ho.seq_end, ss1 = mate ? h.s_lead : ho.s_lead;
    const uint32_t t = p0 < p1 ? p1 + se1 - ss1 + 1u - p0 : p0 + se0 - ss1 + 1u - p1;
    const bool proper = t != 0u && t <= c.max_tlen && t >= c.min_tlen;
    if (proper) bits |= 256u;
    if (mate == 0u) {
        if (proper) atomicAdd(&tab[SALT_STATS_IS + (t < SALT_STATS_IS_MAX ? t : SALT_STATS_IS_MAX)], 1u);
        uint32_t o = 2u;
        if (h.rev != ho.rev) o = (h.rev ? pos_ot : pos_me) <= (h.rev ? pos_me : pos_ot) ? 0u : 1u;
        atomicAdd(&tab[SALT_STATS_OR + o], 1u);
    }
    return bits;
}

__global__ void __launch_bounds__(ST_THREADS) k_stats_add(StatsAdd c)
{
    __shared__ __attribute__((aligned(16))) uint32_t tab[ST_WORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t x = tid; x < ST_WORDS; x += ST_THREADS) tab[x] = 0;
    __syncthreads();
    // the chunk and the rounds are even: in a paired-end batch a lane's records are all of mate tid & 1
    const uint32_t mate = c.pe ? tid & 1u : 0u;
    const unsigned long long mates = c.pe ? (mate ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull) : ~0ull;      // the wave's lanes of this lane's mate
    const uint64_t base = (uint64_t)blockIdx.x * SALT_STATS_CHUNK;
    for (uint32_t r = 0; r < SALT_STATS_CHUNK / ST_THREADS; ++r) {
        const uint64_t i = base + (uint64_t)r * ST_THREADS + tid;
        uint32_t bits = 0;
        if (i < c.n_rec) bits = st_record(c, tab, i, mate);
        // SN 0 .. 10 wave-wide: the lowest lane of each mate adds its mate's count
#pragma unroll
        for (uint32_t b = 0; b < 11; ++b) {
            const unsigned long long m = __ballot((bits >> b) & 1u) & mates;
            if (lane == mate && m) atomicAdd(&tab[SALT_STATS_SN + mate * 16u + b], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    // ---- the non-zero partials leave ----
    for (uint32_t x = tid * 4u; x < ST_WORDS; x += ST_THREADS * 4u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&tab[x]);
        if ((v.x | v.y | v.z | v.w) == 0u) continue;
        const uint32_t vv[4] = { v.x, v.y, v.z, v.w };
        for (uint32_t e = 0; e < 4; ++e) {
            const uint32_t y = x + e;
            if (!vv[e] || y >= ST_USED) continue;
            if (y < ST_CT0) atomicAdd(c.cells + y, (unsigned long long)vv[e] * c.delta);
            else if ((y - ST_CT0) >> 3 < (uint32_t)c.n_contigs) atomicAdd(c.ct + (y - ST_CT0), (unsigned long long)vv[e] * c.delta);
        }
    }
}

hipError_t launch_stats_add(const StatsAdd &c, hipStream_t st)
{
    if (c.n_rec == 0) return hipSuccess;
    const uint32_t chunks = (uint32_t)(((uint64_t)c.n_rec + SALT_STATS_CHUNK - 1) / SALT_STATS_CHUNK);
    hipLaunchKernelGGL(k_stats_add, dim3(chunks), dim3(ST_THREADS), 0, st, c);
    return hipGetLastError();
}

} // namespace salt
