// salt_amd/csrc/salt_errprof.hip -- mismatches by cycle, quality and substitution, SNP sites masked (salt --error-profile).
//
// k_errprof runs behind the kernels that finish a batch's result rows.  It is a histogram of one event per aligned base (about 10^8 a
// step) over a few hundred hot cells, so nothing of it is a global atomic per base:
//   - a workgroup of EP_THREADS lanes owns a chunk of EP_THREADS reads of ONE mate, a lane a read; the lane loads its row head once (24 bytes
//     of the row, two offsets, on the text path the record's quality offset) and keeps it in registers over all tiles;
//   - the cycles are gone over in tiles of EP_TILE = 16: the workgroup's LDS table holds [16 cycles][95 q][4 ref][4 read] uint32 counts
//     (97 KB; a cycle's row is padded by one word so that the 16 rows start in 16 different banks).  Per tile a lane takes its 16 bases and
//     16 quality bytes in one or two 16-byte loads each (the aligned 16-byte pieces that hold a byte of the read's own: no byte of another
//     allocation is touched), fetched one tile ahead, and the three words of mixRef behind them, and adds 1 to one LDS cell per event.
//     Lane l starts at cycle l mod 16 of the tile: 64 reads that agree in q, ref and read spread over 16 addresses.  The stagger is a
//     rotation of the lane's three operands, once a tile, so that the sixteen events are taken at constant bit positions;
//   - behind every tile the workgroup sweeps its table (16-byte LDS reads), sends every non-zero cell as ONE 64-bit global atomic of
//     count * delta and zeroes it.  A cell grows by at most 1 per read and tile, so it never passes EP_THREADS: the uint32 partial counts
//     cannot overflow, whatever the batch size.
// Global atomics of a launch: workgroups * tiles * non-zero cells of the tile, + 7 per workgroup for R.
// A tile is counted in segments that lie inside one M run, where g is linear in the cycle: one segment for a row with one M op; any
// other row (0.3 % of the reads) walks its CIGAR and takes one more segment for every run that begins inside the tile.
// Bounds: a cycle is below min(L, 512), L from the offsets; the quality bytes are read only when qual_off + L lies inside the text block;
// a mixRef word only when it is one of the (ref_len + 7) / 8 words, and a position only below ref_len.  A row the align kernels got wrong
// cannot make this kernel fault.
#include <hip/hip_runtime.h>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_tally.h"

namespace salt {

static constexpr uint32_t EP_THREADS = SALT_EP_CHUNK, EP_TILE = 16, EP_ROW = SALT_ERRPROF_Q * 16 + 1, EP_WORDS = EP_TILE * EP_ROW;
static_assert(EP_WORDS % 4 == 0, "the sweep reads four cells at a time");
static_assert(EP_WORDS * 4 + 64 <= 160 * 1024, "one table per CU");

__device__ __forceinline__ uint32_t ep_sel4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t k) { return k & 2u ? (k & 1u ? a3 : a2) : (k & 1u ? a1 : a0); }

// 16 bytes at p, of which the first nb (1 .. 16) are the caller's: only the aligned 16-byte pieces that hold one of them are loaded
__device__ __forceinline__ void ep_fetch(const uint8_t *p, uint32_t nb, uint4 &A, uint4 &B)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t sh = (uint32_t)(a & 15u);
    A = *reinterpret_cast<const uint4 *>(a - sh);
    B = make_uint4(0, 0, 0, 0);
    if (sh + nb > 16u) B = *reinterpret_cast<const uint4 *>(a - sh + 16);
}
// those 16 bytes as four words, rotated right by r bytes on the way: byte e of out = byte (e + r) & 15 of the 16 (sh = p & 15)
__device__ __forceinline__ void ep_align_rot(const uint4 &A, const uint4 &B, uint32_t sh, uint32_t r, uint32_t out[4])
{
    const uint32_t ws = sh >> 2, bs = (sh & 3u) * 8u;
    const uint32_t x0 = ep_sel4(A.x, A.y, A.z, A.w, ws), x1 = ep_sel4(A.y, A.z, A.w, B.x, ws), x2 = ep_sel4(A.z, A.w, B.x, B.y, ws),
                   x3 = ep_sel4(A.w, B.x, B.y, B.z, ws), x4 = ep_sel4(B.x, B.y, B.z, B.w, ws);
    const uint32_t b0 = __funnelshift_r(x0, x1, bs), b1 = __funnelshift_r(x1, x2, bs), b2 = __funnelshift_r(x2, x3, bs), b3 = __funnelshift_r(x3, x4, bs);
    const uint32_t wr = r >> 2, br = (r & 3u) * 8u;
    const uint32_t y0 = ep_sel4(b0, b1, b2, b3, wr), y1 = ep_sel4(b1, b2, b3, b0, wr), y2 = ep_sel4(b2, b3, b0, b1, wr), y3 = ep_sel4(b3, b0, b1, b2, wr);
    out[0] = __funnelshift_r(y0, y1, br); out[1] = __funnelshift_r(y1, y2, br); out[2] = __funnelshift_r(y2, y3, br); out[3] = __funnelshift_r(y3, y0, br);
}

__global__ void __launch_bounds__(EP_THREADS) k_errprof(ErrProf c)
{
    __shared__ __attribute__((aligned(16))) uint32_t tab[EP_WORDS];
    __shared__ uint32_t rcnt[8];
    __shared__ uint32_t max_l;
    const uint32_t tid = threadIdx.x, r = tid & (EP_TILE - 1);                         // r: the cycle of a tile this lane starts at
    const uint32_t mate = c.pe ? blockIdx.x & 1u : 0u, chunk = c.pe ? blockIdx.x >> 1 : blockIdx.x;
    const uint64_t k = (uint64_t)chunk * EP_THREADS + tid;                             // the lane's read among the mate's reads
    const uint64_t i = c.pe ? 2 * k + mate : k;
    for (uint32_t x = tid; x < EP_WORDS; x += EP_THREADS) tab[x] = 0;
    if (tid < 8) rcnt[tid] = 0;
    if (tid == 8) max_l = 0;
    __syncthreads();

    // ---- the row head, once ----
    uint32_t L = 0, pos = 0, s_lead = 0, m_len = 0, n_ops = 0;
    bool rev = false, slow = false, have_q = false;
    const uint8_t *sq = nullptr, *qp = nullptr;
    const salt_result_t *row = nullptr;
    if (i < c.n_rec) {
        row = c.res + i;
        const TallyRow h = tally_row(row, c.pe, c.min_mapq);
        atomicAdd(&rcnt[0], 1u);
        if (h.fate != TALLY_COUNTED) atomicAdd(&rcnt[h.fate], 1u);                     // R 1 .. 3: skipped, unmapped, below the floor
        else {
            const uint32_t o0 = c.offs[i], l_read = c.offs[i + 1] - o0;
            L = l_read < SALT_MAX_READ_LEN ? l_read : SALT_MAX_READ_LEN;
            pos = h.pos; rev = h.rev;
            sq = c.seqs + o0;
            s_lead = h.s_lead; n_ops = h.n_ops;
            bool gapped = c.pe && (s_lead != 0u || h.seq_end != l_read - 1u);      // the soft clips the SAM / BAM writers print
            const uint32_t op0 = n_ops ? row->cigar[0] : 0u;
            if (n_ops == 1u && (op0 & 3u) == 0u) m_len = op0 >> 4;
            else {
                slow = true;
                for (uint32_t j = 0; j < n_ops; ++j) { const uint32_t what = row->cigar[j] & 3u; gapped |= what == 1u || what == 2u; }
            }
            if (c.quals) {
                const uint64_t qo = c.rec ? c.rec[i].qual_off : o0;
                if (qo <= c.q_bytes && l_read <= c.q_bytes - qo) { have_q = true; qp = c.quals + qo; }
            }
            atomicAdd(&rcnt[4], 1u);
            if (rev) atomicAdd(&rcnt[5], 1u);
            if (gapped) atomicAdd(&rcnt[6], 1u);
            atomicMax(&max_l, L);
        }
    }
    __syncthreads();
    const uint32_t n_tiles = (max_l + EP_TILE - 1) / EP_TILE;
    const int64_t n_words = (int64_t)(((uint64_t)c.ref_len + 7) / 8);
    const uint32_t sh_b = (uint32_t)(reinterpret_cast<uintptr_t>(sq) & 15u), sh_q = (uint32_t)(reinterpret_cast<uintptr_t>(qp) & 15u);      // (16 divides a tile: the same in every tile)

    // the first tile's bases and qualities; every tile fetches the next one's before it counts its own
    uint4 bA = make_uint4(0, 0, 0, 0), bB = bA, qA = bA, qB = bA;
    if (L) { ep_fetch(sq, L < EP_TILE ? L : EP_TILE, bA, bB); if (have_q) ep_fetch(qp, L < EP_TILE ? L : EP_TILE, qA, qB); }

    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t c0 = t * EP_TILE;
        if (c0 < L) {
            const uint32_t nb = L - c0 < EP_TILE ? L - c0 : EP_TILE;
            uint4 nbA = make_uint4(0, 0, 0, 0), nbB = nbA, nqA = nbA, nqB = nbA;
            if (c0 + EP_TILE < L) {
                const uint32_t nn = L - c0 - EP_TILE < EP_TILE ? L - c0 - EP_TILE : EP_TILE;
                ep_fetch(sq + c0 + EP_TILE, nn, nbA, nbB);
                if (have_q) ep_fetch(qp + c0 + EP_TILE, nn, nqA, nqB);
            }
            uint32_t bw[4], qw[4] = { 0, 0, 0, 0 };                                     // element e of both = cycle c0 + ((e + r) & 15); no qualities: bytes 0, q = none
            ep_align_rot(bA, bB, sh_b, r, bw);
            if (have_q) ep_align_rot(qA, qB, sh_q, r, qw);
            // The tile's cycles are the SEQ window [s_lo, s_lo + 16) (cycle c0 + j is s_lo + j forward, s_lo + 15 - j reverse), of which
            // [ts_lo, ts_hi) belongs to the read.  It is gone over in segments, each inside one M run, where the genome position is linear in
            // s: one segment for a row with one M op, one more per run that begins inside the tile for the others.
            const int32_t s_lo = rev ? (int32_t)L - 1 - (int32_t)(c0 + EP_TILE - 1) : (int32_t)c0;
            const int32_t ts_lo = rev ? (int32_t)L - (int32_t)c0 - (int32_t)nb : (int32_t)c0, ts_hi = ts_lo + (int32_t)nb;
            uint32_t op_i = 0, sp = s_lead; uint64_t gg = pos;                         // the CIGAR walk of a row that needs one
            int32_t cur = ts_lo;
            while (cur < ts_hi) {
                int32_t run_lo, run_hi; uint64_t run_g;
                if (!slow) { run_lo = (int32_t)s_lead; run_hi = (int32_t)(s_lead + m_len); run_g = pos; }
                else {                                                                 // the first M run that ends behind cur
                    bool found = false; uint32_t len = 0;
                    while (op_i < n_ops) {
                        const uint32_t op = row->cigar[op_i], what = op & 3u; len = op >> 4;
                        if (what == 0u) { if ((int32_t)(sp + len) > cur) { found = true; break; } sp += len; gg += len; }
                        else if (what == 1u) sp += len;
                        else if (what == 2u) gg += len;
                        ++op_i;
                    }
                    if (!found) break;
                    run_lo = (int32_t)sp; run_hi = (int32_t)(sp + len); run_g = gg;
                    sp += len; gg += len; ++op_i;                                      // (the walk stands behind the run)
                }
                const int32_t seg_lo = cur > run_lo ? cur : run_lo, seg_hi = ts_hi < run_hi ? ts_hi : run_hi;
                cur = slow ? run_hi : ts_hi;                                           // a row with one M op is done after this pass
                if (seg_lo >= seg_hi) continue;
                // window offset d = s - s_lo lies at genome position g_base + d; the segment is d in [d_lo, d_hi), cut to [0, ref_len)
                const int64_t g_base = (int64_t)run_g + ((int64_t)seg_lo - run_lo) - ((int64_t)seg_lo - s_lo);
                int64_t d_lo = seg_lo - s_lo, d_hi = seg_hi - s_lo;
                if (-g_base > d_lo) d_lo = -g_base;
                if ((int64_t)c.ref_len - g_base < d_hi) d_hi = (int64_t)c.ref_len - g_base;
                if (d_lo >= d_hi) continue;
                const int64_t w_base = g_base >> 3;                                    // (floor, also below 0)
                uint32_t rw[3] = { 0, 0, 0 };
                for (int x = 0; x < 3; ++x) { const int64_t w = w_base + x; if (w >= 0 && w < n_words) rw[x] = c.ref[w]; }
                const uint32_t shm = (uint32_t)(g_base & 7) * 4u;
                unsigned long long mk = (rw[0] | (unsigned long long)rw[1] << 32) >> shm;
                if (shm) mk |= (unsigned long long)rw[2] << (64u - shm);
                const unsigned long long below_hi = d_hi >= 16 ? ~0ull : (1ull << (4u * (uint32_t)d_hi)) - 1ull;
                mk &= below_hi & ~((1ull << (4u * (uint32_t)d_lo)) - 1ull);
                if (rev) mk = __brevll(mk);                                            // nibble d -> nibble 15 - d = the cycle, bit c -> bit 3 - c = the complement
                // nibble e = cycle (e + r) & 15, like the bases
                const uint32_t m0 = (uint32_t)mk, m1 = (uint32_t)(mk >> 32), y0 = r & 8u ? m1 : m0, y1 = r & 8u ? m0 : m1, bm = (r & 7u) * 4u;
                const uint32_t mw[2] = { __funnelshift_r(y0, y1, bm), __funnelshift_r(y1, y0, bm) };
#pragma unroll
                for (uint32_t e = 0; e < EP_TILE; ++e) {
                    const uint32_t m = (mw[e >> 3] >> (4u * (e & 7u))) & 15u;
                    const uint32_t rd = (bw[e >> 2] >> (8u * (e & 3u))) & 0xFFu;
                    if (((0x116u >> m) & 1u) == 0u || rd > 3u) continue;               // no position of the segment, N of the genome, a site; a read's N
                    const uint32_t rf = (m >> 1) - (m >> 3);                           // 1 2 4 8 -> 0 1 2 3
                    const uint32_t qb = (qw[e >> 2] >> (8u * (e & 3u))) & 0xFFu, q = qb - 33u < SALT_ERRPROF_Q - 1u ? qb - 33u : SALT_ERRPROF_Q - 1u;
                    const uint32_t j = (e + r) & (EP_TILE - 1);
                    atomicAdd(&tab[j * EP_ROW + q * 16u + rf * 4u + rd], 1u);
                }
            }
            bA = nbA; bB = nbB; qA = nqA; qB = nqB;
        }
        __syncthreads();
        // ---- the tile's non-zero cells leave; the table is zero again ----
        for (uint32_t x = tid * 4u; x < EP_WORDS; x += EP_THREADS * 4u) {
            const uint4 v = *reinterpret_cast<const uint4 *>(&tab[x]);
            if ((v.x | v.y | v.z | v.w) == 0u) continue;
            const uint32_t vv[4] = { v.x, v.y, v.z, v.w };
            for (uint32_t e = 0; e < 4; ++e) {
                if (!vv[e]) continue;
                const uint32_t y = x + e, j = y / EP_ROW, rr = y - j * EP_ROW;         // (rr == EP_ROW - 1: the pad word, never counted into)
                const uint32_t cell = ((mate * SALT_MAX_READ_LEN + c0 + j) * SALT_ERRPROF_Q + (rr >> 4)) * 16u + (rr & 15u);
                atomicAdd(c.cells + cell, (unsigned long long)vv[e] * c.delta);
            }
            *reinterpret_cast<uint4 *>(&tab[x]) = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();
    }
    if (tid < 7 && rcnt[tid]) atomicAdd(c.cells + SALT_ERRPROF_CELLS + mate * 8u + tid, (unsigned long long)rcnt[tid] * c.delta);
}

hipError_t launch_errprof(const ErrProf &c, hipStream_t st)
{
    if (c.n_rec == 0) return hipSuccess;
    const uint64_t per_mate = c.pe ? ((uint64_t)c.n_rec + 1) / 2 : c.n_rec;
    const uint64_t chunks = (per_mate + EP_THREADS - 1) / EP_THREADS;
    hipLaunchKernelGGL(k_errprof, dim3((uint32_t)(c.pe ? 2 * chunks : chunks)), dim3(EP_THREADS), 0, st, c);
    return hipGetLastError();
}

} // namespace salt
