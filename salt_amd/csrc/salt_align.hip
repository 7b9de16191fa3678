// salt_amd/csrc/salt_align.hip -- per-batch kernels of the single-end alignment path (gfx950 only).
//
//   k_seed   one lane per (read, strand, seed slot): 12-mer tables + backward search on the C and R
//            FM-indexes + interval-shrinking left extension            (alnse_seed_overlap, alnse.c:199-312)
//   k_align  one 64-lane wave per read: order seeds (klib introsort), locate under the max_locate
//            cap, sort + dedup loci, masked-Hamming verify of all candidates in parallel with the
//            reference's sequential best/first-hit rule replayed by ballots, Landau-Vishkin on the
//            4-bit masks when nothing matched gap-free, hit selection, MAPQ, CIGAR
//            (alnse_locate_alt alnse.c:633-731, alnse_check_nogap :734-782, alnse_check_withgap
//             :871-901, alnse_overlap_alt :1045-1104, query_set_hits/gen_mapq/query_gen_cigar
//             query.c:270-333, LandauVishkin.c:19-122,176-470, editdistance.c:88-284)
//
// All arithmetic is integer; outputs are bit-exact with the reference CPU path.
#include <type_traits>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_sai_sort.h"

namespace salt {

// Every block is exactly one wave, and the LDS unit executes one wave's DS instructions in issue order, so
// lanes only need the COMPILER not to move LDS accesses across the hand-off point: a wavefront-scope
// fence + wave_barrier costs no instruction, where __syncthreads() costs s_waitcnt vmcnt(0) + s_barrier.
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                     __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); } while (0)

static constexpr int MAXL = SALT_MAX_READ_LEN;
static constexpr int SLOTS = SALT_MAX_SEED_SLOTS;
static constexpr int MAXLOC = SALT_MAX_LOCATE;
static constexpr int LVK = 31;                  // MAX_K (LandauVishkin.c:13)
// k_light writes the first 24 bytes of a result row as six dwords
static_assert(offsetof(salt_result_t, strand) == 4 && offsetof(salt_result_t, mapq) == 7 && offsetof(salt_result_t, b0) == 8 &&
              offsetof(salt_result_t, b1) == 12 && offsetof(salt_result_t, seq_start) == 16 && offsetof(salt_result_t, seq_end) == 18 &&
              offsetof(salt_result_t, n_hits) == 20 && offsetof(salt_result_t, n_cigar) == 22 && offsetof(salt_result_t, skipped) == 23 &&
              offsetof(salt_result_t, hits) == 24 && sizeof(salt_hit_t) == 8, "salt_result_t header layout");
static constexpr int NHIT = 6;                  // first hits kept per strand (5 + the primary)
// gen_mapq's quotient 255 * x / b0 (query.c:270-281; x = |b0 - b1| <= 100000, so the product fits 32 bits).  b0 <= 3 whenever the
// best hit is gap-free: constant divisors there instead of a runtime division (a 64-bit one costs ~100 instructions per read).
__device__ __forceinline__ uint32_t mapq_quot(uint32_t x, uint32_t b0)
{
    const uint32_t v = 255u * x;
    return b0 == 1u ? v : b0 == 2u ? v / 2u : b0 == 3u ? v / 3u : v / b0;
}
static constexpr uint32_t INF = 255;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// Pointers that reach a non-inlined device function lose their address space (flat_load + coupled
// vmcnt/lgkmcnt waits); these casts state that they point to global memory.
typedef const uint32_t __attribute__((address_space(1))) *gp_u32;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef const u32x4_t __attribute__((address_space(1))) *gp_u32x4;
__device__ __forceinline__ gp_u32 as_global(const uint32_t *p) { return (gp_u32)p; }
__device__ __forceinline__ gp_u32x4 as_global(const uint4 *p) { return (gp_u32x4)(const void *)p; }
// ... and these that they point into the block's LDS (ds_read, lgkmcnt alone)
typedef const uint32_t __attribute__((address_space(3))) *lds_u32;
__device__ __forceinline__ lds_u32 as_lds(const uint32_t *p) { return (lds_u32)p; }

// diagnostic phase clock: adds the cycles since the previous stamp to ctr[slot] (lane 0, only when counting)
struct PhaseClock {                    // acc: a per-wave LDS array (flushed once per wave), or nullptr
    unsigned long long *acc; uint64_t t;
    __device__ PhaseClock(unsigned long long *a) : acc(a), t(a ? __builtin_amdgcn_s_memtime() : 0) {}
    __device__ __forceinline__ void stamp(int slot)
    {
        if (!acc) return;
        uint64_t n = __builtin_amdgcn_s_memtime();
        if (lane_id() == 0) acc[slot] += (unsigned long long)(n - t);
        t = n;
    }
    __device__ __forceinline__ void add(int slot, unsigned long long v) { if (acc && lane_id() == 0) acc[slot] += v; }
};

__device__ __forceinline__ uint32_t read_base(const uint8_t *seq, uint32_t L, int strand, uint32_t i)
{
    if (strand == 0) return seq[i];
    uint32_t c = seq[L - 1 - i];
    return c < 4 ? 3 - c : c;                    // query_seq_reverse (query.c:46-71)
}

// ---------------------------------------------------------------------------------------------
// k_pack: the batch's reads in the two packed, fixed-stride forms the other kernels gather from (PackGeom,
// salt_kernels.h).  A block is nw32 x rpb threads (rpb = 256 / nw32, at most 64): thread (j, rr) owns bases 32 j .. 32 j + 31 of
// BOTH strands of read r0 + rr, so the mapping needs no division.  Three steps, each between two barriers:
//   1. stage: the read's bytes come from global memory as aligned 16-byte units, a row of LDS per read that keeps the read's
//      byte offset inside its first unit.  On the way every byte is folded to a nibble: codes 0 .. 3 stay, anything above has
//      bit 2 or bit 3 set (N; nst_nt4_table's "codes > 4 read as N", query.c:177-183).
//   2. pack: one body for both strands.  A chunk is nine aligned LDS words and eight v_perm_b32, which take the 32 bases from any
//      byte offset and, for strand 1, from the read's other end with the bytes of a word reversed (query_seq_reverse,
//      query.c:46-71); the complement is one XOR on the code bits, N keeps its flag bits.  From there both strands run the same
//      shift-and-mask steps under the same "base exists" masks (base i of either strand exists when i < L).
//   3. store: the words go to an image of the block's records in LDS (over the staged bytes) and leave as 16-byte stores; a
//      record's last unit is written word by word up to its L word, so the words behind it stay untouched.
// ---------------------------------------------------------------------------------------------
// words of a read's row of staged bytes: 32 bytes in front (strand 1 of a short read starts before the read), the units of
// 8 nw8 bytes at any offset in the first unit; odd, so that the rows of neighbouring reads start on different LDS banks
__host__ __device__ __forceinline__ uint32_t pack_row_words(const PackGeom &pg) { return (8u + 4u * ((8u * pg.nw8 + 30u) >> 4)) | 1u; }
__host__ __device__ __forceinline__ uint32_t pack_reads_per_block(const PackGeom &pg) { return 256u / pg.nw32 < 64u ? 256u / pg.nw32 : 64u; }
// CORRECTNESS RESTS ON THE MASKS V (pack_chunk): step 2 reads LDS that step 1 never wrote -- the 32 bytes in front of a row, the
// units behind a read's last one, and the ninth word of a row's last chunk, which lies in the next row (or in the 16 spare
// words behind the last row).  Every such byte stands at a base place i >= L of its strand, and places without a base follow
// the places with one in both strands, so a stray high nibble can only spill into another masked place (e0 / e1 in pack_chunk).
// Whoever changes V, the chunk size or the row layout has to keep that true.
// LDS words of a block: the staged rows (+ 16: the ninth word of a chunk that starts in a row's last unit) or the image of the
// records; at most 16 384 bytes (121 .. 128 bases: 64 reads x (36 + 28) words), so eight blocks a CU take 133 of the 160 KB
__host__ __device__ __forceinline__ uint32_t pack_lds_words(const PackGeom &pg)
{
    const uint32_t rpb = pack_reads_per_block(pg), a = rpb * pack_row_words(pg) + 16u, b = rpb * (pg.pm_stride + pg.tb_stride);
    return a > b ? a : b;
}
__device__ __forceinline__ uint32_t pk_fold(uint32_t x) { return (x | (x >> 2) | (x >> 4)) & 0x0F0F0F0Fu; }   // byte -> nibble: code, or bit 2 / 3 set

// the words of one strand's 32 bases: 4 one-hot words, 2 words of 2-bit codes, 1 word of N flags
struct PackChunk { uint32_t pm[4], t2[2], nf; };

// w[0 .. 8]: the aligned LDS words around the chunk's 32 bytes, sh: the first byte's place in w[0]; REV: the bytes are the strand's
// bases from the last to the first, to be complemented.  V[h]: 15 in every nibble of one-hot word h whose base exists.
template <bool REV>
__device__ __forceinline__ PackChunk pack_chunk(const uint32_t (&w)[9], uint32_t sh, const uint32_t (&V)[4])
{
    const uint32_t sel = (REV ? 0x00010203u : 0x03020100u) + sh * 0x01010101u, one = 0x11111111u;
    PackChunk c;
    uint32_t p16[4], nb = 0;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        // bases 8 h .. 8 h + 7 of the chunk as two words of four folded bytes, first base lowest
        const uint32_t d0 = REV ? __builtin_amdgcn_perm(w[8 - 2 * h], w[7 - 2 * h], sel) : __builtin_amdgcn_perm(w[2 * h + 1], w[2 * h], sel);
        const uint32_t d1 = REV ? __builtin_amdgcn_perm(w[7 - 2 * h], w[6 - 2 * h], sel) : __builtin_amdgcn_perm(w[2 * h + 2], w[2 * h + 1], sel);
        const uint32_t e0 = d0 | (d0 >> 4), e1 = d1 | (d1 >> 4);                               // bytes 0 and 2: two nibbles each
        uint32_t n8 = __builtin_amdgcn_perm(e1, e0, 0x06040200u);                              // base q of the word in nibble q
        if (REV) n8 ^= 0x33333333u;                                                            // A <-> T, C <-> G; N keeps bit 2 / 3
        n8 &= V[h];
        const uint32_t isn = ((n8 >> 2) | (n8 >> 3)) & one, n3 = isn | (isn << 1), n15 = n3 | (n3 << 2);    // shifts: a multiply by 15 issues at a quarter of the rate
        const uint32_t a = n8 & one, b = (n8 >> 1) & one, p = a + one, bm = b | (b << 1), t = p & bm;   // p: 1 << (code & 1)
        c.pm[h] = (((p ^ t) | (t << 2)) | n15) & V[h];                                         // 1 << code; N -> 15, no base -> 0 (nt2bit, editdistance.c:40)
        uint32_t q = n8 & 0x33333333u & ~n15;                                                  // 2-bit codes (N and 'no base' read 0)
        q = (q | (q >> 2)) & 0x0F0F0F0Fu; p16[h] = q | (q >> 4);                               // bytes 0 and 2: four codes each
        uint32_t u = isn;
        u = (u | (u >> 3)) & 0x03030303u; u = (u | (u >> 6)) & 0x000F000Fu; u = (u | (u >> 12)) & 0xFFu;
        nb |= u << (8 * h);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const uint32_t rv = __brev(__builtin_amdgcn_perm(p16[2 * g + 1], p16[2 * g], 0x06040200u));   // first base highest; then put each pair back in order
        c.t2[g] = ((rv & 0x55555555u) << 1) | ((rv >> 1) & 0x55555555u);
    }
    c.nf = __brev(nb);
    return c;
}

__global__ void __launch_bounds__(256)
k_pack(PackGeom pg, uint32_t n_reads, const uint8_t *__restrict__ seqs, const uint32_t *__restrict__ offs,
       uint32_t *__restrict__ pm, uint32_t *__restrict__ tb)
{
    extern __shared__ uint4 pk_lds4[];                                      // pack_lds_words(pg) words
    uint32_t *const lds = reinterpret_cast<uint32_t *>(pk_lds4);
    __shared__ uint32_t so[65];
    const uint32_t tpr = blockDim.x, rpb = blockDim.y, j = threadIdx.x, rr = threadIdx.y;      // threads per read (nw32), reads per block
    const uint32_t r0 = blockIdx.x * rpb, nr = n_reads - r0 < rpb ? n_reads - r0 : rpb;
    {   // nr + 1 <= 65 offsets; a block has at least 64 threads
        const uint32_t t = __umul24(rr, tpr) + j, nt = __umul24(tpr, rpb);
        if (t <= nr) so[t] = offs[r0 + t];
        if (t + nt <= nr) so[t + nt] = offs[r0 + t + nt];
    }
    const uint32_t cap = 8 * pg.nw8, rw = pack_row_words(pg);               // bases the records hold per strand
    const uint64_t total_bases = offs[n_reads];                             // end of the valid bytes of seqs[]
    __syncthreads();
    const bool live = rr < nr;
    uint32_t L = 0, mis = 0;
    // ---- 1. the read's bytes as aligned 16-byte units, folded, into its row ----
    if (live) {
        L = so[rr + 1] - so[rr];
        if (L > cap) L = cap;                                               // longer than max_read_len says: truncated, never out of bounds
        const uintptr_t a = (uintptr_t)seqs + so[rr], lo = (uintptr_t)seqs, hi = (uintptr_t)seqs + total_bases;
        mis = (uint32_t)(a & 15u);
        // Only units that hold a byte of the read are asked for, and of those only units that overlap [seqs, seqs + total_bases): an
        // aligned 16-byte unit that overlaps the valid bytes lies inside their allocation granule, so the bytes of it that are not
        // ours can be read; they are never used (the masks V below).  A unit wholly outside reads as 0.
        const uint32_t nu = L ? (mis + L + 15u) >> 4 : 0u;
        uint32_t *row = lds + __umul24(rr, rw) + 8u;
        for (uint32_t u = j; u < nu; u += tpr) {
            const uintptr_t ad = a - mis + 16u * u;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (ad + 16u > lo && ad < hi) v = *reinterpret_cast<const uint4 *>(ad);
            row[4 * u] = pk_fold(v.x); row[4 * u + 1] = pk_fold(v.y); row[4 * u + 2] = pk_fold(v.z); row[4 * u + 3] = pk_fold(v.w);
        }
    }
    __syncthreads();
    // ---- 2. both strands of bases 32 j .. 32 j + 31 ----
    PackChunk fw, rv;
    if (live) {
        uint32_t V[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int nv = (int)L - (int)(32u * j + 8u * h);                                   // bases of either strand in one-hot word 4 j + h
            const uint32_t s = 16u - 2u * (uint32_t)(nv < 0 ? 0 : nv > 8 ? 8 : nv);
            V[h] = (0xFFFFFFFFu >> s) >> s;
        }
        const uint32_t *row = lds + __umul24(rr, rw);
        uint32_t w[9];
        {   // strand 0: the bytes from 32 j on
            const uint32_t at = 32u + mis + 32u * j;
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = row[(at >> 2) + k];
            fw = pack_chunk<false>(w, at & 3u, V);
        }
        {   // strand 1: the 32 bytes that end at base L - 1 - 32 j (a chunk that starts before the read begins in the 32 bytes in front of it)
            const int p0 = (int)L - 32 - 32 * (int)j;
            const uint32_t at = 32u + mis + (uint32_t)(p0 < -32 ? -32 : p0);
#pragma unroll
            for (int k = 0; k < 9; ++k) w[k] = row[(at >> 2) + k];
            rv = pack_chunk<true>(w, at & 3u, V);
        }
    }
    __syncthreads();
    // ---- 3. the block's records as an image in LDS, then out in 16-byte units ----
    uint32_t *const ipm = lds + __umul24(rr, pg.pm_stride), *const itb = lds + rpb * pg.pm_stride + __umul24(rr, pg.tb_stride);
    if (live) {
#pragma unroll
        for (int h = 0; h < 4; ++h) if (4 * j + h < pg.nw8) { ipm[4 * j + h] = fw.pm[h]; ipm[pg.nw8 + 4 * j + h] = rv.pm[h]; }
#pragma unroll
        for (int g = 0; g < 2; ++g) if (2 * j + g < pg.nw16) { itb[2 * j + g] = fw.t2[g]; itb[pg.nw16 + 2 * j + g] = rv.t2[g]; }
        itb[2 * pg.nw16 + j] = fw.nf; itb[2 * pg.nw16 + pg.nw32 + j] = rv.nf;
        if (j == 0) { ipm[2 * pg.nw8] = L; itb[2 * pg.nw16 + 2 * pg.nw32] = L; }
    }
    __syncthreads();
    if (live) {
        uint32_t *pmr = pm + (uint64_t)(r0 + rr) * pg.pm_stride, *tbr = tb + (uint64_t)(r0 + rr) * pg.tb_stride;
        const uint32_t npm = 2 * pg.nw8 + 1, ntb = 2 * pg.nw16 + 2 * pg.nw32 + 1;            // defined words of a record
        for (uint32_t u = 4 * j; u < npm; u += 4 * tpr) {
            if (u + 4 <= npm) *reinterpret_cast<uint4 *>(pmr + u) = *reinterpret_cast<const uint4 *>(ipm + u);
            else for (uint32_t k = u; k < npm; ++k) pmr[k] = ipm[k];
        }
        for (uint32_t u = 4 * j; u < ntb; u += 4 * tpr) {
            if (u + 4 <= ntb) *reinterpret_cast<uint4 *>(tbr + u) = *reinterpret_cast<const uint4 *>(itb + u);
            else for (uint32_t k = u; k < ntb; ++k) tbr[k] = itb[k];
        }
    }
}

void launch_pack(const PackGeom &pg, uint32_t n_reads, const uint8_t *seqs, const uint32_t *offs, uint32_t *pm, uint32_t *tb, hipStream_t st)
{
    if (!n_reads) return;
    const uint32_t rpb = pack_reads_per_block(pg);
    hipLaunchKernelGGL(k_pack, dim3((n_reads + rpb - 1) / rpb), dim3(pg.nw32, rpb), pack_lds_words(pg) * 4u, st, pg, n_reads, seqs, offs, pm, tb);
}

// ---------------------------------------------------------------------------------------------
// k_seed
// ---------------------------------------------------------------------------------------------
// One seed = (read, strand, slot).  Every seed needs the W-mer table gather; after it most C intervals are ONE row and are
// finished on the spot against the genome text, while the seeds that still have to walk -- C intervals with several rows
// (repeats) and seeds alive in the R index (k-mers around SNPs, ~1 in 6) -- are minorities.  A wave pays for the longest of
// its 64 lanes, so those walks are not done where they arise: the block collects them in LDS and its first lanes adopt them,
// densely packed (typically one wave of the four keeps walking and the other three retire).
struct SeedCtx {                       // passed BY VALUE everywhere: anything reached through `this` or a reference stays in scratch memory
    const uint32_t *t2, *tn;           // 2-bit codes / N flags of this strand in the tb record
    uint32_t L, k, W, s, wb, nb, w0, w1, w2, n0, n1;
    bool inreg;                        // seeds of up to 33 bases sit in 3 + 2 registers (bases wb*16 .. wb*16+47)
};
__device__ __forceinline__ bool seed_valid(const SeedCtx c) { return c.L >= c.k && c.s + c.k <= c.L; }
// everything of a seed's context that needs no load: where its strand's words lie in the tb record, and the seed's place in the read
__device__ __forceinline__ SeedCtx seed_ctx_geom(const SeedParams &sp, const uint32_t *tb, uint32_t item, uint32_t lkt_len)
{
    SeedCtx c;
    const uint32_t slot = item % sp.spr, rs = item / sp.spr, strand = rs & 1u, r = rs >> 1;
    // the read as k_pack left it: 2-bit codes (first base in the high bits) and 'is N' bits of this strand
    const uint32_t *rec = tb + (uint64_t)r * sp.pg.tb_stride;
    c.t2 = rec + strand * sp.pg.nw16; c.tn = rec + 2 * sp.pg.nw16 + strand * sp.pg.nw32;
    c.L = 0;                           // seed_ctx loads it; a queued walk has passed seed_valid and needs it no more
    c.k = (uint32_t)sp.l_seed; c.W = lkt_len; c.s = slot * (uint32_t)sp.l_overlap; c.inreg = c.k <= 33;
    c.wb = c.s >> 4; c.nb = c.s >> 5;
    c.w0 = c.w1 = c.w2 = c.n0 = c.n1 = 0;
    return c;
}
__device__ __forceinline__ SeedCtx seed_ctx(const SeedParams &sp, const uint32_t *tb, uint32_t item, uint32_t lkt_len)
{
    SeedCtx c = seed_ctx_geom(sp, tb, item, lkt_len);
    c.L = (tb + (uint64_t)(item / sp.spr >> 1) * sp.pg.tb_stride)[2 * sp.pg.nw16 + 2 * sp.pg.nw32];
    if (seed_valid(c)) { c.w0 = c.t2[c.wb]; c.w1 = c.t2[c.wb + 1]; c.w2 = c.t2[c.wb + 2]; c.n0 = c.tn[c.nb]; c.n1 = c.tn[c.nb + 1]; }     // stays inside the record (PackGeom)
    return c;
}
__device__ __forceinline__ uint32_t seed_base2(const SeedCtx c, uint32_t i)
{
    if (c.inreg && i >= c.s) { const uint32_t rel = i - (c.wb << 4); const uint32_t ws = rel < 16 ? c.w0 : rel < 32 ? c.w1 : c.w2; return (ws >> (30 - 2 * (rel & 15u))) & 3u; }
    return (c.t2[i >> 4] >> (30 - 2 * (i & 15u))) & 3u;
}
__device__ __forceinline__ bool seed_is_n(const SeedCtx c, uint32_t i)
{
    if (c.inreg && i >= c.s) { const uint32_t rel = i - (c.nb << 5); const uint32_t ns = rel < 32 ? c.n0 : c.n1; return (ns >> (31 - (rel & 31u))) & 1u; }
    return (c.tn[i >> 5] >> (31 - (i & 31u))) & 1u;
}

// ---- the rest of a search behind the W-mer table, as a per-lane state and a step ---------------------------------------------------
// C: bwt_match_exact_alt (bwt.c:281-309) from interval [k, l] with head bases s .. s+i still to consume, newest first, then the
// interval-shrinking extension (alnse.c:246-258).  R: Rbwt_exact_match_backward (rbwt.c:619-648) and its extension, which has no N guard: an
// N walks the '#' column there (alnse.c:279-291).  A step is cut in two, seed_walk_issue (the step's loads: at most ONE memory round trip)
// and seed_walk_finish (what the phase does with them), so that k_seed_walk can put the loads of all its lanes, whatever their phases, in
// front of one wait.  This is the only statement of the rules: seed_c_rest / seed_r_rest loop over the same two functions.
//   WK_HEAD  one Occ step on head base s + i.
//   WK_EXT   one Occ step on base s - ext - 1 while the interval is wider than max_seed.
//   WK_SA    (C) the interval is ONE row and cannot branch any more: the search succeeds iff the read's remaining head bases equal the text
//            in front of that suffix.  This step fetches the row's context record, which holds the suffix's position AND the CTX_N_B bases
//            in front of it (salt_ctx_record.h; side B is complete iff CTX_N_B <= p0 <= ctx_len), or without the table the suffix-array
//            entry; the seed leaves located (.w = 2: .x = .y = the genome position), dead, or goes on to
//   WK_TEXT  (C) the comparison against the 2-bit text: at most two pieces of up to 16 bases, the later bases (consumed first) first.
//   WK_REC is k_seed_walk's own (a refilled lane's queue record, which carries the seed's tb words).
enum : uint32_t { WK_IDLE = 0, WK_REC, WK_HEAD, WK_EXT, WK_SA, WK_TEXT };
struct Walk { uint32_t ph, k, l, ext, p0; int i; };                 // p0: WK_TEXT's suffix position
// What a step reads, as addresses: up to four 16-byte pieces from each of pa and pb (the Occ blocks of the interval's two ends; the context
// record; the two halves of k_seed_walk's queue record) and up to three / two words from ps / pt (the base's tb words when it is not in
// registers, the suffix-array entry, the text pieces).  walk_fetch does the loads: every register of WalkLoads is written by
// ONE load and by nothing else, whatever the phase -- a register shared between differently shaped loads would be copied into place
// behind its load, and the copy waits for the load right where it was issued.  Pieces not asked for stay unset and are not read.
struct WalkReq { const uint4 *pa, *pb; const uint32_t *ps, *pt; uint32_t na, nb, ns, nt; };
struct WalkLoads { uint4 a[4], b[4]; uint32_t s[3], t[2]; };
__device__ __forceinline__ WalkReq walk_req_none() { return WalkReq{ nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u, 0u }; }
__device__ __forceinline__ WalkLoads walk_fetch(const WalkReq q)
{
    WalkLoads ld;
    if (q.na > 0) ld.a[0] = q.pa[0];
    if (q.na > 1) ld.a[1] = q.pa[1];
    if (q.na > 2) { ld.a[2] = q.pa[2]; ld.a[3] = q.pa[3]; }
    if (q.nb > 0) { ld.b[0] = q.pb[0]; ld.b[1] = q.pb[1]; }
    if (q.nb > 2) { ld.b[2] = q.pb[2]; ld.b[3] = q.pb[3]; }
    if (q.ns > 0) ld.s[0] = q.ps[0];
    if (q.ns > 1) ld.s[1] = q.ps[1];
    if (q.ns > 2) ld.s[2] = q.ps[2];
    if (q.nt > 0) ld.t[0] = q.pt[0];
    if (q.nt > 1) ld.t[1] = q.pt[1];
    return ld;
}

__device__ __forceinline__ uint32_t walk_pos(const SeedCtx c, const Walk w) { return w.ph == WK_HEAD ? c.s + (uint32_t)w.i : c.s - w.ext - 1u; }
__device__ __forceinline__ bool walk_pos_inreg(const SeedCtx c, uint32_t pos) { return c.inreg && pos >= c.s; }
// behind the head bases, and after every extension step: the extension while the interval is still wide and bases are left, else the row
__device__ __forceinline__ bool walk_enter_ext(const SeedParams &sp, const SeedCtx c, Walk &w, uint4 &row)
{
    if (w.l - w.k > sp.max_seed && w.ext < c.s) { w.ph = WK_EXT; return false; }
    row = make_uint4(w.k, w.l, c.s - w.ext, 1); w.ph = WK_IDLE;
    return true;
}
// every function returns true when the walk has ended, with its row in `row`
template <bool R>
__device__ __forceinline__ bool seed_walk_begin(const SeedParams &sp, const SeedCtx c, uint32_t k, uint32_t l, int i_top, Walk &w, uint4 &row)
{
    w.k = k; w.l = l; w.i = i_top; w.ext = 0; w.p0 = 0;
    if (i_top < 0) return walk_enter_ext(sp, c, w, row);
    w.ph = (!R && c.inreg && sp.resolve_unique && k == l) ? WK_SA : WK_HEAD;
    return false;
}
template <bool R>
__device__ __forceinline__ WalkReq seed_walk_issue(const IndexView &ix, const SeedParams &sp, const SeedCtx c, const Walk w)
{
    WalkReq q = walk_req_none();
    if (!R && w.ph == WK_SA) {
        if (ix.c_ctx && (uint32_t)w.i + 1u <= CTX_N_B) { q.pa = ix.c_ctx + w.k; q.na = 1; } else { q.ps = ix.c_sa + w.k; q.ns = 1; }
    } else if (!R && w.ph == WK_TEXT) {
        const uint32_t m = (uint32_t)w.i + 1u, t0 = w.p0 - (m > 16u ? 16u : m);
        q.ps = ix.text + (t0 >> 4); q.ns = 2;
        if (m > 16u) { q.pt = ix.text + ((w.p0 - m) >> 4); q.nt = 2; }
    } else {
        const uint32_t pos = walk_pos(c, w);
        const bool inr = walk_pos_inreg(c, pos);
        if (!inr) { q.ps = c.t2 + (pos >> 4); q.ns = 1; q.pt = c.tn + (pos >> 5); q.nt = 1; }
        // an N already visible in the registers ends the walk without a fetch; one that comes with the tb words is seen behind the wait, and
        // the blocks requested beside it are dropped uncounted
        if (!(inr && seed_is_n(c, pos) && !(R && w.ph == WK_EXT))) {
            if (R) { r_occ2_addr(ix, w.k, w.l + 1u, q.pa, q.pb); q.na = 4; q.nb = q.pb ? 4u : 0u; }
            else { c_occ2_addr(ix, w.k - 1u, w.l, q.pa, q.pb); q.na = q.pa ? 2u : 0u; q.nb = q.pb ? 2u : 0u; }
        }
    }
    return q;
}
template <bool R>
__device__ __forceinline__ bool seed_walk_finish(const IndexView &ix, const SeedParams &sp, const SeedCtx c, Walk &w, const WalkLoads ld, uint4 &row,
                                                 uint32_t &n_occ, uint32_t &n_aux)
{
    const uint32_t s = c.s;
    const uint4 dead = make_uint4(1, 0, 0, 0);
    if (!R && w.ph == WK_SA) {
        const uint32_t m = (uint32_t)w.i + 1u, reln = s - (c.nb << 5);
        const uint64_t vn = ((uint64_t)c.n0 << 32) | c.n1;
        const bool head_n = ((vn >> (64 - reln - m)) & ((1ull << m) - 1ull)) != 0;
        const uint32_t ctx_len = ix.c_seq_len < ix.ref_len ? ix.c_seq_len : ix.ref_len;
        const bool rec = ix.c_ctx && m <= CTX_N_B;           // the row's context record, whose .x is the suffix-array entry again
        const uint32_t sa0 = rec ? ld.a[0].x : ld.s[0];
        const uint32_t p0 = sa0 == 0xFFFFFFFFu ? ix.c_seq_len : sa0;      // row 0: the empty suffix
        n_aux += 1u << 10;                                   // one suffix-array load (bits 10..20; the context record counts as one)
        if (rec && p0 >= CTX_N_B && p0 <= ctx_len) {
            const uint32_t lo = ctx_front_lo(ld.a[0]), hi = ctx_front_hi(ld.a[0]);
            uint32_t rlo = 0, rhi = 0;
            for (uint32_t u = 0; u < m; ++u) {               // read base s + i - u faces genome base p0 - 1 - u
                const uint32_t rel = s + (uint32_t)w.i - u - (c.wb << 4);
                const uint32_t ws = rel < 16 ? c.w0 : rel < 32 ? c.w1 : c.w2;
                const uint32_t code = (ws >> (30 - 2 * (rel & 15u))) & 3u;
                rlo |= (code & 1u) << u; rhi |= (code >> 1) << u;
            }
            const uint32_t mk = (1u << m) - 1u;
            const bool same = !head_n && (((lo ^ rlo) | (hi ^ rhi)) & mk) == 0;
            row = same ? make_uint4(p0 - m, p0 - m, s, 2) : dead; w.ph = WK_IDLE;
            return true;
        }
        if (head_n || p0 < m) { row = dead; w.ph = WK_IDLE; return true; }
        w.p0 = p0; w.ph = WK_TEXT;
        return false;
    }
    if (!R && w.ph == WK_TEXT) {
        const uint32_t m = (uint32_t)w.i + 1u;
        bool ok = true;
        for (uint32_t done = 0, piece = 0; done < m && ok; ++piece) {
            const uint32_t cnt = (m - done) > 16u ? 16u : (m - done);
            const uint32_t r0 = s + (m - done - cnt), t0 = w.p0 - done - cnt;     // read bases r0 .. r0+cnt-1 against text t0 ..
            const uint32_t rel = r0 - (c.wb << 4), rr = rel & 15u;
            const uint64_t vr = rel < 16 ? (((uint64_t)c.w0 << 32) | c.w1) : (((uint64_t)c.w1 << 32) | c.w2);
            const uint32_t xr = (uint32_t)((vr >> (64 - 2 * rr - 2 * cnt)) & ((1ull << (2 * cnt)) - 1ull));
            const uint32_t tr = t0 & 15u;
            const uint64_t vt = piece == 0 ? (((uint64_t)ld.s[0] << 32) | ld.s[1]) : (((uint64_t)ld.t[0] << 32) | ld.t[1]);
            n_aux += 1u << 21;                               // one 8-byte text load (bits 21..31)
            const uint32_t xt = (uint32_t)((vt >> (64 - 2 * tr - 2 * cnt)) & ((1ull << (2 * cnt)) - 1ull));
            ok = xr == xt;
            done += cnt;
        }
        row = ok ? make_uint4(w.p0 - m, w.p0 - m, s, 2) : dead; w.ph = WK_IDLE;
        return true;
    }
    const bool head = w.ph == WK_HEAD;
    const uint32_t pos = walk_pos(c, w);
    const bool inr = walk_pos_inreg(c, pos);
    const bool isn = inr ? seed_is_n(c, pos) : ((ld.t[0] >> (31 - (pos & 31u))) & 1u) != 0;
    const uint4 stop = head ? dead : make_uint4(w.k, w.l, s - w.ext, 1);      // a head step that fails kills the seed, an extension step only ends the extension
    if (isn && !(R && !head)) { row = stop; w.ph = WK_IDLE; return true; }
    const uint32_t b = isn ? 4u : inr ? seed_base2(c, pos) : (ld.s[0] >> (30 - 2 * (pos & 15u))) & 3u;
    uint32_t ok, ol;
    if (R) n_occ += r_occ2_eval(ix, ROcc2{ ROccBlk{ ld.a[0], ld.a[1], ld.a[2], ld.a[3] }, ROccBlk{ ld.b[0], ld.b[1], ld.b[2], ld.b[3] } }, w.k, w.l + 1u, b, ok, ol);
    else n_occ += c_occ2_eval(ix, COcc2{ ld.a[0], ld.a[1], ld.b[0], ld.b[1] }, w.k - 1u, w.l, b, ok, ol);
    if (ok + 1u > ol) { row = stop; w.ph = WK_IDLE; return true; }             // the interval would be empty
    { const uint32_t first = R ? pick5(ix.r_cum, b) : pick4(ix.c_L2, b); w.k = first + ok + 1u; w.l = first + ol; }
    if (head) {
        if (--w.i >= 0) { if (!R && c.inreg && sp.resolve_unique && w.k == w.l) w.ph = WK_SA; return false; }
    } else ++w.ext;
    return walk_enter_ext(sp, c, w, row);
}

// the whole walk on one lane, as a loop over the step
template <bool R>
__device__ __forceinline__ uint4 seed_walk_rest(const IndexView &ix, const SeedParams &sp, const SeedCtx c, uint32_t k, uint32_t l, int i_top,
                                                uint32_t &n_occ, uint32_t &n_aux)
{
    Walk w; uint4 row = make_uint4(1, 0, 0, 0);
    bool done = seed_walk_begin<R>(sp, c, k, l, i_top, w, row);
    while (!done) { const WalkLoads ld = walk_fetch(seed_walk_issue<R>(ix, sp, c, w)); done = seed_walk_finish<R>(ix, sp, c, w, ld, row, n_occ, n_aux); }
    return row;
}
__device__ __forceinline__ uint4 seed_c_rest(const IndexView &ix, const SeedParams &sp, const SeedCtx c, uint32_t kc, uint32_t lc, int i_top,
                                             uint32_t &n_occ_c, uint32_t &n_aux)
{
    return seed_walk_rest<false>(ix, sp, c, kc, lc, i_top, n_occ_c, n_aux);
}
__device__ __forceinline__ uint4 seed_r_rest(const IndexView &ix, const SeedParams &sp, const SeedCtx c, uint32_t kr, uint32_t lr, int i_top,
                                             uint32_t &n_occ_r)
{
    uint32_t n_aux = 0;
    return seed_walk_rest<true>(ix, sp, c, kr, lr, i_top, n_occ_r, n_aux);
}

static constexpr uint32_t WQ_SEG = 64, WQ_STRIDE = 64;            // segments per walk queue; words between their counters
static constexpr uint32_t WQ_REC = 2;                             // uint4 per walk record: (item, k, l, n0) (w0, w1, w2, n1)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_seed(IndexView ix, SeedParams sp, const uint32_t *__restrict__ tb,
       uint4 *__restrict__ sai_c, uint4 *__restrict__ sai_r, uint4 *__restrict__ wq, uint32_t *__restrict__ wq_cnt, uint32_t wq_seg_cap,
       unsigned long long *__restrict__ ctr)
{
    // walks still to do go to the queues k_seed_walk drains: [0] R searches, [1] C searches.  The block counts its walks in LDS, reserves
    // their slots in ONE of WQ_SEG segments per list with one atomic (an atomic on one address is served every ~11 ns: 31 000 blocks on one
    // counter would be a third of a millisecond) and every lane stores its own record: two uint4, (item, k, l, n0) and (w0, w1, w2, n1), the
    // five tb words seed_ctx has loaded, so that the walk needs no fetch from the read's tb record before its first step (a seed beyond the
    // in-register limit carries them unused).  The slots of a block are dense in its segment: the stores still cover whole lines.
    __shared__ uint32_t q_n[2], q_base[2];
    const uint64_t item = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, n_items = (uint64_t)sp.n_reads * 2u * sp.spr;
    const uint64_t lt = (1ull << lane_id()) - 1ull;
    uint32_t n_lkt = 0, n_occ_c = 0, n_occ_r = 0;
    if (threadIdx.x < 2) { q_n[threadIdx.x] = 0; q_base[threadIdx.x] = 0; }
    __syncthreads();
    bool pend_c = false, pend_r = false;
    uint32_t pk_c = 0, pl_c = 0, pk_r = 0, pl_r = 0, at_r = 0, at_c = 0;
    uint32_t cw0 = 0, cw1 = 0, cw2 = 0, cn0 = 0, cn1 = 0;     // the seed's tb words, for its walk records
    if (item < n_items) {
        const SeedCtx c = seed_ctx(sp, tb, (uint32_t)item, ix.r_lkt_len);
        cw0 = c.w0; cw1 = c.w1; cw2 = c.w2; cn0 = c.n0; cn1 = c.n1;
        uint4 oc = make_uint4(1, 0, 0, 0);
        if (seed_valid(c)) {
            const uint32_t e = c.s + c.k - 1, W = c.W;
            // W-mer at the seed tail: both searches start from their tabulated interval
            // (LKT_seq2LktItem / LKT_lookup_sa lookup.c:163-177 + the first steps of bwt.c:281-309, rbwt.c:619-648)
            uint32_t x = 0; bool has_n = false;
            const uint32_t a0 = e - W + 1;
            if (c.inreg) {
                const uint32_t rel = a0 - (c.wb << 4), rr = rel & 15u;
                const uint64_t v = rel < 16 ? (((uint64_t)c.w0 << 32) | c.w1) : rel < 32 ? (((uint64_t)c.w1 << 32) | c.w2) : ((uint64_t)c.w2 << 32);
                x = (uint32_t)((v >> (64 - 2 * rr - 2 * W)) & ((1ull << (2 * W)) - 1ull));
                const uint32_t reln = a0 - (c.nb << 5);
                const uint64_t vn = ((uint64_t)c.n0 << 32) | c.n1;
                has_n = ((vn >> (64 - reln - W)) & ((1ull << W) - 1ull)) != 0;
            } else {
                for (uint32_t t = 0; t < W; ++t) { has_n |= seed_is_n(c, a0 + t); x = (x << 2) | seed_base2(c, a0 + t); }
            }
            if (!has_n) {
                const uint4 v = ix.wlkt[2 * (uint64_t)x];    // one 32-byte gather (one sector): C interval in .x/.y, R interval in .z/.w,
                const uint4 u = ix.wlkt[2 * (uint64_t)x + 1];//   and for a one-row C interval its genome position + the 16 bases in front of it
                ++n_lkt;                                     // device counters: bits 0..9 W-mer gathers, 10..20 SA loads, 21..31 text loads
                const int i_top = (int)(c.k - W) - 1;        // head bases s .. s+i_top are still to consume
                if (v.x <= v.y) {
                    const uint32_t m = c.k - W;
                    if (v.x == v.y && c.inreg && sp.resolve_unique && m >= 1 && m <= 16) {
                        // one row: the search succeeds iff the m bases in front of the W-mer equal the text in front of that suffix
                        // (what the remaining steps of bwt_match_exact_alt, bwt.c:281-309, decide) -- both are in registers
                        const uint32_t rel = c.s - (c.wb << 4), rr = rel & 15u;
                        const uint64_t vr = rel < 16 ? (((uint64_t)c.w0 << 32) | c.w1) : (((uint64_t)c.w1 << 32) | c.w2);
                        const uint32_t mk = m == 16 ? 0xFFFFFFFFu : ((1u << (2 * m)) - 1u);
                        const uint32_t xr = (uint32_t)(vr >> (64 - 2 * rr - 2 * m)) & mk;
                        const uint32_t reln2 = c.s - (c.nb << 5);
                        const uint64_t vn2 = ((uint64_t)c.n0 << 32) | c.n1;
                        const bool head_n = ((vn2 >> (64 - reln2 - m)) & ((1ull << m) - 1ull)) != 0;
                        if (!head_n && u.x >= m && xr == (u.y & mk)) oc = make_uint4(u.x - m, u.x - m, c.s, 2);
                    }
                    else if (v.y == v.x + 1u && c.inreg && sp.resolve_unique && m >= 1 && m <= 16) {
                        // two rows (a tenth of the seeds at W = 16 on 3.1e9 bases: chance repeats of the 16-mer): the entry holds both
                        // suffixes' positions and the bases in front of them.  The m steps still to do keep exactly the rows whose text
                        // continues like the read: none -> dead, one -> that row, located; both -> the walk decides (a real repeat)
                        const uint32_t rel = c.s - (c.wb << 4), rr = rel & 15u;
                        const uint64_t vr = rel < 16 ? (((uint64_t)c.w0 << 32) | c.w1) : (((uint64_t)c.w1 << 32) | c.w2);
                        const uint32_t mk = m == 16 ? 0xFFFFFFFFu : ((1u << (2 * m)) - 1u);
                        const uint32_t xr = (uint32_t)(vr >> (64 - 2 * rr - 2 * m)) & mk;
                        const uint32_t reln2 = c.s - (c.nb << 5);
                        const uint64_t vn2 = ((uint64_t)c.n0 << 32) | c.n1;
                        const bool head_n = ((vn2 >> (64 - reln2 - m)) & ((1ull << m) - 1ull)) != 0;
                        const bool ok0 = !head_n && u.x >= m && xr == (u.y & mk), ok1 = !head_n && u.z >= m && xr == (u.w & mk);
                        if (ok0 && ok1) { pend_c = true; pk_c = v.x; pl_c = v.y; }
                        else if (ok0) oc = make_uint4(u.x - m, u.x - m, c.s, 2);
                        else if (ok1) oc = make_uint4(u.z - m, u.z - m, c.s, 2);
                    }
                    else {
                        // everything else walks in k_seed_walk, unless the walk ends before its first fetch (k = W and no extension).  The
                        // whole walk inlined here (seed_c_rest) for the few shapes that need no Occ step cost every seed's gather path
                        // its registers: 40 bytes of scratch at the 64 VGPRs of eight waves per SIMD
                        Walk w;
                        if (!seed_walk_begin<false>(sp, c, v.x, v.y, i_top, w, oc)) { pend_c = true; pk_c = v.x; pl_c = v.y; }
                    }
                }
                if (!sp.seed_only_ref) {
                    if (v.z <= v.w) { pend_r = true; pk_r = v.z; pl_r = v.w; }
                }
            }
        }
        sai_c[item] = oc;                                     // a queued seed's row is the dead one here: k_seed_walk stores only the rows of walks that end
                                                              //   alive.  No R row is written: one without this call's epoch is dead (sai_r_row)
    }
    // collect: one LDS atomic per wave and list
    {
        const uint64_t mr = __ballot(pend_r), mc = __ballot(pend_c);
        uint32_t br = 0, bc = 0;
        if (lane_id() == 0) { if (mr) br = atomicAdd(&q_n[0], (uint32_t)__popcll(mr)); if (mc) bc = atomicAdd(&q_n[1], (uint32_t)__popcll(mc)); }
        br = (uint32_t)__shfl((int)br, 0); bc = (uint32_t)__shfl((int)bc, 0);
        at_r = br + (uint32_t)__popcll(mr & lt); at_c = bc + (uint32_t)__popcll(mc & lt);
    }
    __syncthreads();
    const uint32_t seg = blockIdx.x & (WQ_SEG - 1u);
    if (threadIdx.x < 2 && q_n[threadIdx.x]) q_base[threadIdx.x] = atomicAdd(&wq_cnt[(threadIdx.x * WQ_SEG + seg) * WQ_STRIDE], q_n[threadIdx.x]);
    __syncthreads();
    if (pend_r) {
        uint4 *rec = wq + ((size_t)seg * wq_seg_cap + q_base[0] + at_r) * WQ_REC;
        rec[0] = make_uint4((uint32_t)item, pk_r, pl_r, cn0); rec[1] = make_uint4(cw0, cw1, cw2, cn1);
    }
    if (pend_c) {
        uint4 *rec = wq + (((size_t)WQ_SEG + seg) * wq_seg_cap + q_base[1] + at_c) * WQ_REC;
        rec[0] = make_uint4((uint32_t)item, pk_c, pl_c, cn0); rec[1] = make_uint4(cw0, cw1, cw2, cn1);
    }
    if (ctr) {                                                // one atomic per wave and counter
        for (int o = 32; o > 0; o >>= 1) {
            n_lkt += __shfl_down(n_lkt, o); n_occ_c += __shfl_down(n_occ_c, o); n_occ_r += __shfl_down(n_occ_r, o);
        }
        if (lane_id() == 0) {
            atomicAdd(ctr + SALT_CTR_LKT, n_lkt & 1023u); atomicAdd(ctr + SALT_CTR_OCC_C, n_occ_c); atomicAdd(ctr + SALT_CTR_OCC_R, n_occ_r);
            atomicAdd(ctr + SALT_CTR_D_WLKT, n_lkt & 1023u); atomicAdd(ctr + SALT_CTR_D_COCC_SEED, n_occ_c); atomicAdd(ctr + SALT_CTR_D_ROCC_SEED, n_occ_r);
            atomicAdd(ctr + SALT_CTR_D_SA_SEED, (n_lkt >> 10) & 2047u); atomicAdd(ctr + SALT_CTR_D_TEXT_SEED, n_lkt >> 21);
        }
    }
}

// k_seed_walk: the walks k_seed queued, in turns.  In a turn every busy lane does ONE step of its walk (seed_walk_issue / seed_walk_finish:
// one memory round trip), and the lanes whose walks have ended take the next records of the wave's slice, so a wave no longer pays for the
// longest of 64 walks (R walks die after 1 to 5 steps, C walks of repeat seeds run their head and up to s extension steps) with the other
// lanes idle.  A refilled lane's dependent load is a lane state too (WK_REC: both halves of the queue record, which hold the seed's interval
// and its tb words; the walk begins behind that wait and issues its first step in the next turn), and a turn first issues the loads of ALL
// its lanes and then uses them: one wait per turn, whatever the mix of phases.
//   Work is handed out statically: block b serves segment b % WQ_SEG, and wave w of the nw waves on that segment owns the records
// [n w / nw, n (w + 1) / nw) of both of its lists, the first list in front of the second (C first: the long walks start first and the short R
// walks fill the lanes they leave).  No atomics, nothing a wave could wait for.  The ballot and the cursor sit at the top of the turn
// with all 64 lanes present and no lane leaves the loop on its own (loops in which lane groups leave one by one have
// hung); every turn consumes records or advances every live walk, and a walk has at most k - W + s + 3 turns.
//   k_seed has written the dead C row for every queued seed and an R row counts only with this call's epoch in it (sai_r_row, salt_device.h),
// so only a walk that ends alive stores its row.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_seed_walk(IndexView ix, SeedParams sp, const uint32_t *__restrict__ tb, uint4 *__restrict__ sai_c, uint4 *__restrict__ sai_r,
            const uint4 *__restrict__ wq, const uint32_t *__restrict__ wq_cnt, uint32_t wq_seg_cap, uint32_t r_first, unsigned long long *__restrict__ ctr)
{
    const uint32_t seg = blockIdx.x & (WQ_SEG - 1u);
    const uint32_t wv = (blockIdx.x / WQ_SEG) * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = (gridDim.x / WQ_SEG) * 4u;
    const uint64_t lt = (1ull << lane_id()) - 1ull;
    const uint32_t la = r_first ? 0u : 1u, lb = la ^ 1u;                       // list 0: R searches, list 1: C searches
    const uint32_t na = wq_cnt[(la * WQ_SEG + seg) * WQ_STRIDE], nb = wq_cnt[(lb * WQ_SEG + seg) * WQ_STRIDE];
    const uint32_t a0 = (uint32_t)((uint64_t)na * wv / nw), a1 = (uint32_t)((uint64_t)na * (wv + 1u) / nw);
    const uint32_t b0 = (uint32_t)((uint64_t)nb * wv / nw), b1 = (uint32_t)((uint64_t)nb * (wv + 1u) / nw);
    const uint4 *qa = wq + (((size_t)la * WQ_SEG + seg) * wq_seg_cap + a0) * WQ_REC, *qb = wq + (((size_t)lb * WQ_SEG + seg) * wq_seg_cap + b0) * WQ_REC;
    const uint32_t tot_a = a1 - a0, tot = tot_a + (b1 - b0);
    const int i_top = (int)((uint32_t)sp.l_seed - ix.r_lkt_len) - 1;
    uint32_t n_aux = 0, n_sa = 0, n_text = 0, n_occ_c = 0, n_occ_r = 0;
    Walk w; w.ph = WK_IDLE; w.k = w.l = w.ext = w.p0 = 0; w.i = 0;
    SeedCtx c = seed_ctx_geom(sp, tb, 0, ix.r_lkt_len);
    uint32_t item = 0, cur = 0;
    bool is_r = false;
    const uint4 *qp = qa;
    for (;;) {
        // ---- all 64 lanes: who is idle, is anything left, who takes which record ----
        const uint64_t idle = __ballot(w.ph == WK_IDLE);
        if (cur >= tot && idle == ~0ull) break;                               // the one exit, wave-uniform
        if (cur < tot) {
            const uint32_t t = cur + (uint32_t)__popcll(idle & lt);
            if (w.ph == WK_IDLE && t < tot) {
                const bool in_a = t < tot_a;
                qp = in_a ? qa + (size_t)t * WQ_REC : qb + (size_t)(t - tot_a) * WQ_REC; is_r = (in_a ? la : lb) == 0u; w.ph = WK_REC;
            }
            const uint32_t nx = cur + (uint32_t)__popcll(idle);
            cur = nx < tot ? nx : tot;
        }
        // ---- every lane's loads of this turn ----
        WalkReq q = walk_req_none();
        if (w.ph == WK_REC) { q.pa = qp; q.na = WQ_REC; }
        else if (w.ph != WK_IDLE) q = is_r ? seed_walk_issue<true>(ix, sp, c, w) : seed_walk_issue<false>(ix, sp, c, w);
        const WalkLoads ld = walk_fetch(q);
        // ---- and what their phases do with them ----
        bool done = false;
        uint4 row = make_uint4(1, 0, 0, 0);
        if (w.ph == WK_REC) {
            item = ld.a[0].x;
            c = seed_ctx_geom(sp, tb, item, ix.r_lkt_len);
            c.w0 = ld.a[1].x; c.w1 = ld.a[1].y; c.w2 = ld.a[1].z; c.n0 = ld.a[0].w; c.n1 = ld.a[1].w;
            done = is_r ? seed_walk_begin<true>(sp, c, ld.a[0].y, ld.a[0].z, i_top, w, row) : seed_walk_begin<false>(sp, c, ld.a[0].y, ld.a[0].z, i_top, w, row);
        } else if (w.ph != WK_IDLE) {
            done = is_r ? seed_walk_finish<true>(ix, sp, c, w, ld, row, n_occ_r, n_aux) : seed_walk_finish<false>(ix, sp, c, w, ld, row, n_occ_c, n_aux);
        }
        if (done && row.x <= row.y) { if (is_r) { row.w = sai_r_pack(sp.epoch, row.w); sai_r[item] = row; } else sai_c[item] = row; }
        n_sa += (n_aux >> 10) & 2047u; n_text += n_aux >> 21; n_aux = 0;       // a lane does many walks here: the packed fields would run over
    }
    if (ctr) {
        for (int o = 32; o > 0; o >>= 1) { n_sa += __shfl_down(n_sa, o); n_text += __shfl_down(n_text, o); n_occ_c += __shfl_down(n_occ_c, o); n_occ_r += __shfl_down(n_occ_r, o); }
        if (lane_id() == 0) {
            atomicAdd(ctr + SALT_CTR_OCC_C, n_occ_c); atomicAdd(ctr + SALT_CTR_OCC_R, n_occ_r);
            atomicAdd(ctr + SALT_CTR_D_COCC_SEED, n_occ_c); atomicAdd(ctr + SALT_CTR_D_ROCC_SEED, n_occ_r);
            atomicAdd(ctr + SALT_CTR_D_SA_SEED, n_sa); atomicAdd(ctr + SALT_CTR_D_TEXT_SEED, n_text);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_align: LDS of one wave
// ---------------------------------------------------------------------------------------------
template <int NS> struct SaiListsT { uint32_t sp[2][NS], ep[2][NS], off[2][NS]; };     // [0]=C, [1]=R
struct SaiLists { uint32_t *sp[2], *ep[2], *off[2]; };                                // the same lists by reference (the sort replica below)
template <int NS> __device__ __forceinline__ SaiLists sai_ref(SaiListsT<NS> &a) { return SaiLists{ { a.sp[0], a.sp[1] }, { a.ep[0], a.ep[1] }, { a.off[0], a.off[1] } }; }
struct LvTables { short L[LVK][64]; char A[LVK][64]; };
// Where lv_wave's furthest-reaching values and actions go, rows of 64 diagonals, one row a level: a block's LvTables in global memory
// (any k the reference admits) or, for k <= LLV_K, LvTablesLds in the block's LDS, where lane 0's traceback reads them back without
// a trip to L2 per load.  L == nullptr: the distance alone.
struct LvTabRef { short *L; char *A; };
// lane-parallel LV (one candidate per lane): nibble-packed text window per lane and the pattern, both zero-padded in LDS over every
// word lv_lanes can ask for; the DP row lives in registers
static constexpr int LLV_K = 12;                 // handles k <= 12 (reads up to 129 bp at k = L/10)
static constexpr int LLV_TW = 22;                // window words per lane + 1: up to 8 * (LLV_TW - 1) = 168 text nibbles, reads up to 164 bases
static constexpr int LLV_N = 64;                 // candidates per round: one per lane
static constexpr int LLV_WIN = 4;                // the text window is LLV_WIN nibbles longer than the read (ed_diff, editdistance.c:174)
// What lv_lanes indexes (plen = the read, tlen = plen + LLV_WIN <= 8 * (LLV_TW - 1), |d| <= k <= LLV_K):
//   pattern nibble i with 0 <= i <= plen: a cell of a lane that is not done holds a value < plen, so best <= plen;
//   text nibble d + i.  d + i >= 0: on a diagonal d < 0 every cell is >= -d (L[e][-e] = L[e-1][-e+1] + 1 >= e, and a cell never lies
//   under its right neighbour + 1), on d >= 0 every reachable cell is >= 0.  d + i <= LLV_K + plen: the extension stops under
//   min(plen, tlen - d), only the gate looks at best <= plen on d <= LLV_K.
// Both are read eight nibbles at a time from any start, i.e. as the words (i >> 3) and (i >> 3) + 1: text words 0 .. LLV_TS - 1,
// pattern words 0 .. LLV_PW - 1, staged with zeros behind the window / the read (lane_text, lane_pattern), so no load is predicated.
static constexpr int LLV_TS = LLV_TW + 2;        // text words staged per lane
static constexpr int LLV_PW = LLV_TW;            // pattern words staged
static_assert(((8 * (LLV_TW - 1) - LLV_WIN + LLV_K) >> 3) + 2 <= LLV_TS, "text words of the longest window at the widest bound");
static_assert(((8 * (LLV_TW - 1) - LLV_WIN) >> 3) + 2 <= LLV_PW, "pattern words of the longest read");
// T is word-major, T[j * LLV_N + lane]: the LDS bank of a read is the lane's alone, whatever j each lane asks for (lane-major rows of
// 22 words put 32 lanes on 16 banks).  P: the pattern all lanes share in k_gap and k_heavy (k_diag_lv gives every lane its own).
struct LaneLv { uint32_t T[LLV_TS * LLV_N]; uint32_t P[LLV_PW]; };
struct LvBytes { uint8_t T[MAXL + 4 + 64]; uint8_t P[MAXL + 64]; };
struct LvTablesLds { short L[LLV_K + 1][64]; char A[LLV_K + 1][64]; };     // 2 496 B: levels 0 .. LLV_K
__device__ __forceinline__ LvTabRef lv_tab(LvTables *t) { return t ? LvTabRef{ &t->L[0][0], &t->A[0][0] } : LvTabRef{ nullptr, nullptr }; }
__device__ __forceinline__ LvTabRef lv_tab(LvTablesLds &t) { return LvTabRef{ &t.L[0][0], &t.A[0][0] }; }
// the traceback's per-level actions and match runs: lane 0 keeps them over the byte strings, which are done with by then
struct LvTrace { int matched[LVK + 1]; char act[LVK + 1]; };
static_assert(sizeof(LvTrace) <= sizeof(LvBytes::T), "the traceback's levels fit the text bytes");
// NS: seed slots per list the block can hold; LLV: with the lane-LV scratch (6 KB) for gapped passes finished inside the block.
// k_heavy's usual shape is <32, false> = 7.5 KB: its LDS is what decides how much of a CU it leaves to the kernels of the other
// batches in flight (18.6 KB per block with 512 slots and the lane-LV scratch: 303-345 Mreads/s on the 4-stream step; 7.5 KB: 383-388)
template <int NS, bool LLV>
struct WaveLdsT {
    static constexpr bool HAS_LLV = LLV;
    static constexpr int N_SLOTS = NS;
    uint32_t pm[2][MAXL / 8];                               // one-hot nibble words of the read, both strands (k_pack)
    union U { SaiListsT<NS> sai; typename std::conditional<LLV, LaneLv, uint32_t>::type llv; LvBytes lvb; } u;     // seeds | lane-LV scratch | wave-LV byte strings
    uint8_t  cand_e[MAXLOC];
    uint32_t loci[MAXLOC];
    uint32_t hit_pos[2][NHIT];
    uint8_t  hit_nd[2][NHIT], hit_gap[2][NHIT];
    uint16_t cig[SALT_MAX_CIGAR_OPS];
    int      n_cig;
    alignas(8) uint8_t cargs[128];                          // build_candidates' arguments (CandArgs): see there
};
typedef WaveLdsT<SLOTS, true> WaveLds;                      // any read the ABI admits, everything finished inside the block
typedef WaveLdsT<32, false> WaveLdsSmall;                   // <= 32 seed slots per strand; a gapped read without a k_gap slot goes to the overflow queue
typedef WaveLdsT<1, false> WaveLdsCigar;                    // k_cigar: the read, the byte strings of one traceback, the CIGAR

// ---- klib introsort replica (salt_sai_sort.h) on a read's seed lists ----------------------------------
// The triples where they lie, list w: one lane runs the sort, every compare four dependent LDS loads and every swap twelve LDS
// accesses.  For lists of more than 64 seeds (the big shapes).
struct SaiLdsSort {
    SaiLists &s; const int w;
    uint32_t st[SAI_STACK];                                  // a postponed range a word: lo, hi < 2^12 (SLOTS seeds), the depth above them
    __device__ __forceinline__ SaiLdsSort(SaiLists &s_, int w_) : s(s_), w(w_) {}
    __device__ __forceinline__ uint32_t key(int i) const { return s.ep[w][i] - s.sp[w][i]; }       // alnse.c:35
    __device__ __forceinline__ void swap(int i, int j)
    {
        const uint32_t a0 = s.sp[w][i], a1 = s.ep[w][i], a2 = s.off[w][i], b0 = s.sp[w][j], b1 = s.ep[w][j], b2 = s.off[w][j];
        s.sp[w][i] = b0; s.ep[w][i] = b1; s.off[w][i] = b2; s.sp[w][j] = a0; s.ep[w][j] = a1; s.off[w][j] = a2;
    }
    __device__ __forceinline__ void push(int top, int lo, int hi, int d) { st[top] = (uint32_t)lo | ((uint32_t)hi << 12) | ((uint32_t)d << 24); }
    __device__ __forceinline__ void pop(int top, int &lo, int &hi, int &d) const { const uint32_t v = st[top]; lo = (int)(v & 4095u); hi = (int)((v >> 12) & 4095u); d = (int)(v >> 24); }
};
static_assert(SLOTS <= 4096, "a seed index in 12 bits");
__device__ __attribute__((noinline)) void sai_introsort_lds(SaiLists &s, int w, int n) { SaiLdsSort a(s, w); sai_introsort(a, n); }

// A list of up to 64 seeds, element e in lane e: its key (ep - sp) and where it came from.  Every index the sort asks for is the
// same in all lanes, so a key is a v_readlane, a swap four of them and two selects, the stack a register as well (entry t in lane
// t), and a step costs a few cycles where the LDS form waits for its loads; all 64 lanes run it, control flow is wave-uniform.
// What comes out is the permutation: ix of lane e = the element that belongs at place e.
struct SaiLaneSort {
    uint32_t k, ix, stk;
    __device__ __forceinline__ uint32_t key(int i) const { return (uint32_t)__builtin_amdgcn_readlane((int)k, i); }
    __device__ __forceinline__ void swap(int i, int j)
    {
        const uint32_t ki = (uint32_t)__builtin_amdgcn_readlane((int)k, i), kj = (uint32_t)__builtin_amdgcn_readlane((int)k, j);
        const uint32_t xi = (uint32_t)__builtin_amdgcn_readlane((int)ix, i), xj = (uint32_t)__builtin_amdgcn_readlane((int)ix, j);
        const int lane = (int)lane_id();
        if (lane == i) { k = kj; ix = xj; }
        if (lane == j) { k = ki; ix = xi; }                    // (i == j: back to what it was)
    }
    __device__ __forceinline__ void push(int top, int lo, int hi, int d) { if ((int)lane_id() == top) stk = (uint32_t)lo | ((uint32_t)hi << 8) | ((uint32_t)d << 16); }
    __device__ __forceinline__ void pop(int top, int &lo, int &hi, int &d) const
    {
        const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)stk, top);
        lo = (int)(v & 255u); hi = (int)((v >> 8) & 255u); d = (int)(v >> 16);
    }
};
static_assert(SAI_STACK <= 64, "a stack entry a lane");
// All 64 lanes call it (n <= 64, the same in all): sorts the list's keys in lanes, then moves the triples in one step.
typedef uint32_t __attribute__((address_space(3))) *lds_u32w;
__device__ __attribute__((noinline)) void sai_introsort_lanes(lds_u32w sp, lds_u32w ep, lds_u32w off, int n_)
{
    const int n = __builtin_amdgcn_readfirstlane(n_);         // an argument arrives in a VGPR: tell the compiler that every index and branch below is uniform
    if (n < 2) return;
    const int lane = (int)lane_id();
    SaiLaneSort a;
    a.k = lane < n ? ep[lane] - sp[lane] : 0u; a.ix = (uint32_t)lane; a.stk = 0;
    sai_introsort(a, n);
    uint32_t v0 = 0, v1 = 0, v2 = 0;
    if (lane < n) { v0 = sp[a.ix]; v1 = ep[a.ix]; v2 = off[a.ix]; }
    WSYNC();
    if (lane < n) { sp[lane] = v0; ep[lane] = v1; off[lane] = v2; }
}

// ---- wave-wide bitonic sort of loci[0..n) in LDS (ks_introsort(uint32_t): any total sort) --------
__device__ void sort_loci(uint32_t *a, uint32_t n)
{
    if (n < 2) return;
    uint32_t P = 2; while (P < n) P <<= 1;
    for (uint32_t i = n + lane_id(); i < P; i += 64) a[i] = 0xFFFFFFFFu;
    WSYNC();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane_id(); t < (P >> 1); t += 64) {
                uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));       // element with bit j clear
                uint32_t p = i | j;
                uint32_t x = a[i], y = a[p];
                bool up = (i & k) == 0;
                if ((x > y) == up) { a[i] = y; a[p] = x; }
            }
            WSYNC();
        }
    }
}

// drop duplicates and out-of-range loci of a sorted list, keeping order (alnse.c:758-762 / 890-894)
__device__ __forceinline__ uint32_t dedup_loci(uint32_t *loci, uint32_t n, bool gap_mode, uint32_t L, uint32_t ref_len)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t n_out = 0;
    for (uint32_t b = 0; b < n; b += 64) {
        uint32_t i = b + lane;
        bool keep = false; uint32_t pos = 0;
        if (i < n) {
            pos = loci[i];
            bool dup = i > 0 && loci[i - 1] == pos;
            bool out = gap_mode ? (pos + L + 4 >= ref_len) : (pos >= ref_len);
            keep = !dup && !out;
        }
        uint64_t m = __ballot(keep);
        WSYNC();                                           // all reads of this chunk are done
        if (keep) loci[n_out + (uint32_t)__popcll(m & lt)] = pos;
        n_out += (uint32_t)__popcll(m);
        WSYNC();
    }
    return n_out;
}

// ---- candidates of one strand: gather seeds, order them, locate, sort, dedup ----------------------
// Leaves the candidate positions in w.loci[0..return).  gap_mode selects the range filter of
// alnse_check_withgap (alnse.c:894) instead of alnse_check_nogap's (alnse.c:762).
struct CandStats { uint32_t n_cand, n_sa_c, n_sa_r, n_loci; uint32_t in_lds; uint32_t n_ctx_rej, n_ctx_rows; };     // in_lds: the loci went to w.loci (PE lists that fit)
struct CandArgs {                      // everything by value: a by-reference IndexView would live in scratch memory
    const uint32_t *c_sa, *r_pos; const uint4 *sai_c, *sai_r;
    uint32_t ref_len, spr, max_locate, r, L; int strand; bool gap_mode; unsigned long long *phase;
    uint32_t *loci; uint32_t loci_cap; int pe;
    bool finish;                   // false: stop after locate (unsorted, duplicates and out-of-range loci still in)
    uint32_t epoch;                // the call's epoch: which R rows are live (sai_r_row, salt_device.h)
    const uint4 *r_ctx;                    // non-null (with c_ctx): the R rows' records, used the same way
    const uint4 *c_ctx; uint32_t ctx_k;    // non-null: rows come from the context table and a row whose window has more than 3 mismatches for
                                           // certain (ctx_reject, salt_device.h) is counted against the caps but not stored.  Gap-free pass only.
};

// The read's side of a context comparison for a seed that starts at read offset `off` (pm: the strand's one-hot words in LDS).
// Lane t faces the read base ctx_face gives plane bit t (salt_ctx_record.h).
__device__ __forceinline__ CtxRead ctx_read(const uint32_t *pm, uint32_t L, uint32_t off, uint32_t ctx_k)
{
    const int p = ctx_face(lane_id(), off, ctx_a_start(ctx_k));
    const bool v = p >= 0 && p < (int)L;
    const uint32_t nib = v ? (pm[(uint32_t)p >> 3] >> (4u * ((uint32_t)p & 7u))) & 15u : 0u;
    CtxRead rd;
    rd.lo = __ballot(v && ctx_nib_lo(nib));
    rd.hi = __ballot(v && ctx_nib_hi(nib));
    rd.use = __ballot(v && ctx_nib_use(nib));                // N (15) matches everything: not counted
    return rd;
}
// Not inlined (three call sites, ~1 400 instructions).  Its arguments are the same for all 64 lanes: passed by value they would be
// written to and read back from scratch memory once per lane and call (~6 KB per call, measured as 430 MB of writes per launch), so the
// caller leaves ONE copy in the wave's LDS.
template <bool PE, bool GL, class W>       // GL: the block has a global list for located rows beyond the LDS list (paired end; single end with -m above it).
__device__ __attribute__((noinline)) CandStats build_candidates(W &w)      // A template parameter, not a run-time flag: a list that may live in either memory is reached through flat loads
{
    const CandArgs a = *reinterpret_cast<const CandArgs *>(w.cargs);
    const uint32_t lane = lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint32_t L = a.L, r = a.r; const int strand = a.strand; const bool gap_mode = a.gap_mode;
    const gp_u32x4 sai_c = as_global(a.sai_c), sai_r = as_global(a.sai_r);
    struct { gp_u32 c_sa, r_pos; uint32_t ref_len; } ix = { as_global(a.c_sa), as_global(a.r_pos), a.ref_len };
    struct { uint32_t spr, max_locate; } ap = { a.spr, a.max_locate };
    uint32_t n_sa_c = 0, n_sa_r = 0, n_loci_out = 0;
    constexpr bool glob = GL;                                 // a global list is there: used when the rows outgrow the LDS
    uint32_t *loci = glob ? a.loci : w.loci;                 // decided below, once the number of rows is known
    PhaseClock pc(a.phase);
    const uint64_t base_item = ((uint64_t)r * 2u + (uint32_t)strand) * ap.spr;
    uint32_t n_list[2] = { 0, 0 };
    const uint32_t cap_total = PE ? a.loci_cap : ap.max_locate;
    uint32_t rows = 0;                                        // suffix-array rows the locate loops would enumerate (saturating)
    // gather valid seeds in seed order (n_C / n_back_R grow in seed_start order, alnse.c:265-300)
    for (uint32_t b = 0; b < ap.spr; b += 64) {
        const uint32_t slot = b + lane;
        uint4 v2[2] = { make_uint4(1, 0, 0, 0), make_uint4(1, 0, 0, 0) };
        if (slot < ap.spr) {                                  // both lists' loads are in flight together
            const u32x4_t tc = sai_c[base_item + slot], tr = sai_r[base_item + slot];
            v2[0] = make_uint4(tc.x, tc.y, tc.z, tc.w); v2[1] = sai_r_row(make_uint4(tr.x, tr.y, tr.z, tr.w), a.epoch);
        }
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const uint4 v = v2[which];
            const uint32_t n = n_list[which];
            uint64_t m = __ballot(v.w != 0);
            uint32_t sz = 0;
            if (v.w) {
                uint32_t at = n + (uint32_t)__popcll(m & lt); w.u.sai.sp[which][at] = v.x; w.u.sai.ep[which][at] = v.y; w.u.sai.off[which][at] = v.z | (v.w == 2 ? 0x80000000u : 0u);
                sz = v.y - v.x + 1u;
                if (which == 1 && !PE) { uint32_t skip = sz / 0x40000u; if (skip > 1) sz = (sz + skip - 1) / skip; }
                if (PE && which == 0 && sz > ap.max_locate + 1u) sz = ap.max_locate + 1u;              // rows the per-interval cap lets through (alnse.c:523)
                if (PE && which == 1 && v.y - v.x > ap.max_locate) sz = (v.y - v.x) / ((v.y - v.x) / ap.max_locate) + 1u;   // rows the subsampling visits
                if (sz > cap_total) sz = cap_total + 1u;
            }
            for (int o = 32; o > 0; o >>= 1) sz += (uint32_t)__shfl_xor((int)sz, o);
            rows = rows + sz > cap_total ? cap_total + 1u : rows + sz;
            n_list[which] = n + (uint32_t)__popcll(m);
        }
    }
    WSYNC();
    // The reference orders both lists by interval size (alnse.c:307-308, klib introsort).  The order only decides WHICH
    // rows are located before a cap stops the loops; when every row is located the loci are the same set, and they
    // are sorted right after -- so the replica of the sort runs only when the cap can bite.
    if (rows > cap_total) {
        if (W::N_SLOTS <= 64 || (n_list[0] <= 64u && n_list[1] <= 64u)) {     // in lanes: the C list, then the R list (the usual shape has no other form)
#pragma unroll
            for (int which = 0; which < 2; ++which)
                sai_introsort_lanes((lds_u32w)w.u.sai.sp[which], (lds_u32w)w.u.sai.ep[which], (lds_u32w)w.u.sai.off[which], (int)n_list[which]);
        } else if (lane < 2) { SaiLists sl = sai_ref(w.u.sai); sai_introsort_lds(sl, (int)lane, (int)n_list[lane]); }
    }
    // a PE mate may enumerate 0x40000 loci, which need the global scratch; the usual few hundred stay in LDS like an SE read's (the
    // verify and rule passes then pay one memory round trip per trip instead of two or three)
    const bool pe_in_lds = !glob || rows <= (uint32_t)MAXLOC;
    if (pe_in_lds) loci = w.loci;
    WSYNC();
    pc.stamp(SALT_CTR_T_GATHER);
    // locate: SE under the global max_locate cap (alnse_locate_alt, alnse.c:633-731); PE with the per-interval cap
    // and the 0x40000 global cap of alnse_locate (alnse.c:501-629; here bounded by the scratch capacity)
    uint32_t n = 0, ns = 0, n_ctx_rows = 0;                   // rows that count against the cap; rows stored (ns < n only with the context table)
    bool full = false;
    const gp_u32x4 c_ctx = as_global(a.c_ctx);
    const bool use_ctx = a.c_ctx != nullptr && !gap_mode;             // paired end too: a rejected row counts against both caps like any row (alnse.c:523-533)
    for (uint32_t i = 0; i < n_list[0] && !full; ++i) {
        const uint32_t sp = w.u.sai.sp[0][i], off = w.u.sai.off[0][i] & 0x7FFFFFFFu;
        const bool located = (w.u.sai.off[0][i] >> 31) != 0;                  // k_seed resolved this one-row interval to its position
        uint32_t ep = w.u.sai.ep[0][i];
        if (PE && ep - sp > ap.max_locate) ep = sp + ap.max_locate;             // j - sp <= max_locate (alnse.c:523)
        const bool ctx_here = use_ctx && !located;
        CtxRead rd = { 0, 0, 0 };
        if (ctx_here) rd = ctx_read(w.pm[strand], L, off, a.ctx_k);
        for (uint64_t j0 = sp; j0 <= ep && !full; j0 += 64) {
            pc.add(SALT_CTR_X0, 1);
            uint64_t j = j0 + lane;
            bool in = j <= ep, keep = false, rej = false;
            uint32_t pos = 0;
            if (in) {
                uint32_t sa;
                if (ctx_here) { const u32x4_t rc = c_ctx[j]; sa = rc.x; rej = ctx_reject(make_uint4(rc.x, rc.y, rc.z, rc.w), rd, 3u); }
                else sa = located ? (uint32_t)j : ix.c_sa[j];
                pos = sa - off; keep = !(pos + L > ix.ref_len);                 // u32 wrap as in alnse.c:672-673
            }
            uint64_t m = __ballot(keep);
            uint32_t rank = (uint32_t)__popcll(m & lt);
            const bool st = keep && !rej && n + rank < cap_total;              // inside the cap and not ruled out by its context
            const uint64_t ms = __ballot(st);
            if (st) loci[ns + (uint32_t)__popcll(ms & lt)] = pos;
            ns += (uint32_t)__popcll(ms);
            uint32_t tot = (uint32_t)__popcll(m);
            if (n + tot >= cap_total) {
                // lookups the sequential loop would have made before stopping
                uint64_t last = m;                       // position of the cap_total-th kept lane
                uint32_t need = cap_total - n;           // >= 1
                for (uint32_t q = 1; q < need; ++q) last &= last - 1;
                uint32_t stop_lane = (uint32_t)__ffsll((long long)last) - 1;
                n_sa_c += stop_lane + 1; if (ctx_here) n_ctx_rows += stop_lane + 1;
                n = cap_total; full = true;
            } else { n += tot; const uint32_t looked = (uint32_t)__popcll(__ballot(in)); n_sa_c += looked; if (ctx_here) n_ctx_rows += looked; }
        }
    }
    pc.stamp(SALT_CTR_X2);
    const gp_u32x4 r_ctx = as_global(a.r_ctx);
    const bool use_rctx = use_ctx && a.r_ctx != nullptr;
    for (uint32_t i = 0; i < n_list[1] && !full; ++i) {
        const uint32_t sp = w.u.sai.sp[1][i], ep = w.u.sai.ep[1][i], off = w.u.sai.off[1][i];
        uint32_t skip = (ep + 1 - sp) / 0x40000u;                                       // alnse.c:707-708
        if ((int)skip <= 0) skip = 1;
        // PE: an interval wider than max_locate is subsampled with rand() in the reference (alnse.c:587-595), i.e. its
        // result is not defined; the stand-in keeps the first row of every block of (ep-sp)/max_locate rows
        if (PE) skip = ep - sp > ap.max_locate ? (ep - sp) / ap.max_locate : 1;
        CtxRead rd = { 0, 0, 0 };
        if (use_rctx) rd = ctx_read(w.pm[strand], L, off, a.ctx_k);
        for (uint64_t j0 = sp; j0 <= ep && !full; j0 += 64ull * skip) {
            pc.add(SALT_CTR_X1, 1);
            uint64_t j = j0 + (uint64_t)lane * skip;
            bool in = j <= ep, keep = false, rej = false;
            uint32_t pos = 0;
            if (in) {
                uint32_t rp;
                if (use_rctx) { const u32x4_t rc = r_ctx[j]; rp = rc.x; rej = ctx_reject(make_uint4(rc.x, rc.y, rc.z, rc.w), rd, 3u); }
                else rp = ix.r_pos[j];
                pos = rp - off; keep = !(pos > ix.ref_len || pos + L > ix.ref_len);      // alnse.c:715-717
            }
            uint64_t m = __ballot(keep);
            uint32_t rank = (uint32_t)__popcll(m & lt);
            const bool st = keep && !rej && n + rank < cap_total;                       // inside the cap and not ruled out by its context
            const uint64_t ms = __ballot(st);
            if (st) loci[ns + (uint32_t)__popcll(ms & lt)] = pos;
            ns += (uint32_t)__popcll(ms);
            uint32_t tot = (uint32_t)__popcll(m);
            if (n + tot >= cap_total) {
                uint64_t last = m; uint32_t need = cap_total - n;
                for (uint32_t q = 1; q < need; ++q) last &= last - 1;
                const uint32_t looked = (uint32_t)__ffsll((long long)last);
                n_sa_r += looked; if (use_rctx) n_ctx_rows += looked;
                n = cap_total; full = true;
            } else { n += tot; const uint32_t looked = (uint32_t)__popcll(__ballot(in)); n_sa_r += looked; if (use_rctx) n_ctx_rows += looked; }
        }
    }
    const uint32_t n_ctx_rej = n - ns;
    n_loci_out += n;
    n = ns;                                                   // what the passes below see
    WSYNC();
    bool in_lds = pe_in_lds;
    if (glob && !in_lds && n <= (uint32_t)MAXLOC) {
        // the rows that were ENUMERATED outgrew the LDS list, the rows the context table let through do not: bring them in (one trip now
        // instead of two or three per verify / rule pass)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        for (uint32_t i = lane; i < n; i += 64) w.loci[i] = loci[i];
        loci = w.loci; in_lds = true;
        WSYNC();
    }
    pc.stamp(SALT_CTR_T_LOCATE);
    if (!a.finish) return CandStats{ n, n_sa_c, n_sa_r, n_loci_out, in_lds ? 1u : 0u, n_ctx_rej, n_ctx_rows };
    sort_loci(loci, n);
    WSYNC();
    pc.stamp(SALT_CTR_T_SORT);
    const uint32_t n_out = dedup_loci(loci, n, gap_mode, L, ix.ref_len);
    pc.stamp(SALT_CTR_T_DEDUP);
    return CandStats{ n_out, n_sa_c, n_sa_r, n_loci_out, in_lds ? 1u : 0u, n_ctx_rej, n_ctx_rows };
}

template <bool PE, bool GL, class W>
__device__ __forceinline__ CandStats build_candidates_call(const CandArgs a, W &w)
{
    static_assert(sizeof(CandArgs) <= sizeof(w.cargs), "CandArgs outgrew its LDS slot");
    WSYNC();
    if (lane_id() == 0) *reinterpret_cast<CandArgs *>(w.cargs) = a;
    WSYNC();
    return build_candidates<PE, GL, W>(w);
}

// ---- masked Hamming distance, capped: returns 0..3 or INF (ed_mismatch, editdistance.c:88-163) ----
__device__ __forceinline__ uint32_t mismatch_capped(const IndexView &ix, const uint32_t *pm, uint32_t L, uint32_t pos)
{
    // a locate whose `pos - offset` wrapped below 0 survives the range check the way it does in the reference (alnse.c:672-673) and is
    // only dropped by the candidate rule (pos >= mixRef.l, alnse.c:762): it must not be used as an address
    if (pos >= ix.ref_len) return INF;
    const uint32_t nw = (L + 7) >> 3, w0 = pos >> 3, sh = (pos & 7u) * 4u;
    const uint32_t *ref = ix.ref + w0;
    uint32_t lo = ref[0], mism = 0;
    for (uint32_t j = 0; j < nw; ++j) {
        uint32_t hi = ref[j + 1];
        uint32_t rw = sh ? ((lo >> sh) | (hi << (32 - sh))) : lo;
        uint32_t x = rw & pm[j];
        uint32_t nz = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u;
        uint32_t rem = L - j * 8;
        uint32_t vm = rem >= 8 ? 0x11111111u : (0x11111111u >> (4 * (8 - rem)));
        mism += (uint32_t)__popc(vm) - (uint32_t)__popc(nz & vm);
        lo = hi;
    }
    return mism > 3 ? INF : mism;
}

// ---- masked Hamming distance, four lanes per candidate -------------------------------------------
// Each lane of a quad loads 16 contiguous bytes of the candidate's window (one dwordx4), so a wave-wide
// load touches 16 candidates x 64 B instead of 64 lanes x 14 scattered dwords: ~8x fewer cache-line
// lookups per candidate in the texture-address path, which is what bounds this stage.
// Needs (L+7)/8 + 1 <= 16 words, i.e. L <= 120.  Writes min(count, INF) for candidates [0, n) to out[].
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// mismatches of one candidate, computed by its 4 lanes (sub = 0..3 holds words 4*sub..4*sub+3 of the window).
// pmw: the read's one-hot words of this lane (zero past the read's end), nvalid: bases of the read inside them.
// A base matches when (reference mask & one-hot) != 0 (ed_mismatch, editdistance.c:88-163); matches are counted
// per nibble with one add (bit 3 of (n & 7) + 7 | n is set iff the nibble n is non-zero) and subtracted from nvalid.
// LN = 4 lanes per candidate cover 16 window words (reads up to 120 bases), LN = 8 cover 32 (up to 248 bases: 150-bp mates).
template <int LN = 4>
__device__ __forceinline__ uint32_t quad_mismatch(const u32x4_a4 x, const uint32_t pos, const uint32_t (&pmw)[4], const uint32_t nvalid)
{
    const uint32_t sh = (pos & 7u) * 4u;
    const uint32_t nxt = (uint32_t)__shfl_down((int)x.x, 1);             // first word of the next lane of the quad
    const uint32_t xs[5] = { x.x, x.y, x.z, x.w, nxt };
    uint32_t match = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t w = __funnelshift_r(xs[t], xs[t + 1], sh);        // window word: reference nibbles pos+8j .. pos+8j+7
        const uint32_t y = w & pmw[t];
        match += (uint32_t)__popc((((y & 0x77777777u) + 0x77777777u) | y) & 0x88888888u);
    }
    uint32_t mism = nvalid - match;
    mism += (uint32_t)__shfl_xor((int)mism, 1);
    mism += (uint32_t)__shfl_xor((int)mism, 2);
    if (LN == 8) mism += (uint32_t)__shfl_xor((int)mism, 4);
    return mism;
}

template <int G, int LN = 4>                                             // groups of 64 / LN candidates whose loads are in flight together
__device__ __forceinline__ void verify_quads(const uint32_t *__restrict__ ref, uint32_t ref_len, const uint32_t *pm, uint32_t L,
                                             const uint32_t *cand, uint32_t n, uint8_t *out)
{
    constexpr uint32_t CPW = 64u / LN;                                   // candidates per wave-wide load
    const uint32_t lane = lane_id(), sub = lane & (uint32_t)(LN - 1), q = lane / (uint32_t)LN;
    const uint32_t nw = (L + 7) >> 3;
    const uint32_t nvalid = L > 32u * sub ? (L - 32u * sub < 32u ? L - 32u * sub : 32u) : 0u;
    uint32_t pmw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) pmw[t] = (4 * sub + t) < nw ? pm[4 * sub + t] : 0u;
    for (uint32_t c0 = 0; c0 < n; c0 += CPW * G) {                      // up to G groups of CPW candidates per trip
        uint32_t pos[G]; u32x4_a4 x[G]; bool act[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (c0 + CPW * g >= n) break;                                // (uniform) nothing left for this group
            const uint32_t c = c0 + CPW * g + q;
            act[g] = c < n;
            pos[g] = act[g] ? cand[c] : 0u;
            if (pos[g] >= ref_len) pos[g] = 0xFFFFFFFFu;                 // wrapped below 0 (see mismatch_capped): no load, INF
            x[g] = *reinterpret_cast<const u32x4_a4 *>(ref + ((pos[g] == 0xFFFFFFFFu ? 0u : pos[g]) >> 3) + 4 * sub);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (c0 + CPW * g >= n) break;
            const uint32_t mism = quad_mismatch<LN>(x[g], pos[g], pmw, nvalid);
            if (act[g] && sub == 0) out[c0 + CPW * g + q] = (uint8_t)((mism > 3 || pos[g] == 0xFFFFFFFFu) ? INF : mism);
        }
    }
}

// Reads of 121 .. 248 bases (150-base mates), two phases.  A window is 76+ bytes: eight lanes per candidate move 128 (two or three
// 64-byte sectors), and nearly every located row of a repeat read is a false one.  Phase 1 looks at the first 120 bases only -- four
// lanes, one 64-byte stretch per candidate, 128 candidates in flight: a candidate with more than 3 mismatches there cannot pass
// ed_mismatch(..., 3) (editdistance.c:88-163 counts over the whole read).  Phase 2 counts the few survivors over the whole read with
// eight lanes each.  Same out[] as verify_quads<G, 8>.
__device__ __forceinline__ void verify_two_phase(const uint32_t *__restrict__ ref, uint32_t ref_len, const uint32_t *pm, uint32_t L,
                                                 const uint32_t *cand, uint32_t n, uint8_t *out)
{
    verify_quads<8, 4>(ref, ref_len, pm, 120u, cand, n, out);                  // partial counts (<= 3) or INF
    WSYNC();
    const uint32_t lane = lane_id(), sub = lane & 7u, q = lane >> 3;
    const uint32_t nw = (L + 7) >> 3;
    const uint32_t nvalid = L > 32u * sub ? (L - 32u * sub < 32u ? L - 32u * sub : 32u) : 0u;
    uint32_t pmw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) pmw[t] = (4 * sub + t) < nw ? pm[4 * sub + t] : 0u;
    const bool need = 4u * sub < nw + 1u;                                    // this lane's words overlap the window (the rest is never fetched)
    for (uint32_t b = 0; b < n; b += 64) {
        const uint32_t i = b + lane;
        uint64_t m = __ballot(i < n && out[i] != INF);
        while (m) {                                                          // (uniform) eight survivors per trip, one per lane group
            uint64_t mm = m; uint32_t c = 0xFFFFFFFFu;
            for (uint32_t k = 0; k < 8; ++k) {                               // group q takes the q-th survivor
                if (!mm) break;
                const uint32_t bit = (uint32_t)__ffsll((long long)mm) - 1u;
                if (k == q) c = b + bit;
                mm &= mm - 1;
            }
            m = mm;
            const bool act = c != 0xFFFFFFFFu;
            uint32_t pos = act ? cand[c] : 0u;
            if (pos >= ref_len) pos = 0xFFFFFFFFu;                           // (cannot survive phase 1; kept for symmetry with verify_quads)
            u32x4_a4 x = { 0u, 0u, 0u, 0u };
            if (act && need && pos != 0xFFFFFFFFu) x = *reinterpret_cast<const u32x4_a4 *>(ref + (pos >> 3) + 4 * sub);
            const uint32_t mism = quad_mismatch<8>(x, pos, pmw, nvalid);
            if (act && sub == 0) out[c] = (uint8_t)((mism > 3 || pos == 0xFFFFFFFFu) ? INF : mism);
        }
    }
}

// ---- lane groups ------------------------------------------------------------------------------
// The light kernels give a read a whole wave (GW = 64), one of its halves (GW = 32: two reads per wave, each on its own) or one of
// its quarters (GW = 16: four).  What such a group asks of its lanes, all of it settled at compile time: the lane inside the group; a
// ballot over the group (64: the wave's mask; 32: this half's 32 bits of it, by a select and not a 64-bit shift; 16: this quarter's
// 16 bits of that half); a broadcast from a group lane (64: v_readlane, the index is wave-uniform; 32 / 16: a shuffle from the
// group's base); the lanes-below mask; the group-wide add.
__device__ __forceinline__ uint32_t popc(uint32_t m) { return (uint32_t)__popc(m); }
__device__ __forceinline__ uint32_t popc(uint64_t m) { return (uint32_t)__popcll(m); }
__device__ __forceinline__ int first_bit(uint32_t m) { return __ffs((int)m) - 1; }
__device__ __forceinline__ int first_bit(uint64_t m) { return __ffsll((long long)m) - 1; }
template <int GW> struct LaneGroup {
    static_assert(GW == 64 || GW == 32 || GW == 16, "a wave, half of one or a quarter");
    typedef std::conditional_t<GW == 64, uint64_t, uint32_t> mask_t;
    static __device__ __forceinline__ uint32_t lane() { return lane_id() & (uint32_t)(GW - 1); }
    static __device__ __forceinline__ mask_t ballot(bool x)
    {
        const uint64_t m = __ballot(x);
        if constexpr (GW == 64) return m;
        else {
            const uint32_t h = (lane_id() & 32u) ? (uint32_t)(m >> 32) : (uint32_t)m;
            if constexpr (GW == 32) return h; else return (h >> (lane_id() & 16u)) & 0xFFFFu;
        }
    }
    static __device__ __forceinline__ uint32_t bcast(uint32_t v, int src)
    {
        if constexpr (GW == 64) return (uint32_t)__builtin_amdgcn_readlane((int)v, src);
        else return (uint32_t)__shfl((int)v, (int)(lane_id() & (uint32_t)(64 - GW)) + src);
    }
    static __device__ __forceinline__ mask_t below() { return ((mask_t)1 << lane()) - (mask_t)1; }
    static __device__ __forceinline__ uint32_t sum(uint32_t v)
    {
        for (int o = GW / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
        return v;
    }
};

// Both strands of one read in the same trips (the light kernels): candidates c0[0..n0) use pm0, c1[0..n1) use pm1.  A group of GW
// lanes works on them, GW / LN rows per group of loads, four groups of loads in flight.
template <int LN = 4, int GW = 64>
__device__ __forceinline__ void verify_quads_2(const uint32_t *__restrict__ ref, uint32_t ref_len, const uint32_t *pm0, const uint32_t *pm1, uint32_t L,
                                               const uint32_t *c0, uint32_t n0, const uint32_t *c1, uint32_t n1, uint8_t *o0, uint8_t *o1)
{
    constexpr uint32_t CPW = (uint32_t)GW / LN;
    const uint32_t lane = LaneGroup<GW>::lane(), sub = lane & (uint32_t)(LN - 1), q = lane / (uint32_t)LN;
    const uint32_t nw = (L + 7) >> 3, n = n0 + n1;
    const uint32_t nvalid = L > 32u * sub ? (L - 32u * sub < 32u ? L - 32u * sub : 32u) : 0u;
    // A lane whose words lie behind the window fetches nothing.  Its pattern words are zero, so the counts are the same with and without
    // this, at either width; it stays with the one instantiation that had it (two 150-base reads a wave), so that the others compile to
    // what they were.
    const bool behind = LN == 8 && GW == 32 && !(4u * sub < nw + 1u);
    uint32_t pa[4], pb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { const bool in = (4 * sub + t) < nw; pa[t] = in ? pm0[4 * sub + t] : 0u; pb[t] = in ? pm1[4 * sub + t] : 0u; }
    for (uint32_t b = 0; b < n; b += 4u * CPW) {
        uint32_t pos[4]; u32x4_a4 x[4]; bool act[4], rev[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (b + CPW * g >= n) break;
            const uint32_t c = b + CPW * g + q;
            act[g] = c < n; rev[g] = c >= n0;
            pos[g] = act[g] ? (rev[g] ? c1[c - n0] : c0[c]) : 0u;
            if (pos[g] >= ref_len) pos[g] = 0xFFFFFFFFu;                 // wrapped below 0 (see mismatch_capped): no load, INF
            if (behind) x[g] = u32x4_a4{ 0u, 0u, 0u, 0u };
            else x[g] = *reinterpret_cast<const u32x4_a4 *>(ref + ((pos[g] == 0xFFFFFFFFu ? 0u : pos[g]) >> 3) + 4 * sub);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (b + CPW * g >= n) break;
            const uint32_t pw[4] = { rev[g] ? pb[0] : pa[0], rev[g] ? pb[1] : pa[1], rev[g] ? pb[2] : pa[2], rev[g] ? pb[3] : pa[3] };
            const uint32_t mism = quad_mismatch<LN>(x[g], pos[g], pw, nvalid);
            if (act[g] && sub == 0) {
                const uint32_t c = b + CPW * g + q;
                const uint8_t v = (uint8_t)((mism > 3 || pos[g] == 0xFFFFFFFFu) ? INF : mism);
                if (rev[g]) o1[c - n0] = v; else o0[c] = v;
            }
        }
    }
}

// ---- Landau-Vishkin on byte masks, one diagonal per lane ---------------------------------------
// T: text masks (tlen bytes, zero padded), P: one-hot pattern (plen bytes, zero padded).
// Returns e (<= k), or -1.  When tab.L != nullptr also fills the L / action tables and returns the
// finishing diagonal in d_fin (order 0,-1,1,... LandauVishkin.c:248); otherwise the order is
// irrelevant for the distance (LandauVishkin.c:67).  (Both come back by value: a reference into the caller's frame was scratch.)
struct LvEnd { int e, d_fin; };
__device__ __attribute__((noinline)) LvEnd lv_wave(const uint8_t *T, int tlen, const uint8_t *P, int plen, int k, const LvTabRef tab)
{
    int d_fin = 0;
    const int lane = (int)lane_id();
    const int d = lane - 31;
    const int ad = d < 0 ? -d : d;
    int Lprev = -2;
    const int end0 = plen < tlen ? plen : tlen;
    if (d == 0) { int i = 0; while (i < end0 && (P[i] & T[i]) != 0) ++i; Lprev = i; }
    const int r0 = __shfl(Lprev, 31);
    if (tab.L) tab.L[lane] = (short)Lprev;
    if (r0 == end0) return LvEnd{ plen > end0 ? plen - end0 : 0, 0 };
    if (k > LVK - 1) k = LVK - 1;
    for (int e = 1; e <= k; ++e) {
        int left = __shfl_up(Lprev, 1), right = __shfl_down(Lprev, 1);
        if (lane == 0) left = -2;
        if (lane == 63) right = -2;
        const bool active = ad <= e && ad <= LVK - 1;
        int best = Lprev + 1; char act = 'X';
        if (left > best) { best = left; act = 'D'; }
        if (right + 1 > best) { best = right + 1; act = 'I'; }
        int cur = -2;
        if (active) {
            if (P[best] == T[d + best]) {                     // equality gate (LandauVishkin.c:79,264)
                int end = plen < tlen - d ? plen : tlen - d;
                if (best >= end) best = end;
                else { int i = best; while (i < end && (P[i] & T[d + i]) != 0) ++i; best = i; }
            }
            cur = best;
        }
        if (tab.L) { tab.L[e * 64 + lane] = (short)cur; tab.A[e * 64 + lane] = act; }
        uint64_t reach = __ballot(active && cur == plen);
        if (reach) {
            if (tab.L) {
                // first finishing diagonal in the order 0,-1,1,-2,2,...
                int rank = d == 0 ? 0 : (d < 0 ? 2 * ad - 1 : 2 * ad);
                int my = (active && cur == plen) ? rank : 1000;
                for (int o = 32; o > 0; o >>= 1) { int t = __shfl_xor(my, o); my = t < my ? t : my; }
                d_fin = my == 0 ? 0 : ((my & 1) ? -((my + 1) >> 1) : (my >> 1));
            }
            return LvEnd{ e, d_fin };
        }
        Lprev = cur;
    }
    return LvEnd{ -1, 0 };
}

// ---- Landau-Vishkin distance, one candidate per lane (computeEditDistance, LandauVishkin.c:19-122) ----
// Text: the lane's (L+4)-base window of the mixRef, nibble-packed and word-major in s.T (lane_text: zero beyond tlen, like the
// reference's zero-padded byte buffer); pattern: the read's one-hot nibbles (N = 15) behind pm, a per-lane LDS address that
// lane_pattern filled (all lanes the same one in k_gap and k_heavy).  plen + LLV_WIN == tlen <= 8 * (LLV_TW - 1), k <= LLV_K.
// Returns e in 0..k, or 255 for "more than k" / inactive lanes.  The distance does not depend on the diagonal order, so all lanes walk
// the (e, d) cells in the same order: e and d are wave-uniform, the d loop is unrolled over -LLV_K .. LLV_K under a scalar |d| <= e
// test, and the row of furthest-reaching values is LLV_W registers updated in place (cell d of level e needs cells d - 1, d, d + 1
// of level e - 1: the old d - 1 is carried).  A step is one fetch of two pattern and two text words -- both operands are LDS-typed
// and padded, so nothing is predicated -- which serves the equality gate (LandauVishkin.c:79) and the first eight bases of the extension.
__device__ __attribute__((noinline)) uint32_t lv_lanes(LaneLv &s, const uint32_t *pm, int plen, int tlen, int k, bool active)
{
    constexpr int LLV_W = 2 * LLV_K + 1;                 // diagonals -LLV_K .. LLV_K
    const int lane = (int)lane_id() & (LLV_N - 1);      // callers pass active = false for lanes >= LLV_N
    const lds_u32 T = as_lds(s.T) + lane, P = as_lds(pm);
    // 8 nibbles of the pattern from base i and of the text from base t
    auto fetch = [&](int i, int t, uint32_t &p, uint32_t &x) {
        const lds_u32 pp = P + (i >> 3), tt = T + (t >> 3) * LLV_N;
        const uint32_t p0 = pp[0], p1 = pp[1], t0 = tt[0], t1 = tt[LLV_N];
        p = __funnelshift_r(p0, p1, 4u * (uint32_t)(i & 7));
        x = __funnelshift_r(t0, t1, 4u * (uint32_t)(t & 7));
    };
    // leading bases that match among the 8 of p / x: a base matches when mask & one-hot != 0 (LandauVishkin.c:42-53,85-96)
    auto run_of = [](uint32_t p, uint32_t x) -> int {
        const uint32_t y = p & x;
        const uint32_t z = ~(((y & 0x77777777u) + 0x77777777u) | y) & 0x88888888u;     // bit 3 of a nibble: no match there
        return z ? __builtin_ctz(z) >> 2 : 8;
    };
    // the furthest base on diagonal d from `best`: behind the equality gate when `gated` (levels >= 1), min(end, first mismatch)
    auto reach = [&](int d, int best, bool gated) -> int {
        uint32_t p, x;
        fetch(best, d + best, p, x);
        const int end = plen < tlen - d ? plen : tlen - d;
        const bool open = !gated || ((p ^ x) & 15u) == 0;
        int run = run_of(p, x), i = best + run;
        if (open && run == 8) while (i < end) { fetch(i, d + i, p, x); run = run_of(p, x); i += run; if (run < 8) break; }
        i = i < end ? i : end;                            // best >= end included: the reference sets end there
        return open ? i : best;
    };
    int row[LLV_W];
#pragma unroll
    for (int j = 0; j < LLV_W; ++j) row[j] = -2;
    const int end0 = plen < tlen ? plen : tlen;
    uint32_t result = 255;
    bool done = !active;
    if (active) {
        const int i = reach(0, 0, false);
        row[LLV_K] = i;
        if (i == end0) { result = (uint32_t)(plen > end0 ? plen - end0 : 0); done = true; }
    }
    for (int e = 1; e <= k; ++e) {
        if (__ballot(!done) == 0) break;
        int carry = -2;                                   // cell d - 1 of the level before
#pragma unroll
        for (int d = -LLV_K; d <= LLV_K; ++d) {
            if ((d < 0 ? -d : d) > e) continue;
            const int mid = row[d + LLV_K], right = d < LLV_K ? row[d + LLV_K + 1] : -2;
            int best = mid + 1;
            if (carry > best) best = carry;
            if (right + 1 > best) best = right + 1;
            carry = mid;
            if (!done) {
                best = reach(d, best, true);
                if (best == plen) { result = (uint32_t)e; done = true; }
                else row[d + LLV_K] = best;
            }
        }
    }
    return result;
}

// ---------------------------------------------------------------------------------------------
// The reference's candidate loop (code_kmismatch alnse.c:348-369 / code_kdiff alnse.c:371-393) walks the SORTED,
// duplicate-free list: a candidate with distance v counts iff v <= the running bound, the bound drops to the smallest
// distance seen, the first such candidate and every strictly better one become the best, and the first NHIT that
// count are kept as hits.  Equivalently, with P = {candidates with v <= bound_in, inside the reference}:
//   a candidate counts        iff  no member of P at a smaller position has a smaller distance,
//   best                      =    the smallest position among the members of P with the minimal distance,
//   hits                      =    the NHIT smallest distinct positions that count, a0 = the distance of the first.
// None of this needs the list sorted or free of duplicates (equal positions have equal distances), so the kernels run it
// on the located rows as they come: per distance t the smallest position minpos[t] over P (one wave reduction each), then
// "counts" is  pos < min(minpos[0..v-1]),  and the hits are extracted by repeated minimum.
// pos / val: n entries in LDS or global memory; val > VMAX = no candidate.  GAPF: alnse_check_withgap's range filter.
// B: trips of 64 rows asked for together.  1 = a trip is loaded where it is used (lists in LDS); above 1 the list lies in global
// memory, where a trip is a round trip to L2 or HBM and a repeat read's ~900 rows were 15 of them in a row: list_trips keeps two
// batches of B trips in flight, and the caller may have asked for the first batch already (`first`: rows_fetch at row 0).
// ---------------------------------------------------------------------------------------------
template <int B> struct RowBatch { uint32_t p[B], v[B]; };
static constexpr int GAPFIN_B = 8;               // k_gapfin: 512 rows a batch, a repeat read's strand (~900 rows, 1 000 at the cap) in two
// rows b + 64 j + lane (j < B) of a list of n rows; the lanes behind the list's end load nothing and get "no candidate"
template <int B>
__device__ __forceinline__ void rows_fetch(RowBatch<B> &r, const uint32_t *pos, const uint8_t *val, const uint32_t n, const uint32_t b)
{
    const uint32_t lane = lane_id();
#pragma unroll
    for (int j = 0; j < B; ++j) {                                     // one lane offset and an immediate per load: nothing here waits
        const uint32_t i = b + 64u * (uint32_t)j + lane;
        r.p[j] = 0; r.v[j] = 0xFFFFFFFFu;
        if (i < n) { r.p[j] = pos[i]; r.v[j] = val[i]; }
    }
}
// trip(i, p, v) for every trip of the list, i = the lane's row (p = 0, v = NONE behind the end)
// TWO: the batch behind the one in use is in flight as well (the first pass; the hit passes of a list with more than 64 members
// inside the bound are rare and take a batch at a time, for the registers)
template <int B, bool TWO, class F>
__device__ __forceinline__ void list_trips(const uint32_t *pos, const uint8_t *val, const uint32_t n, const RowBatch<B> *first, F trip)
{
    const uint32_t lane = lane_id();
    if constexpr (B == 1) {
        for (uint32_t b = 0; b < n; b += 64) {
            const uint32_t i = b + lane;
            uint32_t p = 0, v = 0xFFFFFFFFu;
            if (i < n) { p = pos[i]; v = val[i]; }
            trip(i, p, v);
        }
    } else {
        if (n == 0) return;
        RowBatch<B> cur;
        if (first) cur = *first; else rows_fetch<B>(cur, pos, val, n, 0u);
        for (uint32_t b = 0; b < n; b += 64u * B) {
            RowBatch<B> nxt;
            const bool more = b + 64u * B < n;
            if (TWO && more) rows_fetch<B>(nxt, pos, val, n, b + 64u * B);   // in flight while this batch is used
#pragma unroll
            for (int j = 0; j < B; ++j) if (b + 64u * (uint32_t)j < n) trip(b + 64u * (uint32_t)j + lane, cur.p[j], cur.v[j]);
            if (more) { if (TWO) cur = nxt; else rows_fetch<B>(cur, pos, val, n, b + 64u * B); }
        }
    }
}
template <int VMAX, bool GAPF, int B = 1>
__device__ __forceinline__ void rule_unsorted(const uint32_t *pos, const uint8_t *val, const uint32_t n, const uint32_t L, const uint32_t ref_len,
                                              uint32_t &bound, bool &any, uint32_t &best_pos, uint32_t &best_v,
                                              uint32_t &n_hits, uint32_t &a0, uint32_t *hit_pos, uint8_t *hit_nd,
                                              const RowBatch<B> *first = nullptr)
{
    const uint32_t lane = lane_id();
    const uint32_t NONE = 0xFFFFFFFFu;
    auto in_range = [&](uint32_t p) -> bool { return GAPF ? !(p + L + 4 >= ref_len) : p < ref_len; };
    uint32_t mp[VMAX + 1];
#pragma unroll
    for (int t = 0; t <= VMAX; ++t) mp[t] = NONE;
    // The members of P are few (a repeat read's list: ~900 located rows, a handful inside the bound), and the hits below are six more
    // passes over whatever they are taken from: while P has at most 64 members, member k is copied to lane k (scalar steps per member,
    // none for a trip without one) and the hit passes run on that register copy instead of the list.
    uint32_t my_p = 0, my_v = NONE, n_p = 0;                      // n_p > 64: P outgrew the lanes, the passes walk the list
    list_trips<B, true>(pos, val, n, first, [&](const uint32_t i, const uint32_t p, const uint32_t v) {
        const bool in = i < n && v <= bound && in_range(p);
        if (in) {
#pragma unroll
            for (int t = 0; t <= VMAX; ++t) if (v == (uint32_t)t && p < mp[t]) mp[t] = p;
        }
        uint64_t m = __ballot(in);
        if (m && n_p <= 64u) {
            if (n_p + (uint32_t)__popcll(m) > 64u) n_p = 65u;
            else
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    const uint32_t pl = (uint32_t)__builtin_amdgcn_readlane((int)p, l), vl = (uint32_t)__builtin_amdgcn_readlane((int)v, l);
                    if (lane == n_p) { my_p = pl; my_v = vl; }
                    ++n_p; m &= m - 1;
                }
        }
    });
#pragma unroll
    for (int t = 0; t <= VMAX; ++t)
        for (int o = 32; o > 0; o >>= 1) { const uint32_t x = (uint32_t)__shfl_xor((int)mp[t], o); mp[t] = x < mp[t] ? x : mp[t]; }
    // before[t] = smallest position of P with a distance below t
    uint32_t before[VMAX + 1];
    before[0] = NONE;
#pragma unroll
    for (int t = 1; t <= VMAX; ++t) before[t] = mp[t - 1] < before[t - 1] ? mp[t - 1] : before[t - 1];
    any = false; n_hits = 0;
#pragma unroll
    for (int t = VMAX; t >= 0; --t) if (mp[t] != NONE) { any = true; best_v = (uint32_t)t; best_pos = mp[t]; }
    if (!any) return;
    unsigned long long last = 0;
    const bool in_lanes = n_p <= 64u;
    unsigned long long my_key = ~0ull;                            // this lane's member, if it counts (p < the smallest position of a smaller distance)
    if (in_lanes && lane < n_p) {
        uint32_t lim = NONE;
#pragma unroll
        for (int t = 1; t <= VMAX; ++t) if (my_v == (uint32_t)t) lim = before[t];
        if (my_p < lim) my_key = ((unsigned long long)my_p << 8) | my_v;
    }
    for (uint32_t h = 0; h < (uint32_t)NHIT; ++h) {
        unsigned long long cur = ~0ull;
        if (in_lanes) { if (h == 0 || my_key > last) cur = my_key; }
        else
        list_trips<B, false>(pos, val, n, (const RowBatch<B> *)nullptr, [&](const uint32_t i, const uint32_t p, const uint32_t v) {
            if (i < n && v <= bound && in_range(p)) {
                uint32_t lim = NONE;
#pragma unroll
                for (int t = 1; t <= VMAX; ++t) if (v == (uint32_t)t) lim = before[t];
                const unsigned long long key = ((unsigned long long)p << 8) | v;
                if (p < lim && (h == 0 || key > last) && key < cur) cur = key;
            }
        });
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long x = ((unsigned long long)(uint32_t)__shfl_xor((int)(cur >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)cur, o);
            cur = x < cur ? x : cur;
        }
        if (cur == ~0ull) break;
        if (lane == 0) { hit_pos[h] = (uint32_t)(cur >> 8); hit_nd[h] = (uint8_t)(cur & 255u); }
        if (h == 0) a0 = (uint32_t)(cur & 255u);
        last = cur; ++n_hits;
    }
    bound = best_v < bound ? best_v : bound;
}

// rule_unsorted for short lists with few candidates inside the bound (the light kernels), on a group of GW lanes: lane i of the group
// holds candidates i, i + GW, ...  The reductions walk the set bits of a ballot with a broadcast each, i.e. they cost scalar
// instructions per candidate instead of six cross-lane steps per value.
template <int VMAX, bool GAPF, int GW = 64>
__device__ __forceinline__ void rule_sparse(const uint32_t *pos, const uint8_t *val, const uint32_t n, const uint32_t L, const uint32_t ref_len,
                                            uint32_t &bound, bool &any, uint32_t &best_pos, uint32_t &best_v,
                                            uint32_t &n_hits, uint32_t &a0, uint32_t *hit_pos, uint8_t *hit_nd)
{
    typedef LaneGroup<GW> G;
    typedef typename G::mask_t mask_t;
    const uint32_t lane = G::lane();
    const uint32_t NONE = 0xFFFFFFFFu;
    auto in_range = [&](uint32_t p) -> bool { return GAPF ? !(p + L + 4 >= ref_len) : p < ref_len; };
    any = false; n_hits = 0;
    if (n == 0) return;
    if (n <= (uint32_t)GW) {                                  // the usual case: every candidate inside the bound is the same locus
        uint32_t p = 0, v = NONE;
        if (lane < n) { p = pos[lane]; v = val[lane]; }
        const bool ok = v <= bound && in_range(p);
        const mask_t m = G::ballot(ok);
        if (m == 0) return;
        const int l0 = first_bit(m);
        const uint32_t p0 = G::bcast(p, l0);
        if (G::ballot(ok && p != p0) == 0) {
            const uint32_t v0 = G::bcast(v, l0);
            any = true; best_pos = p0; best_v = v0; n_hits = 1; a0 = v0;
            if (lane == 0) { hit_pos[0] = p0; hit_nd[0] = (uint8_t)v0; }
            bound = v0 < bound ? v0 : bound;
            return;
        }
    }
    uint32_t mp[VMAX + 1];
#pragma unroll
    for (int t = 0; t <= VMAX; ++t) mp[t] = NONE;
    for (uint32_t b = 0; b < n; b += GW) {
        const uint32_t i = b + lane;
        uint32_t p = 0, v = NONE;
        if (i < n) { p = pos[i]; v = val[i]; }
        mask_t m = G::ballot(v <= bound && in_range(p));
        while (m) {
            const int l = first_bit(m);
            const uint32_t pl = G::bcast(p, l), vl = G::bcast(v, l);
#pragma unroll
            for (int t = 0; t <= VMAX; ++t) if (vl == (uint32_t)t && pl < mp[t]) mp[t] = pl;
            m &= m - 1;
        }
    }
    uint32_t before[VMAX + 1];
    before[0] = NONE;
#pragma unroll
    for (int t = 1; t <= VMAX; ++t) before[t] = mp[t - 1] < before[t - 1] ? mp[t - 1] : before[t - 1];
#pragma unroll
    for (int t = VMAX; t >= 0; --t) if (mp[t] != NONE) { any = true; best_v = (uint32_t)t; best_pos = mp[t]; }
    if (!any) return;
    uint32_t last_p = 0;
    for (uint32_t h = 0; h < (uint32_t)NHIT; ++h) {
        uint32_t cur_p = NONE, cur_v = 0;
        for (uint32_t b = 0; b < n; b += GW) {
            const uint32_t i = b + lane;
            uint32_t p = 0, v = NONE;
            if (i < n) { p = pos[i]; v = val[i]; }
            uint32_t lim = NONE;
#pragma unroll
            for (int t = 1; t <= VMAX; ++t) if (v == (uint32_t)t) lim = before[t];
            mask_t m = G::ballot(v <= bound && in_range(p) && p < lim && (h == 0 || p > last_p));
            while (m) {
                const int l = first_bit(m);
                const uint32_t pl = G::bcast(p, l);
                if (pl < cur_p) { cur_p = pl; cur_v = G::bcast(v, l); }
                m &= m - 1;
            }
        }
        if (cur_p == NONE) break;
        if (lane == 0) { hit_pos[h] = cur_p; hit_nd[h] = (uint8_t)cur_v; }
        if (h == 0) a0 = cur_v;
        last_p = cur_p; ++n_hits;
    }
    bound = best_v < bound ? best_v : bound;
}

// unpack text masks / one-hot pattern for LV (editdistance.c:183-227)
template <class W>
__device__ void lv_unpack(const uint32_t *ref_generic, W &w, int strand, uint32_t L, uint32_t pos)
{
    const gp_u32 ref = as_global(ref_generic);
    const uint32_t tlen = L + 4;
    for (uint32_t i = lane_id(); i < tlen + 48; i += 64) {
        uint32_t p = pos + i;
        w.u.lvb.T[i] = i < tlen ? (uint8_t)((ref[p >> 3] >> (4 * (p & 7u))) & 15u) : (uint8_t)0;
    }
    for (uint32_t i = lane_id(); i < L + 48; i += 64) {
        w.u.lvb.P[i] = i < L ? (uint8_t)((w.pm[strand][i >> 3] >> (4 * (i & 7u))) & 15u) : (uint8_t)0;
    }
    WSYNC();
}

// CIGAR of a gapped hit into w.cig / w.n_cig (computeEditDistanceWithCigar, useM=1) ------------------
// lv_cigar_here is the body in place (k_cigar: a function that calls lv_wave from inside a call keeps a frame in scratch); lv_cigar,
// below it, is the same as a call, for the kernels that hold it beside much else.
template <class W>
__device__ __forceinline__ void lv_cigar_here(const uint32_t *ref, W &w, const LvTabRef tab, int strand, uint32_t L, uint32_t pos, int k)
{
    lv_unpack(ref, w, strand, L, pos);
    WSYNC();
    const LvEnd fin = lv_wave(w.u.lvb.T, (int)L + 4, w.u.lvb.P, (int)L, k, tab);
    const int e = fin.e, d_fin = fin.d_fin;
    __threadfence_block();
    WSYNC();
    if (lane_id() == 0) {
        int n = 0;
        uint16_t *cg = w.cig;
        if (e == 0) { cg[n++] = (uint16_t)((L << 4) | 0u); }
        else if (e > 0) {
            LvTrace &tr = *reinterpret_cast<LvTrace *>(w.u.lvb.T);
            char *act = tr.act; int *matched = tr.matched;
            int cd = d_fin;
            for (int ce = e; ce >= 1; --ce) {
                char a = tab.A[ce * 64 + cd + 31];
                act[ce] = a;
                int cur = tab.L[ce * 64 + cd + 31];
                if (a == 'I') { matched[ce] = cur - tab.L[(ce - 1) * 64 + cd + 1 + 31] - 1; cd += 1; }
                else if (a == 'D') { matched[ce] = cur - tab.L[(ce - 1) * 64 + cd - 1 + 31]; cd -= 1; }
                else { matched[ce] = cur - tab.L[(ce - 1) * 64 + cd + 31] - 1; }
            }
            int acc = tab.L[31];
            int ce = 1;
            while (ce <= e) {
                char a = act[ce]; int cnt = 1;
                while (ce + 1 <= e && matched[ce] == 0 && act[ce + 1] == a) { ++cnt; ++ce; }
                if (a == 'X') acc += cnt;
                else {
                    if (acc != 0 && n < SALT_MAX_CIGAR_OPS) { cg[n++] = (uint16_t)((acc << 4) | 0); }
                    acc = 0;
                    if (n < SALT_MAX_CIGAR_OPS) cg[n++] = (uint16_t)((cnt << 4) | (a == 'I' ? 1 : 2));
                }
                if (matched[ce] > 0) acc += matched[ce];
                ++ce;
            }
            if (acc != 0 && n < SALT_MAX_CIGAR_OPS) cg[n++] = (uint16_t)((acc << 4) | 0);
        }
        w.n_cig = n;
    }
    WSYNC();
}
template <class W>
__device__ __attribute__((noinline)) void lv_cigar(const uint32_t *ref, W &w, const LvTabRef tab, int strand, uint32_t L, uint32_t pos, int k)
{
    lv_cigar_here(ref, w, tab, strand, L, pos, k);
}

// ---------------------------------------------------------------------------------------------
// k_align
// ---------------------------------------------------------------------------------------------
// the text window of one candidate for lv_lanes: tl reference masks from pos, nibble-packed, into the lane's column of the word-major
// T (T = LaneLv::T + lane); zero past the end, over every word lv_lanes can ask for at this tl (see LLV_TS)
__device__ __forceinline__ void lane_text(const uint32_t *__restrict__ ref, uint32_t *T, uint32_t pos, uint32_t tl)
{
    const uint32_t w0 = pos >> 3, sh = (pos & 7u) * 4u, nwt = (tl + 7) >> 3, nst = ((tl - LLV_WIN + LLV_K) >> 3) + 2;
    // every word of the window is asked for before the first is used (one load, one wait, one store per word was 22 memory round trips
    // in a row per candidate)
    uint32_t wv[LLV_TW + 1];
#pragma unroll
    for (int j = 0; j <= LLV_TW; ++j) wv[j] = (uint32_t)j <= nwt ? ref[w0 + (uint32_t)j] : 0u;
#pragma unroll
    for (int j = 0; j < LLV_TW; ++j) {
        uint32_t word = 0;
        if ((uint32_t)j < nwt) {
            word = __funnelshift_r(wv[j], wv[j + 1], sh);
            const uint32_t rem = tl - (uint32_t)j * 8;
            if (rem < 8) word &= (1u << (4 * rem)) - 1u;
        }
        if ((uint32_t)j < nst) T[j * LLV_N] = word;
    }
#pragma unroll
    for (int j = LLV_TW; j < LLV_TS; ++j) if ((uint32_t)j < nst) T[j * LLV_N] = 0u;
}
// the pattern for lv_lanes: words j = first, first + step, ... of P are word(j) for j < nw and zero up to what lv_lanes can ask for
// (see LLV_PW).  The lanes of a wave share the words of one pattern (first = lane, step = 64) or a lane fills its own (0, 1).
template <class F>
__device__ __forceinline__ void lane_pattern(uint32_t *P, uint32_t nw, uint32_t first, uint32_t step, F word)
{
    for (uint32_t j = first; j < (uint32_t)LLV_PW; j += step) P[j] = j < nw ? word(j) : 0u;
}

// A read without a gap-free hit needs Landau-Vishkin over all its candidates plus LV tracebacks for its CIGARs:
// hundreds of microseconds on one wave, i.e. the tail of a persistent kernel.  k_heavy therefore only stores such a
// read's candidate lists; k_gap computes the distances with one wave per (read, strand, 32 candidates), k_gapfin
// replays the reference's sequential rule over the stored distances and writes the result, and k_cigar runs one
// traceback per wave.  (GapBufs is declared in salt_kernels.h; a read that finds no free slot is finished inline.)
__device__ __forceinline__ uint32_t store_gap_list(const uint32_t *loci, uint32_t n, uint32_t L, uint32_t ref_len, uint32_t *__restrict__ dst)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t n_out = 0;
    for (uint32_t b = 0; b < n; b += 64) {                    // the gap-free list minus alnse_check_withgap's range filter (alnse.c:894)
        const uint32_t i = b + lane;
        const uint32_t pos = i < n ? loci[i] : 0u;
        const bool keep = i < n && !(pos + L + 4 >= ref_len);
        const uint64_t m = __ballot(keep);
        if (keep) dst[n_out + (uint32_t)__popcll(m & lt)] = pos;
        n_out += (uint32_t)__popcll(m);
    }
    return n_out;
}

template <bool PE, bool GL, class W>
__device__ __forceinline__ void align_general(const IndexView ix, const AlignParams ap, W &w, const uint32_t r,
                              const uint32_t *__restrict__ pm,
                              const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r,
                              salt_result_t *__restrict__ results, unsigned long long *__restrict__ ctr,
                              unsigned long long *phase, LvTables *lvtab, const GapBufs g, uint32_t *pe_loci, uint8_t *pe_cand)
{
    const uint32_t lane = lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint32_t *rec = pm + (uint64_t)r * ap.pg.pm_stride;               // k_pack's record of this read
    const uint32_t L = rec[2 * ap.pg.nw8];
    salt_result_t *out = results + r;
    uint32_t c_sa_c = 0, c_sa_r = 0, c_verify = 0, c_vwords = 0, c_lv = 0, c_loci = 0, c_ctx_rej = 0, c_ctx_rows = 0;
    PhaseClock pc(phase);
    const uint64_t rt0 = phase ? __builtin_amdgcn_s_memrealtime() : 0;
    constexpr bool glob = GL;                                 // paired end (0x40000 loci per strand, alnse.c:42) or single end with -m above the LDS list
    uint32_t *loci = glob ? pe_loci : w.loci;                 // candidate loci: LDS, or the block's global scratch when a list outgrows it
    uint8_t *cand_e = glob ? pe_cand : w.cand_e;              // (set after every build_candidates call from what it reports)
    const uint32_t loci_cap = PE ? PE_LOCI_CAP : (uint32_t)MAXLOC;

    // ---- the read: one-hot masks of both strands, 8 bases per word, LSB first like the mixRef (editdistance.c:40) ----
    const uint32_t nw = (L + 7) >> 3;
    uint32_t n_amb = 0;
    for (uint32_t t = lane; t < 2 * nw; t += 64) {
        const uint32_t s = t >= nw, j = s ? t - nw : t;
        const uint32_t word = rec[s * ap.pg.nw8 + j];
        w.pm[s][j] = word;
        if (!s) n_amb += (uint32_t)__popc(word & (word >> 1) & (word >> 2) & (word >> 3) & 0x11111111u);     // N = all four bits
    }
    if (ap.max_amb < L) { for (int o = 32; o > 0; o >>= 1) n_amb += (uint32_t)__shfl_xor((int)n_amb, o); }
    else n_amb = 0;                                           // (uniform) the limit cannot be passed
    WSYNC();
    // result defaults (query_read_seq, query.c:199-206)
    uint32_t q_pos = 0xFFFFFFFFu; uint32_t q_strand = 3, q_ndiff = 255, q_gap = 255;
    const bool too_short = L < (uint32_t)ap.l_seed;
    if (n_amb > ap.max_amb) {                                 // alnse.c:1328 (200) / alnpe.c:495 (5): record left untouched
        if (lane == 0) {
            out->pos = q_pos; out->strand = 3; out->n_diff = 255; out->is_gap = 255; out->mapq = 0;
            out->b0 = -1; out->b1 = -1; out->seq_start = 0; out->seq_end = (uint16_t)(L - 1);
            out->n_hits[0] = out->n_hits[1] = 0; out->n_cigar = 0; out->skipped = 1;
        }
        return;
    }
    pc.stamp(SALT_CTR_T_LOAD);
    // ---- gap-free pass over both strands (alnse.c:1077-1084) ----
    uint32_t bound = 3;
    bool found[2] = { false, false };
    uint32_t n_hits_s[2] = { 0, 0 };            // hits recorded (<= NHIT) per strand
    uint32_t a0[2] = { 0, 0 };                  // n_diff of the first hit of each list
    uint32_t n_cand_nogap = 0, n_loc_s[2] = { 0, 0 };
    if (!too_short)
    for (int strand = 0; strand < 2; ++strand) {
        pc.stamp(SALT_CTR_T_SCAN);
        // Located rows first, unsorted: only loci that can pass (<= 3 mismatches, inside the reference) matter to the
        // sequential rule, so the sort (alnse.c:726-729), the duplicate filter (alnse.c:758-762) and the rule run on
        // those few; the result is the one the full sorted list gives.
        const CandStats cs = build_candidates_call<PE, GL>(CandArgs{ ix.c_sa, ix.r_pos, sai_c, sai_r, ix.ref_len, ap.spr, ap.max_locate, r, L, strand, false, phase, pe_loci, loci_cap, ap.pe, false, ap.epoch, ix.r_ctx, ix.c_ctx, ix.ctx_k }, w);
        if (glob) { loci = cs.in_lds ? w.loci : pe_loci; cand_e = cs.in_lds ? w.cand_e : pe_cand; }
        pc.t = phase ? __builtin_amdgcn_s_memtime() : 0;
        const uint32_t n_loc = cs.n_cand; c_sa_c += cs.n_sa_c; c_sa_r += cs.n_sa_r; c_loci += cs.n_loci; c_ctx_rej += cs.n_ctx_rej; c_ctx_rows += cs.n_ctx_rows;
        uint32_t call_best_n = INF, call_best_pos = 0;
        if (SALT_DIAG_VAL(ap.heavy_stop) == 1) continue;
        auto verify_all = [&](uint32_t n) {                   // cand_e[i] = min(mismatches, INF) of loci[i], loads of 128 candidates in flight
            if (L <= 120) verify_quads<8>(ix.ref, ix.ref_len, w.pm[strand], L, loci, n, cand_e);
            else if (L <= 248) verify_two_phase(ix.ref, ix.ref_len, w.pm[strand], L, loci, n, cand_e);
            else for (uint32_t i = lane; i < n; i += 64) cand_e[i] = (uint8_t)mismatch_capped(ix, w.pm[strand], L, loci[i]);
            WSYNC();
        };
        verify_all(n_loc);
        pc.stamp(SALT_CTR_T_VERIFY);
        if (SALT_DIAG_VAL(ap.heavy_stop) == 2) continue;
        {
            bool any = false; uint32_t bp = 0, bv = 0, nh = 0, a0s = 0;
            rule_unsorted<3, false>(loci, cand_e, n_loc, L, ix.ref_len, bound, any, bp, bv, nh, a0s, w.hit_pos[strand], w.hit_nd[strand]);
            if (any) {
                found[strand] = true; call_best_pos = bp; call_best_n = bv; n_hits_s[strand] = nh; a0[strand] = a0s;
                if (lane < NHIT) w.hit_gap[strand][lane] = 0;
            }
        }
        const uint32_t n_cand = n_loc;
        c_verify += n_loc; n_cand_nogap += n_loc + cs.n_ctx_rej; n_loc_s[strand] = n_loc;
        for (uint32_t b = lane; b < n_cand; b += 64) c_vwords += ((loci[b] & 7u) + L + 7) >> 3;
        if (found[strand]) { q_pos = call_best_pos; q_ndiff = call_best_n; q_gap = 0; q_strand = (uint32_t)strand; }
        WSYNC();
        pc.stamp(SALT_CTR_T_SCAN);
    }

    if (SALT_DIAG_VAL(ap.heavy_stop)) return;
    // ---- gapped pass (alnse.c:1089-1096): sequential per candidate, LV across lanes ----
    if (!too_short && !found[0] && !found[1]) {
        int maxd = PE ? 3 : (int)(L / 10);                    // alnse.c:1090 (SE) / alnse.c:1016-1028 (PE keeps 3)
        const int gap_k0 = maxd;
        const bool lanes_fit = gap_k0 <= LLV_K && L + 4 <= 8u * (LLV_TW - 1);
        if (lanes_fit && g.cap && n_cand_nogap > 0) {
            // k_gap / k_gapfin / k_cigar take it from here: both strands' located rows go to the pool as they are (unsorted,
            // duplicates included -- rule_unsorted needs neither).  Strand 1's rows are still in `loci` (unless the context table
            // thinned them: the gapped pass needs every row); strand 0's are located again.  (Single end and paired end alike.)
            uint32_t slot = 0;
            if (lane == 0) slot = atomicAdd(&g.gctl->gap_slots, 1u);
            slot = (uint32_t)__shfl((int)slot, 0);
            if (slot < g.cap) {
                uint32_t ns[2], off[2];
                bool ok = true;
                for (int k = 0; k < 2 && ok; ++k) {
                    const int strand = 1 - k;
                    uint32_t n = n_loc_s[1];
                    if (strand == 0 || ix.c_ctx != nullptr) {
                        WSYNC();
                        const CandStats cs = build_candidates_call<PE, GL>(CandArgs{ ix.c_sa, ix.r_pos, sai_c, sai_r, ix.ref_len, ap.spr, ap.max_locate, r, L, strand, true, phase, pe_loci, loci_cap, ap.pe, false, ap.epoch, nullptr, nullptr, 0 }, w);
                        if (glob) { loci = cs.in_lds ? w.loci : pe_loci; cand_e = cs.in_lds ? w.cand_e : pe_cand; }
                        c_sa_c += cs.n_sa_c; c_sa_r += cs.n_sa_r; c_loci += cs.n_loci;
                        n = cs.n_cand;
                    }
                    if (n > 1024u * LLV_N) { ok = false; break; }        // a work item names its chunk in 10 bits; PE lists can be longer
                    uint32_t o = 0;
                    if (lane == 0) o = atomicAdd(&g.gctl->pool_used, n);
                    o = (uint32_t)__shfl((int)o, 0);
                    ok = (uint64_t)o + n <= g.pool;
                    if (ok) for (uint32_t i = lane; i < n; i += 64) g.gloci[o + i] = loci[i];
                    ns[strand] = n; off[strand] = o;
                }
                const uint32_t ch0 = ok ? (ns[0] + LLV_N - 1) / LLV_N : 0, ch1 = ok ? (ns[1] + LLV_N - 1) / LLV_N : 0;
                uint32_t base = 0;
                if (ok && lane == 0) base = atomicAdd(&g.gctl->gap_items, ch0 + ch1);
                base = (uint32_t)__shfl((int)base, 0);
                ok = ok && (uint64_t)base + ch0 + ch1 <= g.items_cap;
                if (lane == 0) {
                    g.gq[slot] = ok ? r : 0xFFFFFFFFu;                    // an unusable slot is skipped by the later kernels
                    g.gn[2 * slot] = ok ? ns[0] : 0; g.gn[2 * slot + 1] = ok ? ns[1] : 0;
                    g.goff[2 * slot] = off[0]; g.goff[2 * slot + 1] = off[1];
                }
                if (ok) {
                    for (uint32_t c = lane; c < ch0 + ch1; c += 64) g.gitems[base + c] = (slot << 11) | (c >= ch0 ? (0x400u | (c - ch0)) : c);
                    if (ctr) {
                        for (int o2 = 32; o2 > 0; o2 >>= 1) c_vwords += __shfl_down(c_vwords, o2);
                        if (lane == 0) {
                            atomicAdd(ctr + SALT_CTR_SA_C, c_sa_c); atomicAdd(ctr + SALT_CTR_SA_R, c_sa_r);
                            atomicAdd(ctr + SALT_CTR_VERIFY, c_verify); atomicAdd(ctr + SALT_CTR_VERIFY_WORDS, c_vwords);
                            atomicAdd(ctr + SALT_CTR_LV, ns[0] + ns[1]); atomicAdd(ctr + SALT_CTR_READS, 1ull);
                            atomicAdd(ctr + SALT_CTR_BASES, L); atomicAdd(ctr + SALT_CTR_LOCI, c_loci);
                            atomicAdd(ctr + SALT_CTR_D_SA_HEAVY, c_sa_c + c_sa_r);
                            atomicAdd(ctr + SALT_CTR_D_VERIFY_HEAVY, c_verify * (L <= 248 ? 4u : (((L + 7) >> 3) + 4u) / 4u));      // 121 .. 248 bases: phase 1 of verify_two_phase (the survivors' second look is not counted)
                            atomicAdd(ctr + SALT_CTR_D_OUT_HEAVY, 5u * (ns[0] + ns[1]) + 16u);      // the located rows + distances handed to k_gap
                            if (ix.c_ctx) { atomicAdd(ctr + SALT_CTR_D_CTX_ROWS, c_ctx_rows); atomicAdd(ctr + SALT_CTR_D_CTX_REJECTED, c_ctx_rej); }
                        }
                    }
                    return;
                }
                WSYNC();                                                  // pool exhausted: finish this read here
            }
        }
        if constexpr (!W::HAS_LLV) {
            // ... which takes the lane-LV scratch this block does not carry: the read goes to the overflow queue and the pass behind
            // this kernel (the same code in a block that has it) starts it again.  Nothing of it has been written yet.
            if (lanes_fit && n_cand_nogap > 0) {
                if (lane == 0) g.ovq[atomicAdd(&g.gctl->ovq_count, 1u)] = r;
                return;
            }
        }
        for (int strand = 0; strand < 2; ++strand) {
            pc.stamp(SALT_CTR_T_GAP);
            const CandStats cs = build_candidates_call<PE, GL>(CandArgs{ ix.c_sa, ix.r_pos, sai_c, sai_r, ix.ref_len, ap.spr, ap.max_locate, r, L, strand, true, phase, pe_loci, loci_cap, ap.pe, true, ap.epoch, nullptr, nullptr, 0 }, w);
            if (glob) { loci = cs.in_lds ? w.loci : pe_loci; cand_e = cs.in_lds ? w.cand_e : pe_cand; }
            pc.t = phase ? __builtin_amdgcn_s_memtime() : 0;
            const uint32_t n_cand = cs.n_cand; c_sa_c += cs.n_sa_c; c_sa_r += cs.n_sa_r; c_loci += cs.n_loci;
            bool any = false;
            // all candidates' distances at the call's initial bound, 64 at a time (one per lane); the
            // sequential rule below then only compares numbers
            const bool lanes_ok = lanes_fit && W::HAS_LLV;
            if constexpr (W::HAS_LLV) if (lanes_ok) {
                const int k0 = gap_k0;
                WSYNC();
                lane_pattern(w.u.llv.P, (L + 7) >> 3, lane, 64u, [&](uint32_t j) { return w.pm[strand][j]; });
                for (uint32_t b = 0; b < n_cand; b += LLV_N) {
                    WSYNC();
                    const uint32_t i = b + lane;
                    bool act = false;
                    if (lane < LLV_N && i < n_cand) {
                        const uint32_t pos = loci[i];
                        act = !(pos > ix.ref_len || pos + L + 4 > ix.ref_len);           // ed_diff guard (editdistance.c:178)
                        if (act) lane_text(ix.ref, w.u.llv.T + lane, pos, L + 4);
                    }
                    const uint32_t e = lv_lanes(w.u.llv, w.u.llv.P, (int)L, (int)L + 4, k0, act);
                    if (lane < LLV_N && i < n_cand) cand_e[i] = (uint8_t)e;
                }
                WSYNC();
            }
            for (uint32_t i = 0; i < n_cand; ++i) {
                uint32_t pos = loci[i];
                int e = -1;
                if (lanes_ok) { const uint32_t ev = cand_e[i]; e = (ev != 255 && (int)ev <= maxd) ? (int)ev : -1; }
                else if (!(pos > ix.ref_len || pos + L + 4 > ix.ref_len)) {   // ed_diff guard (editdistance.c:178)
                    lv_unpack(ix.ref, w, strand, L, pos);
                    e = lv_wave(w.u.lvb.T, (int)L + 4, w.u.lvb.P, (int)L, maxd, LvTabRef{ nullptr, nullptr }).e;
                    WSYNC();
                }
                ++c_lv;
                if (e >= 0) {
                    if (e < maxd || !any) { maxd = e; q_gap = 1; q_ndiff = (uint32_t)e; q_strand = (uint32_t)strand; q_pos = pos; }
                    if (n_hits_s[strand] < NHIT && lane == 0) {
                        uint32_t h = n_hits_s[strand];
                        w.hit_pos[strand][h] = pos; w.hit_nd[strand][h] = (uint8_t)e; w.hit_gap[strand][h] = 1;
                    }
                    if (n_hits_s[strand] == 0) a0[strand] = (uint32_t)e;
                    if (n_hits_s[strand] < NHIT) ++n_hits_s[strand];
                    any = true;
                }
            }
            found[strand] = any;
            WSYNC();
        }
    }
    WSYNC();
    pc.stamp(SALT_CTR_T_GAP);

    // ---- hits, MAPQ (query_set_hits / gen_mapq, query.c:270-333) ----
    // every lane computes the same small loop; lane 0 writes
    int b0 = (int)q_ndiff, b1 = 100000, tot = 0;
    uint32_t nh[2] = { 0, 0 };
    uint32_t sel_idx[2][SALT_MAX_HITS];
    for (int s = 0; s < 2 && tot < ap.max_hits; ++s) {
        for (uint32_t j = 0; j < n_hits_s[s]; ++j) {
            uint32_t p = w.hit_pos[s][j];
            if (p == 0xFFFFFFFFu || p == q_pos) continue;
            if (a0[s] <= q_ndiff) {
                if ((int)a0[s] <= b1) b1 = (int)a0[s];
                if (nh[s] < SALT_MAX_HITS) sel_idx[s][nh[s]] = j;
                ++nh[s]; ++tot;
            }
            if (tot == ap.max_hits) break;
        }
    }
    uint32_t mapq = 0;
    if (b0 != 0) {                                            // integer form of 255*|b0-b1|/b0, identical for all inputs
        uint32_t x = (uint32_t)(b0 > b1 ? b0 - b1 : b1 - b0);
        uint64_t q = mapq_quot(x, (uint32_t)b0);
        mapq = q < 254 ? (uint32_t)q : 254u;
    }
    if (lane == 0) {
        out->pos = q_pos; out->strand = (uint8_t)q_strand; out->n_diff = (uint8_t)q_ndiff; out->is_gap = (uint8_t)q_gap;
        out->mapq = (uint8_t)mapq; out->b0 = b0; out->b1 = b1; out->seq_start = 0; out->seq_end = (uint16_t)(L - 1);
        out->n_hits[0] = (uint8_t)nh[0]; out->n_hits[1] = (uint8_t)nh[1]; out->skipped = 0;
        for (int s = 0; s < 2; ++s)
            for (uint32_t j = 0; j < nh[s]; ++j) {
                uint32_t h = sel_idx[s][j];
                out->hits[s][j].pos = w.hit_pos[s][h]; out->hits[s][j].n_diff = w.hit_nd[s][h];
                out->hits[s][j].is_gap = w.hit_gap[s][h]; out->hits[s][j].strand = (uint16_t)s;
            }
    }
    // ---- CIGARs (query_gen_cigar query.c:282-296; XA cigars sam.c:216-225) ----
    if (q_pos != 0xFFFFFFFFu) {
        if (q_gap) {
            lv_cigar(ix.ref, w, lv_tab(lvtab), (int)q_strand, L, q_pos, (int)q_ndiff);
            if (lane < (uint32_t)w.n_cig) out->cigar[lane] = w.cig[lane];
            if (lane == 0) out->n_cigar = (uint8_t)w.n_cig;
        } else if (lane == 0) { out->cigar[0] = (uint16_t)((L << 4) | 0u); out->n_cigar = 1; }
    } else if (lane == 0) out->n_cigar = 0;
    uint32_t hidx = 0;
    for (int s = 0; s < 2; ++s)
        for (uint32_t j = 0; j < nh[s]; ++j, ++hidx) {
            uint32_t h = sel_idx[s][j];
            if (w.hit_gap[s][h]) {
                WSYNC();
                lv_cigar(ix.ref, w, lv_tab(lvtab), s, L, w.hit_pos[s][h], (int)w.hit_nd[s][h]);
                if (lane < (uint32_t)w.n_cig) out->hit_cigar[hidx][lane] = w.cig[lane];
                if (lane == 0) out->hit_n_cigar[hidx] = (uint8_t)w.n_cig;
            } else if (lane == 0) out->hit_n_cigar[hidx] = 0;
        }

    pc.stamp(SALT_CTR_T_TAIL);
    if (phase) {
        const unsigned long long dt = (unsigned long long)(__builtin_amdgcn_s_memrealtime() - rt0);
        pc.add(SALT_CTR_X3, dt);
        if (ctr && lane == 0) atomicMax(ctr + SALT_CTR_MAX_HEAVY, (dt << 32) | r);
    }
    if (ctr) {
        for (int o = 32; o > 0; o >>= 1) c_vwords += __shfl_down(c_vwords, o);
        if (lane == 0) {
            atomicAdd(ctr + SALT_CTR_SA_C, c_sa_c); atomicAdd(ctr + SALT_CTR_SA_R, c_sa_r);
            atomicAdd(ctr + SALT_CTR_VERIFY, c_verify); atomicAdd(ctr + SALT_CTR_VERIFY_WORDS, c_vwords);
            atomicAdd(ctr + SALT_CTR_LV, c_lv); atomicAdd(ctr + SALT_CTR_READS, 1ull);
            atomicAdd(ctr + SALT_CTR_BASES, L); atomicAdd(ctr + SALT_CTR_LOCI, c_loci);
            atomicAdd(ctr + SALT_CTR_D_SA_HEAVY, c_sa_c + c_sa_r);
            atomicAdd(ctr + SALT_CTR_D_VERIFY_HEAVY, c_verify * (L <= 248 ? 4u : (((L + 7) >> 3) + 4u) / 4u));      // 121 .. 248 bases: phase 1 of verify_two_phase (the survivors' second look is not counted)
            atomicAdd(ctr + SALT_CTR_D_OUT_HEAVY, 128u);
            if (ix.c_ctx) { atomicAdd(ctr + SALT_CTR_D_CTX_ROWS, c_ctx_rows); atomicAdd(ctr + SALT_CTR_D_CTX_REJECTED, c_ctx_rej); }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// Persistent kernels: one-wave blocks pull work items until the queue is empty (k_heavy, k_gap, k_gapfin: pop_ranged; k_cigar: sw_pull)
// ---------------------------------------------------------------------------------------------
// Thread 0 of a persistent one-wave block: the next item of a queue of n_items cut into QUEUE_RANGES ranges (ranges[range].heads[which],
// zero at launch); 0xFFFFFFFF once every range is empty.  seg / tried: where this block is (start at blockIdx % QUEUE_RANGES, 0).
__device__ __forceinline__ uint32_t pop_ranged(QueueRange *ranges, const uint32_t which, const uint32_t n_items, uint32_t &seg, uint32_t &tried)
{
    while (tried < QUEUE_RANGES) {
        const uint32_t lo = (uint32_t)((uint64_t)n_items * seg / QUEUE_RANGES), hi = (uint32_t)((uint64_t)n_items * (seg + 1u) / QUEUE_RANGES);
        uint32_t *h = &ranges[seg].heads[which];
        if (lo < hi && __hip_atomic_load(h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < hi - lo) {      // (a look first: late waves do not queue up on an empty range's counter)
            const uint32_t k = atomicAdd(h, 1u);
            if (k < hi - lo) return lo + k;
        }
        seg = (seg + 1u) & (QUEUE_RANGES - 1u); ++tried;
    }
    return 0xFFFFFFFFu;
}
// The same for a whole wave: every lane calls it and gets the wave's item.  With pop_ranged a block whose range has run dry looks at
// the other 63 heads one after the other, a round trip each, before it takes an item elsewhere or leaves -- for the kernels with a
// few items a block (k_gapfin: about three) that walk is most of their time.  Here lane l looks at range l's head, all of them in
// one trip, whenever an add has come back dry; `live` keeps the ranges that had items left at that look (all of them at launch) and
// lane 0 adds to the first of them at or behind seg.  A head only grows, so `live` only shrinks and the loop ends.  k_gapfin takes
// its items this way (87.6 / 92.6 -> 72.4 / 78.6 us alone, profiles/r19); k_gap, four times the blocks, lost 11 us with it and keeps
// pop_ranged.
__device__ __forceinline__ uint32_t pop_ranged_wave(QueueRange *ranges, const uint32_t which, const uint32_t n_items, uint32_t &seg, uint64_t &live)
{
    static_assert(QUEUE_RANGES == 64, "a range a lane");
    const uint32_t lane = lane_id();
    const uint32_t my_size = (uint32_t)((uint64_t)n_items * (lane + 1u) / QUEUE_RANGES) - (uint32_t)((uint64_t)n_items * lane / QUEUE_RANGES);
    while (live) {
        const uint64_t rot = seg ? (live >> seg) | (live << (64u - seg)) : live;
        const uint32_t s = (seg + (uint32_t)__builtin_ctzll(rot)) & (QUEUE_RANGES - 1u);
        const uint32_t lo = (uint32_t)((uint64_t)n_items * s / QUEUE_RANGES), hi = (uint32_t)((uint64_t)n_items * (s + 1u) / QUEUE_RANGES);
        uint32_t k = 0;
        if (lane == 0) k = atomicAdd(&ranges[s].heads[which], 1u);
        k = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        seg = s;
        if (k < hi - lo) return lo + k;
        live = __ballot(__hip_atomic_load(&ranges[lane].heads[which], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < my_size);
    }
    return 0xFFFFFFFFu;
}
template <bool PE, bool GL, class W>
__device__ __forceinline__ void heavy_body(const IndexView &ix, const AlignParams &ap, const uint32_t *__restrict__ pm,
                                           const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r,
                                           salt_result_t *__restrict__ results, const uint32_t *__restrict__ queue,
                                           unsigned long long *__restrict__ ctr, LvTables *__restrict__ lvtab, const GapBufs g,
                                           uint8_t *__restrict__ pe_scr, const int overflow_pass)
{
    __shared__ W w;
    __shared__ uint32_t s_item;
    __shared__ unsigned long long s_phase[SALT_CTR_N];
    unsigned long long *phase = ctr ? s_phase : nullptr;
    if (ctr) { for (int i = threadIdx.x; i < SALT_CTR_N; i += 64) s_phase[i] = 0; }
    WSYNC();
    // the usual pass takes the reads k_light queued (or all of them); the overflow pass the ones a block without the lane-LV scratch left
    const uint32_t n_items = overflow_pass ? g.gctl->ovq_count : ap.all_heavy ? ap.n_reads : g.gctl->light_queued;
    // One read per pop.  The pops of all waves on ONE counter are served one after the other, ~14 ns each whatever the waves do in between
    // (75 700 queued reads: 1.09 of the kernel's 1.165 ms, the same at 8, 12 and 16 blocks per CU; time = 0.08 ms + 14.4 ns x reads from
    // 9 000 to 150 000 reads, profiles/r03/heavy_vs_batch.log).  So the queue is cut into QUEUE_RANGES ranges with a head each, 256 bytes
    // apart; a wave starts at range blockIdx % QUEUE_RANGES and moves on to the next when one is empty (pop_ranged).  k_gap and k_gapfin
    // take their items the same way; the counters k_heavy's gapped reads push through are a cache line apart each (SeCtl).
    uint32_t seg = blockIdx.x & (QUEUE_RANGES - 1u), tried = 0;
    for (;;) {
        if (threadIdx.x == 0) {
            uint32_t got = 0xFFFFFFFFu;
            if (overflow_pass) { got = atomicAdd(&g.gctl->ovq_head, 1u); if (got >= n_items) got = 0xFFFFFFFFu; }
            else got = pop_ranged(g.ranges, QueueRange::HEAVY, n_items, seg, tried);
            s_item = got;
        }
        WSYNC();
        const uint32_t it = s_item;
        WSYNC();
        if (it == 0xFFFFFFFFu) break;
        const uint32_t r = overflow_pass ? g.ovq[it] : ap.all_heavy ? it : queue[it];
        align_general<PE, GL>(ix, ap, w, r, pm, sai_c, sai_r, results, ctr, phase, lvtab + blockIdx.x, g,
                          pe_scr ? reinterpret_cast<uint32_t *>(pe_scr + (size_t)blockIdx.x * PE_LOCI_CAP * 5) : nullptr,
                          pe_scr ? pe_scr + (size_t)blockIdx.x * PE_LOCI_CAP * 5 + (size_t)PE_LOCI_CAP * 4 : nullptr);
        if (phase && threadIdx.x == 0) s_phase[SALT_CTR_HEAVY_READS] += 1;
        WSYNC();
    }
    if (phase) {                                                         // one flush per wave
        WSYNC();
        for (int i = SALT_CTR_T_LOAD + (int)threadIdx.x; i < SALT_CTR_N; i += 64) if (s_phase[i]) atomicAdd(ctr + i, s_phase[i]);
    }
}

// Registers of the persistent kernels capped for four waves per SIMD (128 VGPRs, ~20 spilled on rare paths): 16 one-wave blocks per CU.
// Uncapped (12 per CU) k_heavy takes 0.83 ms per 10^6 GRCh38-scale reads and k_heavy_pe 2.01 per 10^6 mates; capped 0.73 and 1.76, and the
// kernels of the other batches in flight find more room beside them (profiles/r03/ab_heavy_ranged_pops.log).  -DSALT_HEAVY_WAVES=0: no cap.
#ifndef SALT_HEAVY_WAVES
#define SALT_HEAVY_WAVES 4
#endif
#if SALT_HEAVY_WAVES > 0
#define HEAVY_OCC __attribute__((amdgpu_waves_per_eu(SALT_HEAVY_WAVES, SALT_HEAVY_WAVES)))
#else
#define HEAVY_OCC
#endif
#define HEAVY_KERNEL(NAME, PE, GL, LDS)                                                                                    \
__global__ void __launch_bounds__(64) HEAVY_OCC                                                                         \
NAME(IndexView ix, AlignParams ap, const uint32_t *__restrict__ pm,                                                     \
     const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r, salt_result_t *__restrict__ results,             \
     const uint32_t *__restrict__ queue, unsigned long long *__restrict__ ctr,                                          \
     LvTables *__restrict__ lvtab, GapBufs g, uint8_t *__restrict__ pe_scr, int overflow_pass)                          \
{ heavy_body<PE, GL, LDS>(ix, ap, pm, sai_c, sai_r, results, queue, ctr, lvtab, g, pe_scr, overflow_pass); }
HEAVY_KERNEL(k_heavy, false, false, WaveLdsSmall)      // the usual shape: <= 32 seed slots per strand, gapped reads handed to k_gap
HEAVY_KERNEL(k_heavy_pe, true, true, WaveLdsSmall)    // paired-end mates: PE locate rule, loci in global scratch, gap bound 3
HEAVY_KERNEL(k_heavy_big, false, false, WaveLds)      // any read the ABI admits, everything finished inside the block: batches with more seed
HEAVY_KERNEL(k_heavy_pe_big, true, true, WaveLds)
HEAVY_KERNEL(k_heavy_glob, false, true, WaveLds)    // single end with -m above the LDS list (SALT_MAX_LOCATE): located rows in the block's global list, everything in this one shape
//    // slots, runs without the k_gap buffers, and the overflow pass behind the usual shape

// k_gap: one item = 32 candidates of one strand of one queued read: their Landau-Vishkin distances at the bound L/10
// (ed_diff -> computeEditDistance, editdistance.c:174-232, LandauVishkin.c:19-122), one candidate per lane
__global__ void __launch_bounds__(64)
k_gap(IndexView ix, AlignParams ap, const uint32_t *__restrict__ pm, GapBufs g)
{
    __shared__ LaneLv s;
    __shared__ uint32_t s_item;
    const uint32_t lane = lane_id();
    const uint32_t n_items = g.gctl->gap_items < g.items_cap ? g.gctl->gap_items : g.items_cap;
    uint32_t seg = blockIdx.x & (QUEUE_RANGES - 1u), tried = 0;
    for (;;) {
        if (threadIdx.x == 0) s_item = pop_ranged(g.ranges, QueueRange::GAP, n_items, seg, tried);
        WSYNC();
        const uint32_t it = s_item;
        WSYNC();
        if (it == 0xFFFFFFFFu) break;
        const uint32_t item = g.gitems[it], slot = item >> 11, strand = (item >> 10) & 1u, chunk = item & 1023u;
        const uint32_t r = g.gq[slot];
        const uint32_t *rec = pm + (uint64_t)r * ap.pg.pm_stride;
        const uint32_t L = rec[2 * ap.pg.nw8], nw = (L + 7) >> 3;
        lane_pattern(s.P, nw, lane, 64u, [&](uint32_t j) { return rec[strand * ap.pg.nw8 + j]; });
        const uint32_t n = g.gn[2 * slot + strand], i = chunk * LLV_N + lane;
        const size_t row = g.goff[2 * slot + strand];
        bool act = false;
        if (lane < LLV_N && i < n) {
            const uint32_t pos = g.gloci[row + i];
            act = !(pos > ix.ref_len || pos + L + 4 > ix.ref_len);               // ed_diff guard (editdistance.c:178)
            if (act) lane_text(ix.ref, s.T + lane, pos, L + 4);
        }
        WSYNC();
        const uint32_t e = lv_lanes(s, s.P, (int)L, (int)L + 4, ap.pe ? 3 : (int)(L / 10), act);   // alnse.c:1090 / 1016-1028
        if (lane < LLV_N && i < n) g.ge[row + i] = (uint8_t)e;
        WSYNC();
    }
}

// k_gapfin: one queued read per wave: alnse_check_withgap's sequential rule (alnse.c:871-901, code_kdiff 371-393)
// replayed by ballots over the stored distances, strand 0 then 1 with the bound carried over; then
// query_set_hits / gen_mapq (query.c:270-333) and the result row; every LV traceback becomes a k_cigar item.
struct FinLds { uint32_t hit_pos[2][NHIT]; uint8_t hit_nd[2][NHIT]; };
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))      // 128 VGPRs: 16 one-wave blocks a CU, as the kernels beside it
k_gapfin(IndexView ix, AlignParams ap, const uint32_t *__restrict__ pm, salt_result_t *__restrict__ results, GapBufs g,
         unsigned long long *__restrict__ ctr)
{
    __shared__ FinLds w;
    const uint32_t lane = lane_id();
    const uint32_t n_items = g.gctl->gap_slots < g.cap ? g.gctl->gap_slots : g.cap;
    uint32_t seg = blockIdx.x & (QUEUE_RANGES - 1u);
    uint64_t live = ~0ull;
    for (;;) {
        const uint32_t slot = pop_ranged_wave(g.ranges, QueueRange::GAPFIN, n_items, seg, live);
        if (slot == 0xFFFFFFFFu) break;
        const uint64_t rt0 = ctr ? __builtin_amdgcn_s_memrealtime() : 0;
        // An item is a chain of loads, not work: the slot's read and both strands' list heads are asked for together, then the read's
        // length and the first GAPFIN_B trips of BOTH lists (strand 1's addresses do not depend on the bound strand 0 leaves, only its
        // filter does), and the rule takes the rest of a list two batches at a time (list_trips).
        // (Everything about the item is the wave's, not the lane's: said so, the lists' addresses are scalar and a batch's 2 B loads
        // take one lane offset between them.)
        auto uni = [](uint32_t x) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); };
        const uint32_t r_v = g.gq[slot];
        const uint2 n2 = *reinterpret_cast<const uint2 *>(g.gn + 2 * slot), off2 = *reinterpret_cast<const uint2 *>(g.goff + 2 * slot);
        const uint32_t r = uni(r_v);
        if (r == 0xFFFFFFFFu) continue;                                   // the pool was full: k_heavy finished this read itself
        const uint32_t L_v = pm[(uint64_t)r * ap.pg.pm_stride + 2 * ap.pg.nw8];
        const uint32_t n_s[2] = { uni(n2.x), uni(n2.y) };
        const size_t row_s[2] = { uni(off2.x), uni(off2.y) };
        RowBatch<GAPFIN_B> first[2];
#pragma unroll
        for (int strand = 0; strand < 2; ++strand)
            if (n_s[strand]) rows_fetch<GAPFIN_B>(first[strand], g.gloci + row_s[strand], g.ge + row_s[strand], n_s[strand], 0u);
        const uint32_t L = uni(L_v);
        salt_result_t *out = results + r;
        uint32_t q_pos = 0xFFFFFFFFu, q_strand = 3, q_ndiff = 255, q_gap = 255;
        uint32_t bound = ap.pe ? 3u : L / 10;                             // alnse.c:1090 (SE) / alnse.c:1016-1028 (PE keeps 3)
        uint32_t n_hits_s[2] = { 0, 0 }, a0[2] = { 0, 0 };
#pragma unroll
        for (int strand = 0; strand < 2; ++strand) {
            const uint32_t n = n_s[strand];
            const size_t row = row_s[strand];
            bool any = false; uint32_t bp = 0, bv = 0;
            rule_unsorted<LLV_K, true, GAPFIN_B>(g.gloci + row, g.ge + row, n, L, ix.ref_len, bound, any, bp, bv, n_hits_s[strand], a0[strand],
                                                 w.hit_pos[strand], w.hit_nd[strand], &first[strand]);
            if (any) { q_pos = bp; q_ndiff = bv; q_gap = 1; q_strand = (uint32_t)strand; }
        }
        WSYNC();
        int b0 = (int)q_ndiff, b1 = 100000, tot = 0;
        uint32_t nh[2] = { 0, 0 };
        uint32_t sel_idx[2][SALT_MAX_HITS];
        for (int s = 0; s < 2 && tot < ap.max_hits; ++s)
            for (uint32_t j = 0; j < n_hits_s[s]; ++j) {
                const uint32_t p = w.hit_pos[s][j];
                if (p == 0xFFFFFFFFu || p == q_pos) continue;
                if (a0[s] <= q_ndiff) {
                    if ((int)a0[s] <= b1) b1 = (int)a0[s];
                    if (nh[s] < SALT_MAX_HITS) sel_idx[s][nh[s]] = j;
                    ++nh[s]; ++tot;
                }
                if (tot == ap.max_hits) break;
            }
        uint32_t mapq = 0;
        if (b0 != 0) {
            const uint32_t x = (uint32_t)(b0 > b1 ? b0 - b1 : b1 - b0);
            const uint64_t q = mapq_quot(x, (uint32_t)b0);
            mapq = q < 254 ? (uint32_t)q : 254u;
        }
        const uint32_t n_cig_items = q_pos != 0xFFFFFFFFu ? 1u + nh[0] + nh[1] : 0u;
        const uint32_t first_cig = ap.pe ? 1u : 0u;                        // paired end: the alignment's own CIGAR is made after pairing (k_pe_final)
        if (lane == 0) {
            out->pos = q_pos; out->strand = (uint8_t)q_strand; out->n_diff = (uint8_t)q_ndiff; out->is_gap = (uint8_t)q_gap;
            out->mapq = (uint8_t)mapq; out->b0 = b0; out->b1 = b1; out->seq_start = 0; out->seq_end = (uint16_t)(L - 1);
            out->n_hits[0] = (uint8_t)nh[0]; out->n_hits[1] = (uint8_t)nh[1]; out->skipped = 0; out->n_cigar = 0;
            for (int s = 0; s < 2; ++s)
                for (uint32_t j = 0; j < nh[s]; ++j) {
                    const uint32_t h = sel_idx[s][j];
                    out->hits[s][j].pos = w.hit_pos[s][h]; out->hits[s][j].n_diff = w.hit_nd[s][h];
                    out->hits[s][j].is_gap = 1; out->hits[s][j].strand = (uint16_t)s;
                }
            if (n_cig_items > first_cig) {                                // main hit (which = 0) and every alternative hit (1 + index)
                const uint32_t base = atomicAdd(&g.gctl->cigar_items, n_cig_items - first_cig);
                for (uint32_t c = first_cig; c < n_cig_items; ++c) g.cq[base + c - first_cig] = (r << 3) | c;
            }
            if (ctr) atomicMax(ctr + SALT_CTR_MAX_GAPFIN, ((unsigned long long)(__builtin_amdgcn_s_memrealtime() - rt0) << 32) | r);
        }
        WSYNC();
    }
}

// k_cigar: one LV traceback per wave (query_gen_cigar query.c:282-296; XA CIGARs sam.c:216-225).
// items[i] = (read << 3) | which, which 0 = the alignment itself, 1 + h = alternative hit h; *count items, *head = the queue head
__global__ void __launch_bounds__(64)
k_cigar(IndexView ix, PackGeom pg, const uint32_t *__restrict__ pm, salt_result_t *__restrict__ results,
        const uint32_t *__restrict__ items, const uint32_t *__restrict__ count, uint32_t *__restrict__ head, uint32_t cap_items,
        LvTables *__restrict__ lvtab)
{
    __shared__ WaveLdsCigar w;
    __shared__ LvTablesLds tl;                                          // the tables of a traceback at k <= LLV_K; a larger k takes the block's global table
    __shared__ uint32_t s_item;
    const uint32_t lane = lane_id();
    const uint32_t n_items = *count < cap_items ? *count : cap_items;
    struct { PackGeom pg; } ap = { pg };
    bool first = true;
    for (;;) {
        if (threadIdx.x == 0) s_item = first ? blockIdx.x : sw_pull(head, 1u, gridDim.x, n_items);      // the block's own index first
        first = false;
        WSYNC();
        const uint32_t it = s_item;
        WSYNC();
        if (it >= n_items) break;
        const uint32_t item = items[it], which = item & 7u, r = item >> 3;
        salt_result_t *out = results + r;
        const uint32_t *rec = pm + (uint64_t)r * ap.pg.pm_stride;
        const uint32_t L = rec[2 * ap.pg.nw8];
        uint32_t strand, pos, k;
        if (which == 0) { strand = out->strand; pos = out->pos; k = out->n_diff; }
        else {
            const uint32_t h = which - 1, n0 = out->n_hits[0];
            strand = h >= n0; const uint32_t j = strand ? h - n0 : h;
            pos = out->hits[strand][j].pos; k = out->hits[strand][j].n_diff;
        }
        for (uint32_t t = lane; t < (L + 7) >> 3; t += 64) w.pm[strand][t] = rec[strand * ap.pg.nw8 + t];
        WSYNC();
        lv_cigar_here(ix.ref, w, k <= (uint32_t)LLV_K ? lv_tab(tl) : lv_tab(lvtab + blockIdx.x), (int)strand, L, pos, (int)k);
        uint16_t *dst = which == 0 ? out->cigar : out->hit_cigar[which - 1];
        if (lane < (uint32_t)w.n_cig) dst[lane] = w.cig[lane];
        if (lane == 0) { if (which == 0) out->n_cigar = (uint8_t)w.n_cig; else out->hit_n_cigar[which - 1] = (uint8_t)w.n_cig; }
        WSYNC();
    }
}

// ---------------------------------------------------------------------------------------------
// The light kernels (k_light, k_light2, k_light4): one body, light_read, at three widths -- a wave per read, half a wave, or a quarter.
// The common case in three memory round trips.
//
// A read stays here when (a) it is short enough for the small LDS image (a wave: L <= 160, <= 16 seed slots; a half: 120 / 248, <= 8;
// a quarter: 120, <= 4),
// (b) each of its four seed lists (C/R x strand) enumerates at most 64 suffix-array rows, so that the
// max_locate cap (>= 128) can never bite and locate order is irrelevant once the loci are sorted, and
// (c) a gap-free hit exists.  Everything else is queued for k_heavy, which replays the reference's
// general control flow.  Same results either way; the split only changes who computes them.
// ---------------------------------------------------------------------------------------------
// The queue of reads for k_heavy.  One counter for all of them was what k_light2 waited for: an atomic on ONE address is served every
// ~11 ns however many waves ask (75 700 queued reads: 0.83 of its 0.87 ms).  The reads of workgroup-sized groups of four go to one
// of QUEUE_RANGES segments, each with a counter 256 bytes from the next (QueueRange::push) and room for every read that can map to it;
// k_queue_pack then lays the segments end to end (the order of the queue does not matter) and leaves the count where k_heavy reads it.
__host__ __device__ __forceinline__ uint32_t qseg_cap(uint32_t n_reads) { return n_reads / QUEUE_RANGES + 8u; }
__device__ __forceinline__ void queue_push(uint32_t *__restrict__ qseg, QueueRange *__restrict__ ranges, uint32_t n_reads, uint32_t r)
{
    const uint32_t s = (r >> 2) & (QUEUE_RANGES - 1u);
    qseg[(size_t)s * qseg_cap(n_reads) + atomicAdd(&ranges[s].push, 1u)] = r;
}
// The reads a quarter of a wave cannot hold (k_light4: a list above L4_ROWS rows, none above 64) wait in segments of their own behind
// k_heavy's, built the same way (QueueRange::retry), for k_light_retry.
__device__ __forceinline__ uint32_t *retry_segs(uint32_t *qseg, uint32_t n_reads) { return qseg + (size_t)QUEUE_RANGES * qseg_cap(n_reads); }
__device__ __forceinline__ void retry_push(uint32_t *__restrict__ qseg, QueueRange *__restrict__ ranges, uint32_t n_reads, uint32_t r)
{
    const uint32_t s = (r >> 2) & (QUEUE_RANGES - 1u);
    retry_segs(qseg, n_reads)[(size_t)s * qseg_cap(n_reads) + atomicAdd(&ranges[s].retry, 1u)] = r;
}
__global__ void __launch_bounds__(256)
k_queue_pack(const uint32_t *__restrict__ qseg, const QueueRange *__restrict__ ranges, uint32_t n_reads, uint32_t *__restrict__ queue, SeCtl *__restrict__ ctl)
{
    __shared__ uint32_t base_s, cnt_s;
    if (threadIdx.x == 0) {
        uint32_t base = 0, total = 0;
        for (uint32_t s = 0; s < QUEUE_RANGES; ++s) { const uint32_t c = ranges[s].push; if (s < blockIdx.x) base += c; total += c; }
        base_s = base; cnt_s = ranges[blockIdx.x].push;
        if (blockIdx.x == 0) ctl->light_queued = total;
    }
    __syncthreads();
    const uint32_t *src = qseg + (size_t)blockIdx.x * qseg_cap(n_reads);
    for (uint32_t i = threadIdx.x; i < cnt_s; i += 256) queue[base_s + i] = src[i];
}

static constexpr int LT_LOCI = 128;      // loci per strand handled here
static constexpr int LT_MAXL = 160;      // longest read that gets a whole wave here
static constexpr int L2_SLOTS = 8;       // seed slots per list of a read that gets a half-wave
static constexpr int L4_SLOTS = 4;       // ... of a read that gets a quarter
#ifndef SALT_L4_ROWS
#define SALT_L4_ROWS 16
#endif
static constexpr int L4_ROWS = SALT_L4_ROWS;     // rows per list a quarter's record holds; a read with a longer list (up to 64) goes to the retry launch

// A read's LDS record: SLOTS seed slots per list (a quarter of the group's lanes), PMW one-hot words per strand, LOCI located rows per strand
template <int SLOTS, int PMW, int LOCI> struct LightRec {
    uint32_t pm[2][PMW];
    uint32_t sp[4][SLOTS], off[4][SLOTS];
    uint32_t pre[4][SLOTS + 1];          // rows enumerated before slot i of list l
    uint32_t loci[2][LOCI];
    uint32_t hit_pos[2][NHIT];
    uint8_t  hit_nd[2][NHIT];
    uint8_t  val[2][LOCI];
};
// a wave's read: 16 slots, 160 bases; a half-wave's: 8 slots, 32 words (reads up to 120 bases use 15 a strand, up to 248 bases 31);
// a quarter's: 4 slots, 16 words (120 bases), L4_ROWS rows a list
template <int GW> using LightLds = LightRec<GW / 4, GW == 64 ? LT_MAXL / 8 : GW == 32 ? 32 : 16, GW == 16 ? 2 * L4_ROWS : LT_LOCI>;
static_assert(sizeof(LightLds<32>) == 1996 && 8 * sizeof(LightLds<16>) <= 4 * sizeof(LightLds<32>), "eight quarter records in the LDS of four half-wave ones");

// The body of the light kernels: read r on a group of GW lanes (LaneGroup), every ballot / shuffle inside the group.
// LN: lanes per located row in the window check: 4 cover reads up to 120 bases, 8 up to 248; 0 = picked by the read's length.
// INSTR: the access counters and phase stamps behind `ctr`, and the diagnostics build's early exits (ap.dbg_stop); without it none of
// that is compiled.
template <int GW, int LN, bool INSTR>
__device__ __forceinline__ void light_read(const IndexView &ix, const AlignParams &ap, const uint32_t *__restrict__ pm,
                                           const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r, salt_result_t *__restrict__ results,
                                           uint32_t *__restrict__ queue /* the segments */, QueueRange *__restrict__ ranges,
                                           unsigned long long *__restrict__ ctr, LightLds<GW> &w, const uint32_t r)
{
    typedef LaneGroup<GW> G;
    typedef typename G::mask_t mask_t;
    constexpr uint32_t SLOTS = GW / 4, HALF = GW / 2;
    constexpr uint32_t LMAX = LN == 4 ? 120u : LN == 8 ? 248u : (uint32_t)LT_MAXL;
    static_assert(LMAX <= 8 * sizeof(w.pm[0]) / 4 && (LN != 0 || LMAX <= 248u), "the read fits the record and the window check");
    const uint32_t lane = G::lane();
    const mask_t lt = G::below();
    const uint32_t *rec = pm + (uint64_t)r * ap.pg.pm_stride;               // k_pack's one-hot words of this read, both strands
    const uint32_t L = rec[2 * ap.pg.nw8];
    bool heavy = L > LMAX || L < (uint32_t)ap.l_seed || ap.spr > SLOTS || ap.max_locate < 2 * 64;
    uint32_t c_sa_c = 0, c_sa_r = 0, c_verify = 0, c_loci = 0;
    const bool prof = INSTR && ctr && (r & 127u) == 0;                       // phase clock of every 128th read
    uint64_t tp = prof ? __builtin_amdgcn_s_memtime() : 0;
    auto stamp = [&](int slot) {
        if (!prof) return;
        const uint64_t n = __builtin_amdgcn_s_memtime();
        if (lane == 0) atomicAdd(ctr + slot, (unsigned long long)(n - tp));
        tp = n;
    };
    // a suffix-array row of list l (or, with bit 31 of `of`, a genome position) less the seed's offset, and whether alnse_locate_alt
    // keeps it (alnse.c:672-673,715-717)
    auto locate = [&](uint32_t l, uint32_t j, uint32_t of, uint32_t &p) -> bool {
        p = ((of >> 31) ? j : (l & 1) ? ix.r_pos[j] : ix.c_sa[j]) - (of & 0x7FFFFFFFu);
        return (l & 1) ? !(p > ix.ref_len || p + L > ix.ref_len) : !(p + L > ix.ref_len);
    };

    if (!heavy) {
        // ---- round trip 1: the read (as one-hot nibble words, both strands) and its seeds ----
        const uint32_t nw = (L + 7) >> 3;
        __builtin_assume(nw <= (LMAX + 7) / 8);
        uint32_t n_amb = 0;
        for (uint32_t x = lane; x < 2 * nw; x += GW) {                      // (one trip unless 150-base reads share a wave)
            const uint32_t s = x >= nw, j = s ? x - nw : x;
            const uint32_t word = rec[s * ap.pg.nw8 + j];
            w.pm[s][j] = word;
            if (!s) n_amb += popc(word & (word >> 1) & (word >> 2) & (word >> 3) & 0x11111111u);   // N = all four bits
        }
        if (ap.max_amb < L) {                                               // (uniform) otherwise the limit cannot be passed
            n_amb = G::sum(n_amb);
            if (n_amb > ap.max_amb) {                                       // alnse.c:1328 / alnpe.c:495: record left untouched
                if (lane == 0) {
                    salt_result_t *out = results + r;
                    out->pos = 0xFFFFFFFFu; out->strand = 3; out->n_diff = 255; out->is_gap = 255; out->mapq = 0;
                    out->b0 = -1; out->b1 = -1; out->seq_start = 0; out->seq_end = (uint16_t)(L - 1);
                    out->n_hits[0] = out->n_hits[1] = 0; out->n_cigar = 0; out->skipped = 1;
                }
                return;
            }
        }
        uint32_t tot[4];
        bool small;
        {
            // lane = (list, slot); list: 0 C/fwd 1 R/fwd 2 C/rev 3 R/rev.  The reference orders each list by
            // interval size (alnse.c:307-308), which only decides what is located first when the max_locate
            // cap bites; here it cannot (<= 64 rows per list), and the loci are sorted afterwards anyway.
            const uint32_t l = lane / SLOTS, slot = lane % SLOTS;
            uint4 v = make_uint4(1, 0, 0, 0);
            if (slot < ap.spr) { v = ((l & 1) ? sai_r : sai_c)[((uint64_t)r * 2u + (l >> 1)) * ap.spr + slot]; if (l & 1) v = sai_r_row(v, ap.epoch); }
            uint32_t sz = v.w ? v.y - v.x + 1u : 0u;
            if (sz > 65u) sz = 65u;                                         // keeps the sums below from wrapping
            uint32_t inc = sz;                                              // inclusive prefix sum within the list's row of lanes
            for (int o = 1; o < (int)SLOTS; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)inc, o, SLOTS); if (slot >= (uint32_t)o) inc += t; }
            for (int q = 0; q < 4; ++q) tot[q] = G::bcast(inc, (int)SLOTS * q + (int)SLOTS - 1);
            small = tot[0] <= SLOTS && tot[1] <= SLOTS && tot[2] <= SLOTS && tot[3] <= SLOTS;      // (uniform) the usual case
            if (small) {
                // every seed writes the suffix-array rows of its interval where the row lanes of its list will look them up
                for (uint32_t k2 = 0; k2 < sz; ++k2) { w.sp[l][inc - sz + k2] = v.x + k2; w.off[l][inc - sz + k2] = v.z | (v.w == 2 ? 0x80000000u : 0u); }
            } else {
                w.sp[l][slot] = v.x; w.off[l][slot] = v.z | (v.w == 2 ? 0x80000000u : 0u);        // bit 31: .x is a genome position already
                w.pre[l][slot + 1] = inc;
                if (slot == 0) w.pre[l][0] = 0;
            }
        }
        WSYNC();
        stamp(SALT_CTR_LT_SEEDS);
        for (int l = 0; l < 4; ++l) heavy |= tot[l] > 64;
        if constexpr (GW == 16) {
            // a list the record cannot hold: the half-wave body takes the read (k_light_retry), which also decides whether it is heavy
            if (!heavy && (tot[0] > (uint32_t)L4_ROWS || tot[1] > (uint32_t)L4_ROWS || tot[2] > (uint32_t)L4_ROWS || tot[3] > (uint32_t)L4_ROWS)) {
                if (lane == 0) retry_push(queue, ranges, ap.n_reads, r);
                return;
            }
        }
        if (INSTR && ap.dbg_stop == 1) { if (lane == 0) results[r].pos = tot[0] + tot[1] + tot[2] + tot[3] + w.pm[0][0] + w.pm[1][1]; return; }
        if (!heavy) {
            // ---- round trip 2: the suffix-array rows of the four lists ----
            uint32_t n_s[2] = { 0, 0 };
            if (small) {
                // lane = (list, row): at most SLOTS rows per list, so one lane per row covers all four lists in one go
                const uint32_t l = lane / SLOTS, x = lane % SLOTS;
                const uint32_t tl = l == 0 ? tot[0] : l == 1 ? tot[1] : l == 2 ? tot[2] : tot[3];
                bool keep = false; uint32_t p = 0;
                if (x < tl) keep = locate(l, w.sp[l][x], w.off[l][x], p);
                stamp(SALT_CTR_LT_LOCATE);
                if (INSTR && ap.dbg_stop == 2) { if (__ballot(p == 12345u) == 1) results[r].pos = p; return; }
                const mask_t km = G::ballot(keep);                          // a strand's two lists are one half of it
                const uint32_t k0 = (uint32_t)(km & (((mask_t)1 << HALF) - 1)), k1 = (uint32_t)(km >> HALF), s = lane / HALF;
                if (keep) w.loci[s][popc((s ? k1 : k0) & ((1u << (lane % HALF)) - 1u))] = p;
                n_s[0] = popc(k0); n_s[1] = popc(k1);
                c_sa_c += tot[0] + tot[2]; c_sa_r += tot[1] + tot[3];
            } else {
                // row x of list l: its seed slot by the prefix sums (empty slots, with equal sums, are skipped), then as above
                auto locate_row = [&](uint32_t l, uint32_t x, uint32_t &p) -> bool {
                    uint32_t i = 0;
                    while (w.pre[l][i + 1] <= x) ++i;
                    return locate(l, w.sp[l][i] + (x - w.pre[l][i]), w.off[l][i], p);
                };
                if constexpr (GW == 64 || (GW == 16 && L4_ROWS <= 16)) {
                    // A list has at most 64 rows (a quarter's: L4_ROWS), one a lane: the loads of all four lists are in flight before the
                    // first ballot.
                    uint32_t pos4[4]; bool keep4[4];
                    for (int l = 0; l < 4; ++l) {
                        keep4[l] = false; pos4[l] = 0;
                        if (lane < tot[l]) keep4[l] = locate_row(l, lane, pos4[l]);
                    }
                    stamp(SALT_CTR_LT_LOCATE);
                    if (INSTR && ap.dbg_stop == 2) { const uint32_t x = pos4[0] + pos4[1] + pos4[2] + pos4[3]; if (__ballot(x == 12345u) == 1) results[r].pos = x; return; }
                    for (int s = 0; s < 2; ++s) {                           // both lists of a strand, as located (no order, duplicates stay)
                        const mask_t mc = G::ballot(keep4[2 * s]), mr = G::ballot(keep4[2 * s + 1]);
                        const uint32_t nc = popc(mc);
                        if (keep4[2 * s]) w.loci[s][popc(mc & lt)] = pos4[2 * s];
                        if (keep4[2 * s + 1]) w.loci[s][nc + popc(mr & lt)] = pos4[2 * s + 1];
                        n_s[s] = nc + popc(mr);
                    }
                } else {
                    // Half a wave needs two trips for such a list, and eight rows a lane in flight do not fit the 64 registers that 8
                    // waves a SIMD leave (58 - 60 are in use): list by list, a trip at a time, as this kernel always went.  Neither
                    // width was measured with the other's order.
                    for (int l = 0; l < 4; ++l) {
                        const int s = l >> 1;
                        for (uint32_t x = lane; x - lane < tot[l]; x += GW) {     // (x - lane) is the same for the whole group: a uniform trip count
                            bool keep = false; uint32_t p = 0;
                            if (x < tot[l]) keep = locate_row(l, x, p);
                            const mask_t km = G::ballot(keep);
                            if (keep) w.loci[s][n_s[s] + popc(km & lt)] = p;
                            n_s[s] += popc(km);
                        }
                    }
                }
                c_sa_c += tot[0] + tot[2]; c_sa_r += tot[1] + tot[3];
            }
            c_loci += n_s[0] + n_s[1];
            WSYNC();
            stamp(SALT_CTR_LT_SORT);
            if (INSTR && ap.dbg_stop == 3) { if (lane == 0) results[r].pos = w.loci[0][0] + w.loci[1][0] + n_s[0] + n_s[1]; return; }
            // ---- round trip 3: masked Hamming distance of every located row of both strands, 4 or 8 lanes per row ----
            if (LN == 4 || (LN == 0 && L <= 120)) verify_quads_2<4, GW>(ix.ref, ix.ref_len, w.pm[0], w.pm[1], L, w.loci[0], n_s[0], w.loci[1], n_s[1], w.val[0], w.val[1]);
            else verify_quads_2<8, GW>(ix.ref, ix.ref_len, w.pm[0], w.pm[1], L, w.loci[0], n_s[0], w.loci[1], n_s[1], w.val[0], w.val[1]);
            WSYNC();
            stamp(SALT_CTR_LT_VERIFY);
            if (INSTR && ap.dbg_stop == 4) { if (__ballot(w.val[0][0] + w.val[1][0] == 12345u) == 1) results[r].pos = w.val[0][0]; return; }
            c_verify += n_s[0] + n_s[1];
            // ---- the sequential best/first-hit rule (alnse.c:348-369, 1079-1083) on the unsorted rows: rule_sparse ----
            uint32_t bound = 3, q_pos = 0xFFFFFFFFu, q_strand = 3, q_ndiff = 255;
            uint32_t n_hits_s[2] = { 0, 0 }, a0[2] = { 0, 0 };
            bool found[2] = { false, false };
            for (int s = 0; s < 2; ++s) {
                bool any = false; uint32_t bp = 0, bv = 0;
                rule_sparse<3, false, GW>(w.loci[s], w.val[s], n_s[s], L, ix.ref_len, bound, any, bp, bv, n_hits_s[s], a0[s], w.hit_pos[s], w.hit_nd[s]);
                if (any) { found[s] = true; q_pos = bp; q_ndiff = bv; q_strand = (uint32_t)s; }
            }
            if (INSTR && ap.dbg_stop == 5) { if (lane == 0) results[r].pos = q_pos + n_hits_s[0] + n_hits_s[1] + a0[0] + a0[1]; return; }
            if (!found[0] && !found[1]) heavy = true;                       // needs the gapped pass
            else {
                WSYNC();
                // ---- query_set_hits / gen_mapq (query.c:270-333): lane t < 2*NHIT looks at recorded hit (t / NHIT, t % NHIT);
                // the sequential loop keeps the first max_hits of them that are neither the primary nor worse than it ----
                const uint32_t hs = lane >= (uint32_t)NHIT, hj = lane - hs * NHIT;
                uint32_t hp = 0xFFFFFFFFu, hn = 0;
                bool cand = false;
                if (lane < 2u * NHIT && hj < (hs ? n_hits_s[1] : n_hits_s[0])) {
                    hp = w.hit_pos[hs][hj]; hn = w.hit_nd[hs][hj];
                    cand = hp != 0xFFFFFFFFu && hp != q_pos && (hs ? a0[1] : a0[0]) <= q_ndiff;
                }
                const mask_t cm = G::ballot(cand);
                const bool sel = cand && popc(cm & lt) < (uint32_t)ap.max_hits;
                const mask_t sm = G::ballot(sel);
                const uint32_t nh0 = popc(sm & (((mask_t)1 << NHIT) - 1)), nh1 = popc(sm >> NHIT);
                const int b0 = (int)q_ndiff;
                int b1 = 100000;
                if (nh0) b1 = (int)a0[0];
                if (nh1 && (int)a0[1] <= b1) b1 = (int)a0[1];
                uint32_t mapq = 0;
                if (b0 != 0) {
                    const uint32_t x = (uint32_t)(b0 > b1 ? b0 - b1 : b1 - b0);
                    const uint64_t q = mapq_quot(x, (uint32_t)b0);
                    mapq = q < 254 ? (uint32_t)q : 254u;
                }
                salt_result_t *out = results + r;
                if (sel) {                                                  // one 8-byte store per kept hit, all in one instruction
                    const uint32_t hidx = popc(sm & lt);
                    salt_hit_t hv; hv.pos = hp; hv.n_diff = (uint8_t)hn; hv.is_gap = 0; hv.strand = (uint16_t)hs;
                    out->hits[hs][hs ? hidx - nh0 : hidx] = hv;
                    out->hit_n_cigar[hidx] = 0;
                }
                // the 24 header bytes as six dwords, by lanes 0..5 of a wave or a quarter and 16..21 of a half-wave: where each kernel
                // had them when it was last timed; the other place was not measured
                const uint32_t t = lane - (GW == 32 ? 16u : 0u);
                if (t < 6) {
                    const uint32_t d = t == 0 ? q_pos
                                     : t == 1 ? (q_strand | (q_ndiff << 8) | (mapq << 24))                // strand, n_diff, is_gap = 0, mapq
                                     : t == 2 ? (uint32_t)b0
                                     : t == 3 ? (uint32_t)b1
                                     : t == 4 ? ((L - 1) << 16)                                           // seq_start = 0, seq_end
                                     : (nh0 | (nh1 << 8) | (1u << 16));                                   // n_hits[2], n_cigar = 1, skipped = 0
                    reinterpret_cast<uint32_t *>(out)[t] = d;
                } else if (t == 6) out->cigar[0] = (uint16_t)((L << 4) | 0u);
            }
        }
    }
    if (heavy) {
        if (lane == 0) queue_push(queue, ranges, ap.n_reads, r);
        return;                                                             // k_heavy does (and counts) all of it
    }
    if constexpr (INSTR) {
        stamp(SALT_CTR_LT_OUT);
        if (prof && lane == 0) atomicAdd(ctr + SALT_CTR_LT_SAMPLES, 1ull);
        if (ctr && lane == 0) {
            atomicAdd(ctr + SALT_CTR_SA_C, c_sa_c); atomicAdd(ctr + SALT_CTR_SA_R, c_sa_r);
            atomicAdd(ctr + SALT_CTR_VERIFY, c_verify);
            atomicAdd(ctr + SALT_CTR_READS, 1ull); atomicAdd(ctr + SALT_CTR_BASES, L); atomicAdd(ctr + SALT_CTR_LOCI, c_loci);
            atomicAdd(ctr + SALT_CTR_D_SA_LIGHT, c_sa_c + c_sa_r);
            atomicAdd(ctr + SALT_CTR_D_VERIFY_LIGHT, c_verify * (L <= 120 ? 4u : 8u));
            atomicAdd(ctr + SALT_CTR_D_OUT_LIGHT, 40u);                     // 24-byte header + CIGAR word + (typically one) 8-byte hit
        }
    }
}

// k_light: LT_WAVES independent reads (waves) per workgroup: half the workgroups to dispatch.  It takes what k_light2 does not: paired-end
// mates, reads above 120 / 248 bases or with more than 8 seed slots, and every step with the access counters on.
static constexpr int LT_WAVES = 2;
__global__ void __launch_bounds__(64 * LT_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_light(IndexView ix, AlignParams ap, const uint32_t *__restrict__ pm,
        const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r, salt_result_t *__restrict__ results,
        uint32_t *__restrict__ queue /* the segments */, QueueRange *__restrict__ ranges, unsigned long long *__restrict__ ctr)
{
    __shared__ LightLds<64> w[LT_WAVES];
    const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * LT_WAVES + (threadIdx.x >> 6));
    if (r < ap.n_reads) light_read<64, 0, true>(ix, ap, pm, sai_c, sai_r, results, queue, ranges, ctr, w[threadIdx.x >> 6], r);
}

// k_light2: TWO reads per wave (32 lanes each) for reads with few seed slots (spr <= 8; L <= 120 with LN = 4 lanes per located row: the
// 100-bp single-end case; L <= 248 with 8: 150-base reads).  The light pass is bound by instruction issue and by the dispatch of its
// workgroups; with two reads per wave both halve.  Same steps, same results.
// L2_WAVES waves per workgroup; each wave still works alone on its two reads (no block-level synchronisation).  Two waves per
// workgroup halve the number of workgroups the dispatcher has to place (5 x 10^5 -> 2.5 x 10^5 per batch): the kernel alone takes
// the same 0.48 ms, but with other batches' kernels on the GPU the step rate rises ~6 %; four are slower again.
template <int L2_WAVES, int LN = 4>
__global__ void __launch_bounds__(64 * L2_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_light2(IndexView ix, AlignParams ap, const uint32_t *__restrict__ pm,
         const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r, salt_result_t *__restrict__ results,
         uint32_t *__restrict__ queue /* the segments */, QueueRange *__restrict__ ranges)
{
    __shared__ LightLds<32> w[2 * L2_WAVES];
    const uint32_t h = 2u * (threadIdx.x >> 6) + (lane_id() >> 5);        // this half-wave among the workgroup's
    const uint32_t r = 2u * blockIdx.x * (uint32_t)L2_WAVES + h;
    if (r < ap.n_reads) light_read<32, LN, false>(ix, ap, pm, sai_c, sai_r, results, queue, ranges, nullptr, w[h], r);
}

// k_light4: FOUR reads per wave (16 lanes each) for reads with at most 4 seed slots and 120 bases: the 100-base single-end case at the
// default stride.  Such a read's seeds fill 16 lanes, its usual 4 - 6 located rows 16 - 24 lanes of the window check, its hits 12, its
// header 7; the instruction stream of a wave now serves four of them.  Each quarter works alone and takes its own path (skipped,
// queued, small, general).  A read with a list above L4_ROWS rows (and none above 64) is left to k_light_retry.
template <int L4_WAVES>
__global__ void __launch_bounds__(64 * L4_WAVES) __attribute__((amdgpu_waves_per_eu(8, 8)))
k_light4(IndexView ix, AlignParams ap, const uint32_t *__restrict__ pm,
         const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r, salt_result_t *__restrict__ results,
         uint32_t *__restrict__ queue /* the segments */, QueueRange *__restrict__ ranges)
{
    __shared__ LightLds<16> w[4 * L4_WAVES];
    const uint32_t q = 4u * (threadIdx.x >> 6) + (lane_id() >> 4);        // this quarter among the workgroup's
    const uint32_t r = 4u * blockIdx.x * (uint32_t)L4_WAVES + q;
    if (r < ap.n_reads) light_read<16, 4, false>(ix, ap, pm, sai_c, sai_r, results, queue, ranges, nullptr, w[q], r);
}

// k_light_retry: the half-wave body over the reads k_light4 left (retry_push), right behind it.  A fixed grid, a multiple of QUEUE_RANGES
// blocks of four half-waves: block b takes every (gridDim / QUEUE_RANGES)-th group of four of segment b % QUEUE_RANGES, and leaves at
// once when there is none.  The loop around the body keeps a few more registers alive than k_light2's 59; with the 64 of 8 waves a
// SIMD it spills, so this small launch is left to the compiler's own budget.
__global__ void __launch_bounds__(128)
k_light_retry(IndexView ix, AlignParams ap, const uint32_t *__restrict__ pm,
              const uint4 *__restrict__ sai_c, const uint4 *__restrict__ sai_r, salt_result_t *__restrict__ results,
              uint32_t *__restrict__ queue /* the segments */, QueueRange *__restrict__ ranges)
{
    __shared__ LightLds<32> w[4];
    const uint32_t h = 2u * (threadIdx.x >> 6) + (lane_id() >> 5);
    const uint32_t seg = blockIdx.x & (QUEUE_RANGES - 1u), step = 4u * (gridDim.x / QUEUE_RANGES);
    const uint32_t cnt = __hip_atomic_load(&ranges[seg].retry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t *src = retry_segs(queue, ap.n_reads) + (size_t)seg * qseg_cap(ap.n_reads);
    for (uint32_t i = 4u * (blockIdx.x / QUEUE_RANGES) + h; i < cnt; i += step) {
        light_read<32, 4, false>(ix, ap, pm, sai_c, sai_r, results, queue, ranges, nullptr, w[h], src[i]);
        WSYNC();
    }
}

// ---------------------------------------------------------------------------------------------
// k_pe_final: one thread per pair -- apply the first successful mate rescue (in the order pairing2 /
// pairing_singleton try them, alnpe.c:213-252, 420-470), then query_gen_cigar for the mates that keep their
// seed-and-verify mapping (query.c:282-296): "<L>M", or a k_cigar item when the mapping is gapped
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_pe_final(PackGeom pg, uint32_t n_pairs, const uint32_t *__restrict__ pm,
           salt_result_t *__restrict__ res, const PePair *__restrict__ pairs, const PeSwRes *__restrict__ sw,
           uint32_t *__restrict__ citems, uint32_t *__restrict__ ccount)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const PePair pr = pairs[p];
    int rescued = -1;
    for (int k = 0; k < pr.n_req && rescued < 0; ++k) {
        const PeSwRes &r = sw[pr.req0 + k];
        if (!r.ok) continue;
        rescued = pr.rescued[k];
        salt_result_t *q = res + 2 * p + rescued;
        const int b0 = r.score1, b1 = r.score2;
        uint32_t mapq = 0;
        if (b0 != 0) { const uint32_t x = (uint32_t)(b0 > b1 ? b0 - b1 : b1 - b0); const uint64_t v = mapq_quot(x, (uint32_t)b0); mapq = v < 254 ? (uint32_t)v : 254u; }
        q->b0 = b0; q->b1 = b1; q->mapq = (uint8_t)mapq;
        q->pos = (uint32_t)r.ref_begin + r.start; q->strand = (uint8_t)r.strand;
        q->seq_start = (uint16_t)r.read_begin; q->seq_end = (uint16_t)r.read_end;
        q->n_cigar = (uint8_t)r.n_cigar;
        for (uint32_t c = 0; c < r.n_cigar; ++c) q->cigar[c] = r.cigar[c];
    }
    for (int m = 0; m < 2; ++m) {
        if (m == rescued) continue;
        salt_result_t *q = res + 2 * p + m;
        const uint32_t L = pm[(uint64_t)(2 * p + m) * pg.pm_stride + 2 * pg.nw8];
        q->seq_start = 0; q->seq_end = (uint16_t)(L - 1);
        if (q->pos == 0xFFFFFFFFu) q->n_cigar = 0;
        else if (q->is_gap) { q->n_cigar = 0; citems[atomicAdd(ccount, 1u)] = ((2 * p + (uint32_t)m) << 3) | 0u; }
        else { q->cigar[0] = (uint16_t)((L << 4) | 0u); q->n_cigar = 1; }
    }
}

void launch_pe_final(const IndexView &ix, const PackGeom &pg, uint32_t n_pairs, const uint32_t *pm, salt_result_t *res, const PePair *pairs,
                     const PeSwRes *sw, void *lvtab, uint32_t *citems, PeCtl *ctl, uint32_t n_blocks, hipStream_t st)
{
    if (!n_pairs) return;
    hipLaunchKernelGGL(k_pe_final, dim3((n_pairs + 255) / 256), dim3(256), 0, st, pg, n_pairs, pm, res, pairs, sw, citems, &ctl->n_cigar);
    hipLaunchKernelGGL(k_cigar, dim3(n_blocks), dim3(64), 0, st, ix, pg, pm, res, citems, &ctl->n_cigar, &ctl->cigar_head, 2 * n_pairs, static_cast<LvTables *>(lvtab));
}

// ---------------------------------------------------------------------------------------------
// launch wrappers (called from salt_gpu.hip)
// ---------------------------------------------------------------------------------------------
uint32_t seed_wq_seg_cap(uint64_t items) { return (uint32_t)(((items + 255) / 256 + WQ_SEG - 1) / WQ_SEG) * 256u; }      // every seed of every block of a segment
// 32-byte records of both lists, in words.  Sized for the worst case, every seed walking in both searches: 64 bytes a seed, 512 MB for a
// workspace at 8 M seeds (10^6 reads of 100 bases at the default stride; 256 MB while a record was one uint4)
size_t seed_wq_words(uint64_t items) { return (size_t)2 * WQ_SEG * seed_wq_seg_cap(items) * WQ_REC * 4; }
uint32_t seed_wq_cnt_words() { return 2u * WQ_SEG * WQ_STRIDE; }
void launch_seed(const IndexView &ix, const SeedParams &sp, const uint32_t *tb, uint4 *sai_c, uint4 *sai_r, uint4 *wq, uint32_t *wq_cnt,
                 uint32_t walk_blocks, unsigned long long *ctr, hipStream_t st)
{
    uint64_t items = (uint64_t)sp.n_reads * 2u * sp.spr;
    if (!items) return;
    uint32_t blocks = (uint32_t)((items + 255) / 256);
    const uint32_t cap = seed_wq_seg_cap(items);
    hipLaunchKernelGGL(k_seed, dim3(blocks), dim3(256), 0, st, ix, sp, tb, sai_c, sai_r, wq, wq_cnt, cap, ctr);
    walk_blocks = (walk_blocks + WQ_SEG - 1) / WQ_SEG * WQ_SEG;
    static const uint32_t r_first = getenv("SALT_GPU_WALK_R_FIRST") && atoi(getenv("SALT_GPU_WALK_R_FIRST")) ? 1u : 0u;      // measurements: the R list in front of the C list
    hipLaunchKernelGGL(k_seed_walk, dim3(walk_blocks), dim3(256), 0, st, ix, sp, tb, sai_c, sai_r, wq, wq_cnt, cap, r_first, ctr);
}

void launch_light(const IndexView &ix, const AlignParams &ap, const uint32_t *pm, const uint8_t *, const uint32_t *, const uint4 *sai_c,
                  const uint4 *sai_r, salt_result_t *results, uint32_t *queue, SeCtl *ctl, uint32_t *qseg, QueueRange *ranges, unsigned long long *ctr, hipStream_t st)
{
    if (!ap.n_reads) return;
    static const bool no_half = getenv("SALT_GPU_NO_LIGHT2") && atoi(getenv("SALT_GPU_NO_LIGHT2"));
    static const bool no_quarter = getenv("SALT_GPU_NO_LIGHT4") && atoi(getenv("SALT_GPU_NO_LIGHT4"));
    if (!no_half && !no_quarter && !ctr && !SALT_DIAG_VAL(ap.dbg_stop) && ap.spr <= (uint32_t)L4_SLOTS && ap.pg.nw8 <= 15) {  // at most 120 bases and 4 seed slots: four per wave
        static const int wv = getenv("SALT_GPU_L4_WAVES") ? atoi(getenv("SALT_GPU_L4_WAVES")) : 2;
        if (wv == 1) hipLaunchKernelGGL(k_light4<1>, dim3((ap.n_reads + 3) / 4), dim3(64), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges);
        else if (wv == 4) hipLaunchKernelGGL(k_light4<4>, dim3((ap.n_reads + 15) / 16), dim3(256), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges);
        else hipLaunchKernelGGL(k_light4<2>, dim3((ap.n_reads + 7) / 8), dim3(128), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges);
        // the reads with a list a quarter cannot hold (3 % of the GRCh38-scale batches): as many blocks a CU as its registers let a CU
        // hold at once (8; SALT_GPU_L4_RETRY_PER_CU for measurements), rounded up to whole rounds over the segments
        static const uint32_t retry_blocks = [] {
            int dev = 0, cus = 0, per_cu = getenv("SALT_GPU_L4_RETRY_PER_CU") ? atoi(getenv("SALT_GPU_L4_RETRY_PER_CU")) : 8;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = (int)QUEUE_RANGES;
            if (per_cu < 1 || per_cu > 64) per_cu = 8;
            return ((uint32_t)(cus * per_cu) + QUEUE_RANGES - 1u) / QUEUE_RANGES * QUEUE_RANGES;
        }();
        hipLaunchKernelGGL(k_light_retry, dim3(retry_blocks), dim3(128), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges);
    } else if (!no_half && !ctr && !SALT_DIAG_VAL(ap.dbg_stop) && ap.spr <= (uint32_t)L2_SLOTS && ap.pg.nw8 <= 31) {          // reads of at most 120 / 248 bases with at most 8 seed slots: two per wave
        static const int wv = getenv("SALT_GPU_L2_WAVES") ? atoi(getenv("SALT_GPU_L2_WAVES")) : 2;
        if (ap.pg.nw8 > 15) hipLaunchKernelGGL((k_light2<2, 8>), dim3((ap.n_reads + 3) / 4), dim3(128), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges);
        else if (wv == 1) hipLaunchKernelGGL(k_light2<1>, dim3((ap.n_reads + 1) / 2), dim3(64), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges);
        else hipLaunchKernelGGL(k_light2<2>, dim3((ap.n_reads + 3) / 4), dim3(128), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges);
    } else
        hipLaunchKernelGGL(k_light, dim3((ap.n_reads + LT_WAVES - 1) / LT_WAVES), dim3(64 * LT_WAVES), 0, st, ix, ap, pm, sai_c, sai_r, results, qseg, ranges, ctr);
    hipLaunchKernelGGL(k_queue_pack, dim3(QUEUE_RANGES), dim3(256), 0, st, qseg, ranges, ap.n_reads, queue, ctl);
}
size_t queue_words(uint32_t max_reads) { return (size_t)max_reads * 2 + (size_t)2 * QUEUE_RANGES * qseg_cap(max_reads); }     // flat queue | overflow queue | segments | retry segments

// ---------------------------------------------------------------------------------------------
// k_diag_rule: unit access to rule_unsorted / rule_sparse (tests only).  One wave per case; out[case] = any, best_pos,
// best_v, n_hits, a0, bound_out, then NHIT x (hit_pos, hit_nd).  mode 0: rule_unsorted<3, false>, 1: rule_sparse<3, false>,
// 2: rule_unsorted<LLV_K, true>, 3: rule_sparse<3, false, 32> as k_light2 runs it -- two cases per wave, 2b and 2b + 1 in the halves
// of block b, each half with its own hit arrays, 4: rule_sparse<3, false, 16> as k_light4 runs it -- four cases per wave, 4b .. 4b + 3
// in the quarters of block b, each quarter with its own hit arrays, 5: rule_unsorted<LLV_K, true, GAPFIN_B> as k_gapfin runs it on a
// list in global memory, the first batch of rows asked for ahead of the call
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_diag_rule(uint32_t n_cases, const uint32_t *__restrict__ pos, const uint8_t *__restrict__ val, const uint32_t *__restrict__ offs,
            const uint32_t *__restrict__ bound_in, uint32_t L, uint32_t ref_len, int mode, uint32_t *__restrict__ out)
{
    __shared__ uint32_t hit_pos_s[4][NHIT];
    __shared__ uint8_t hit_nd_s[4][NHIT];
    const uint32_t gw = mode == 3 ? 32u : mode == 4 ? 16u : 64u, half = lane_id() / gw, lane = lane_id() & (gw - 1u);
    const uint32_t c = (64u / gw) * blockIdx.x + half;
    if (c >= n_cases) return;
    uint32_t *hit_pos = hit_pos_s[half];
    uint8_t *hit_nd = hit_nd_s[half];
    const uint32_t o = offs[c], n = offs[c + 1] - o;
    uint32_t bound = bound_in[c], bp = 0, bv = 0, nh = 0, a0 = 0;
    bool any = false;
    if (lane < NHIT) { hit_pos[lane] = 0; hit_nd[lane] = 0; }
    WSYNC();
    if (mode == 0) rule_unsorted<3, false>(pos + o, val + o, n, L, ref_len, bound, any, bp, bv, nh, a0, hit_pos, hit_nd);
    else if (mode == 1) rule_sparse<3, false>(pos + o, val + o, n, L, ref_len, bound, any, bp, bv, nh, a0, hit_pos, hit_nd);
    else if (mode == 3) rule_sparse<3, false, 32>(pos + o, val + o, n, L, ref_len, bound, any, bp, bv, nh, a0, hit_pos, hit_nd);
    else if (mode == 4) rule_sparse<3, false, 16>(pos + o, val + o, n, L, ref_len, bound, any, bp, bv, nh, a0, hit_pos, hit_nd);
    else if (mode == 5) {
        RowBatch<GAPFIN_B> first;
        if (n) rows_fetch<GAPFIN_B>(first, pos + o, val + o, n, 0u);
        rule_unsorted<LLV_K, true, GAPFIN_B>(pos + o, val + o, n, L, ref_len, bound, any, bp, bv, nh, a0, hit_pos, hit_nd, &first);
    }
    else rule_unsorted<LLV_K, true>(pos + o, val + o, n, L, ref_len, bound, any, bp, bv, nh, a0, hit_pos, hit_nd);
    WSYNC();
    uint32_t *w = out + (size_t)c * (6 + 2 * NHIT);
    if (lane == 0) { w[0] = any; w[1] = any ? bp : 0; w[2] = any ? bv : 0; w[3] = nh; w[4] = nh ? a0 : 0; w[5] = bound; }
    if (lane < NHIT) { w[6 + 2 * lane] = lane < nh ? hit_pos[lane] : 0; w[7 + 2 * lane] = lane < nh ? hit_nd[lane] : 0; }
}

void launch_diag_rule(uint32_t n_cases, const uint32_t *pos, const uint8_t *val, const uint32_t *offs, const uint32_t *bound_in,
                      uint32_t L, uint32_t ref_len, int mode, uint32_t *out, hipStream_t st)
{
    const uint32_t blocks = mode == 3 ? (n_cases + 1) / 2 : mode == 4 ? (n_cases + 3) / 4 : n_cases;
    if (n_cases) hipLaunchKernelGGL(k_diag_rule, dim3(blocks), dim3(64), 0, st, n_cases, pos, val, offs, bound_in, L, ref_len, mode, out);
}
uint32_t diag_rule_words() { return 6 + 2 * NHIT; }

// ---------------------------------------------------------------------------------------------
// k_diag_lv: unit access to the verify / LV device functions for the golden vectors (tests only)
// ---------------------------------------------------------------------------------------------
// One case per block for mismatch_capped, lv_wave and lv_cigar.  lv_lanes takes one candidate per lane, staged by lane_text as k_gap
// and k_heavy stage theirs: the block of case c runs it for the lane_n[c] cases lane_case[lane_first[c] ..) -- 64 different cases
// of one (L, k), each lane with its own read and window, or case c alone in every lane -- and writes their out[.][2]; a case
// some other block serves has lane_n = 0.  Cases beyond the lane kernel's limits get -2 there.
__host__ __device__ static inline bool lv_fit_dev(uint32_t L, uint32_t k) { return k <= (uint32_t)LLV_K && L + 4 <= 8u * (LLV_TW - 1); }
bool lv_lanes_fit(uint32_t L, uint32_t k) { return lv_fit_dev(L, k); }

__global__ void __launch_bounds__(64)
k_diag_lv(IndexView ix, uint32_t n_cases, const uint32_t *__restrict__ pos, const uint32_t *__restrict__ kdiff,
          const uint8_t *__restrict__ seqs, const uint32_t *__restrict__ offs, const uint32_t *__restrict__ lane_first,
          const uint32_t *__restrict__ lane_n, const uint32_t *__restrict__ lane_case, int32_t *__restrict__ out /* [n][4] */,
          uint16_t *__restrict__ cig_out /* [n][64] */, LvTables *__restrict__ lvtab, int lds_tab)
{
    __shared__ WaveLds w;
    __shared__ LvTablesLds tl;                                             // lds_tab: lv_cigar's tables as k_cigar places them
    __shared__ uint32_t lane_pm[LLV_N][LLV_PW];
    const uint32_t c = blockIdx.x, lane = lane_id();
    if (c >= n_cases) return;
    const uint32_t off = offs[c], L = offs[c + 1] - off, p = pos[c];
    const uint32_t nw = (L + 7) >> 3;
    auto pm_word = [&](uint32_t o, uint32_t j) -> uint32_t {
        uint32_t word = 0;
        for (uint32_t q = 0; q < 8; ++q) {
            uint32_t i = j * 8 + q, cc = i < L ? seqs[o + i] : 5u;
            word |= (cc < 4 ? (1u << cc) : (cc == 4 ? 15u : 0u)) << (4 * q);
        }
        return word;
    };
    for (uint32_t j = lane; j < nw; j += 64) w.pm[0][j] = pm_word(off, j);
    WSYNC();
    int32_t v = -2, e_wave = -1, n_cig = -2;
    if (p + L <= ix.ref_len) v = (int32_t)mismatch_capped(ix, w.pm[0], L, p);
    const bool in_range = !(p > ix.ref_len || p + L + 4 > ix.ref_len);
    const int k = (int)kdiff[c];
    if (in_range) {
        lv_unpack(ix.ref, w, 0, L, p);
        e_wave = lv_wave(w.u.lvb.T, (int)L + 4, w.u.lvb.P, (int)L, k, LvTabRef{ nullptr, nullptr }).e;
        WSYNC();
    }
    const bool fit = lv_fit_dev(L, (uint32_t)k);
    const uint32_t gn = fit ? lane_n[c] : 0u;
    if (gn) {                                                             // gn is 1 or LLV_N
        const uint32_t m = lane_case[lane_first[c] + lane % gn], mo = offs[m], mp = pos[m];      // same L and k as case c
        lane_pattern(lane_pm[lane], nw, 0u, 1u, [&](uint32_t j) { return pm_word(mo, j); });
        const bool act = !(mp > ix.ref_len || mp + L + 4 > ix.ref_len);   // ed_diff guard, as k_gap has it
        if (act) lane_text(ix.ref, w.u.llv.T + lane, mp, L + 4);
        WSYNC();
        const uint32_t el = lv_lanes(w.u.llv, lane_pm[lane], (int)L, (int)L + 4, k, act);
        if (lane < gn) out[(size_t)m * 4 + 2] = el == 255 ? -1 : (int32_t)el;
        WSYNC();
    }
    if (in_range && e_wave >= 0 && e_wave < LVK) {
        lv_cigar(ix.ref, w, lds_tab && e_wave <= LLV_K ? lv_tab(tl) : lv_tab(lvtab + blockIdx.x), 0, L, p, e_wave);
        n_cig = w.n_cig;
        if (lane < (uint32_t)w.n_cig) cig_out[(size_t)c * SALT_MAX_CIGAR_OPS + lane] = w.cig[lane];
    }
    if (lane == 0) {
        out[(size_t)c * 4 + 0] = v; out[(size_t)c * 4 + 1] = e_wave; out[(size_t)c * 4 + 3] = n_cig;
        if (!fit) out[(size_t)c * 4 + 2] = -2;
    }
}

size_t lv_table_bytes() { return sizeof(LvTables); }

void launch_diag_lv(const IndexView &ix, uint32_t n, const uint32_t *pos, const uint32_t *kdiff, const uint8_t *seqs,
                    const uint32_t *offs, const uint32_t *lane_first, const uint32_t *lane_n, const uint32_t *lane_case,
                    int32_t *out, uint16_t *cig, void *lvtab, int lds_tab, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(k_diag_lv, dim3(n), dim3(64), 0, st, ix, n, pos, kdiff, seqs, offs, lane_first, lane_n, lane_case, out, cig,
                              static_cast<LvTables *>(lvtab), lds_tab);
}

// k_diag_verify: unit access to the candidate verifiers (tests only).  One wave per case: the read seqs[offs[c]..offs[c+1]) against
// candidates cand[coffs[c]..coffs[c+1]) (at most 256) on the caller's mixRef.  mode 0: mismatch_capped per lane, 1: verify_quads<8>
// (4 lanes per candidate, L <= 120), 2: verify_quads<8, 8> (L <= 248), 3 / 4: verify_quads_2<4> / <8> with the list split between the
// "strands" (both use the same read), 5 / 6: verify_quads_2<4, 32> / <8, 32> as k_light2 runs them -- two cases per wave, 2b and 2b + 1
// in the halves of block b, each set up like a case of modes 3 / 4; 7: verify_quads_2<4, 16> as k_light4 runs it -- four cases per
// wave, in the quarters of block b.  out[i] = 0..3 or 255.  Candidates >= ref_len (a locate that wrapped
// below 0, alnse.c:672-673) must come back 255 WITHOUT being used as an address: the test's mixRef is a few KB, so a regression reads
// far outside of it only by value.
__global__ void __launch_bounds__(64)
k_diag_verify(const uint32_t *__restrict__ ref, uint32_t ref_len, uint32_t n_cases, const uint8_t *__restrict__ seqs, const uint32_t *__restrict__ offs,
              const uint32_t *__restrict__ cand, const uint32_t *__restrict__ coffs, int mode, uint8_t *__restrict__ out)
{
    __shared__ uint32_t pm_s[4][64];
    __shared__ uint32_t loci_s[4][256];
    __shared__ uint8_t val_s[4][256];
    const uint32_t gw = mode == 7 ? 16u : mode >= 5 ? 32u : 64u, half = lane_id() / gw, lane = lane_id() & (gw - 1u);
    const uint32_t c = (64u / gw) * blockIdx.x + half;
    if (c >= n_cases) return;
    uint32_t *pm = pm_s[half], *loci = loci_s[half];
    uint8_t *val = val_s[half];
    const uint32_t off = offs[c], L = offs[c + 1] - off, c0 = coffs[c];
    uint32_t n = coffs[c + 1] - c0;
    if (n > 256) n = 256;
    const uint32_t nw = (L + 7) >> 3;
    for (uint32_t j = lane; j < 64; j += gw) {
        uint32_t word = 0;
        for (uint32_t q = 0; q < 8 && j < nw; ++q) {
            const uint32_t i = j * 8 + q, cc = i < L ? seqs[off + i] : 5u;
            word |= (cc < 4 ? (1u << cc) : (cc == 4 ? 15u : 0u)) << (4 * q);
        }
        pm[j] = word;
    }
    for (uint32_t i = lane; i < n; i += gw) { loci[i] = cand[c0 + i]; val[i] = 77; }
    WSYNC();
    IndexView ix; ix.ref = ref; ix.ref_len = ref_len;
    if (mode == 0) { for (uint32_t i = lane; i < n; i += 64) val[i] = (uint8_t)mismatch_capped(ix, pm, L, loci[i]); }
    else if (mode == 1) verify_quads<8>(ref, ref_len, pm, L, loci, n, val);
    else if (mode == 2) verify_quads<8, 8>(ref, ref_len, pm, L, loci, n, val);
    else if (mode == 3) verify_quads_2(ref, ref_len, pm, pm, L, loci, n / 2, loci + n / 2, n - n / 2, val, val + n / 2);
    else if (mode == 4) verify_quads_2<8>(ref, ref_len, pm, pm, L, loci, n / 2, loci + n / 2, n - n / 2, val, val + n / 2);
    else if (mode == 5) verify_quads_2<4, 32>(ref, ref_len, pm, pm, L, loci, n / 2, loci + n / 2, n - n / 2, val, val + n / 2);
    else if (mode == 6) verify_quads_2<8, 32>(ref, ref_len, pm, pm, L, loci, n / 2, loci + n / 2, n - n / 2, val, val + n / 2);
    else verify_quads_2<4, 16>(ref, ref_len, pm, pm, L, loci, n / 2, loci + n / 2, n - n / 2, val, val + n / 2);
    WSYNC();
    for (uint32_t i = lane; i < n; i += gw) out[c0 + i] = val[i];
}
void launch_diag_verify(const uint32_t *ref, uint32_t ref_len, uint32_t n_cases, const uint8_t *seqs, const uint32_t *offs, const uint32_t *cand,
                        const uint32_t *coffs, int mode, uint8_t *out, hipStream_t st)
{
    const uint32_t blocks = mode == 7 ? (n_cases + 3) / 4 : mode >= 5 ? (n_cases + 1) / 2 : n_cases;
    if (n_cases) hipLaunchKernelGGL(k_diag_verify, dim3(blocks), dim3(64), 0, st, ref, ref_len, n_cases, seqs, offs, cand, coffs, mode, out);
}

// ---------------------------------------------------------------------------------------------
// k_polish (row N4): the re-scoring step of the reference's SAM post-processor (Polish_src/polish.c:461-497, 190-249).
// One wave per item = (read, strand, genome offset): the plain edit distance (k <= 13) between the read and the bases at that offset
// -- stock Landau-Vishkin on EQUAL bytes (Polish_src/lv.c), which lv_wave computes when both strings are one-hot: equal <=> AND != 0
// -- and, for the items that ask for it, the CIGAR (computeEditDistanceWithCigar with useM: first "e plain mismatches on diagonal 0 ->
// <L>M", lv.c:274-296, then the traceback).  The reference's window buffer is calloc'ed, so what lies behind the text reads as 'A'
// (code 0) there; a window clipped at the genome end keeps the previous hit's bytes behind the clip (polish.c:84-92): the host hands
// those few windows over explicitly (`pool`).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_polish(const uint8_t *__restrict__ pac, const uint8_t *__restrict__ codes, const uint32_t *__restrict__ offs, const salt_polish_item_t *__restrict__ items,
         uint32_t n_items, const uint8_t *__restrict__ pool, uint32_t pool_stride, int want_cigar, int32_t *__restrict__ dist,
         uint16_t *__restrict__ cigars, uint8_t *__restrict__ n_cigar, LvTables *__restrict__ tabs)
{
    __shared__ LvBytes s;
    __shared__ int s_n;
    const uint32_t lane = lane_id();
    for (uint32_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const salt_polish_item_t x = items[it];
        const uint32_t o = offs[x.read], L = offs[x.read + 1] - o, tl = x.tlen;
        WSYNC();
        for (uint32_t i = lane; i < L + 48; i += 64) {
            uint8_t pv = 1;                                                    // behind the read: calloc'ed zeros = 'A'
            if (i < L) { const uint8_t c = x.strand ? codes[o + L - 1 - i] : codes[o + i]; pv = c < 4 ? (uint8_t)(1u << (x.strand ? 3 - c : c)) : (uint8_t)(x.strand ? 0x20 : 0x10); }
            s.P[i] = pv;
        }
        for (uint32_t i = lane; i < L + 48; i += 64) {
            uint8_t tv = 1;
            if (x.pool != 0xFFFFFFFFu) { if (i < pool_stride) tv = (uint8_t)(1u << (pool[(uint64_t)x.pool * pool_stride + i] & 3u)); }
            else if (i < tl) { const uint64_t l = (uint64_t)x.offset + i; tv = (uint8_t)(1u << ((pac[l >> 2] >> ((~l & 3u) << 1)) & 3u)); }
            s.T[i] = tv;
        }
        WSYNC();
        LvTables *tab = want_cigar ? tabs + blockIdx.x : nullptr;
        const LvEnd fin = lv_wave(s.T, (int)tl, s.P, (int)L, (int)x.k, lv_tab(tab));
        const int e = fin.e, d_fin = fin.d_fin;
        if (lane == 0) dist[it] = e;
        if (want_cigar) {
            __threadfence_block();
            WSYNC();
            // e plain mismatches on diagonal 0?  (lv.c:274-296)
            const int end0 = (int)(L < tl ? L : tl);
            int straight = 0;
            for (int i = (int)lane; i < end0; i += 64) straight += s.P[i] != s.T[i];
            for (int w = 32; w > 0; w >>= 1) straight += __shfl_xor(straight, w);
            straight += (int)L - end0;
            if (lane == 0) {
                int n = 0;
                uint16_t *cg = cigars + (uint64_t)it * SALT_MAX_CIGAR_OPS;
                if (e == 0 || (e > 0 && straight == e)) cg[n++] = (uint16_t)((L << 4) | 0u);
                else if (e > 0) {
                    char act[LVK + 1]; int matched[LVK + 1];
                    int cd = d_fin;
                    for (int ce = e; ce >= 1; --ce) {
                        const char a = tab->A[ce][cd + 31];
                        act[ce] = a;
                        const int cur = tab->L[ce][cd + 31];
                        if (a == 'I') { matched[ce] = cur - tab->L[ce - 1][cd + 1 + 31] - 1; cd += 1; }
                        else if (a == 'D') { matched[ce] = cur - tab->L[ce - 1][cd - 1 + 31]; cd -= 1; }
                        else { matched[ce] = cur - tab->L[ce - 1][cd + 31] - 1; }
                    }
                    int acc = tab->L[0][31];
                    int ce = 1;
                    while (ce <= e) {
                        const char a = act[ce]; int cnt = 1;
                        while (ce + 1 <= e && matched[ce] == 0 && act[ce + 1] == a) { ++cnt; ++ce; }
                        if (a == 'X') acc += cnt;
                        else {
                            if (acc != 0 && n < SALT_MAX_CIGAR_OPS) cg[n++] = (uint16_t)((acc << 4) | 0);
                            acc = 0;
                            if (n < SALT_MAX_CIGAR_OPS) cg[n++] = (uint16_t)((cnt << 4) | (a == 'I' ? 1 : 2));
                        }
                        if (matched[ce] > 0) acc += matched[ce];
                        ++ce;
                    }
                    if (acc != 0 && n < SALT_MAX_CIGAR_OPS) cg[n++] = (uint16_t)((acc << 4) | 0);
                }
                n_cigar[it] = (uint8_t)n;
                s_n = n;
            }
            WSYNC();
        }
    }
}
void launch_polish(const uint8_t *pac, const uint8_t *codes, const uint32_t *offs, const salt_polish_item_t *items, uint32_t n_items, const uint8_t *pool,
                   uint32_t pool_stride, int want_cigar, int32_t *dist, uint16_t *cigars, uint8_t *n_cigar, void *tabs, uint32_t n_blocks, hipStream_t st)
{
    if (n_items) hipLaunchKernelGGL(k_polish, dim3(n_blocks), dim3(64), 0, st, pac, codes, offs, items, n_items, pool, pool_stride, want_cigar, dist, cigars, n_cigar,
                                    static_cast<LvTables *>(tabs));
}

// first 128 bytes of every result row, densely packed (what the host needs of nearly every row)
__global__ void __launch_bounds__(256)
k_heads(const salt_result_t *__restrict__ res, uint32_t n, uint4 *__restrict__ heads)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n * 8u) return;
    const uint32_t i = (uint32_t)(t >> 3), c = (uint32_t)t & 7u;
    heads[t] = reinterpret_cast<const uint4 *>(res + i)[c];
}
void launch_heads(const salt_result_t *res, uint32_t n, uint8_t *heads, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(k_heads, dim3((uint32_t)(((uint64_t)n * 8u + 255) / 256)), dim3(256), 0, st, res, n, reinterpret_cast<uint4 *>(heads));
}

uint32_t heavy_blocks_per_cu()
{
    static int cached = 0;
    if (!cached) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_heavy, 64, 0) != hipSuccess || n < 1) n = 8;
        cached = n;
    }
    return (uint32_t)cached;
}

void launch_heavy(const IndexView &ix, const AlignParams &ap, const uint32_t *pm, const uint4 *sai_c,
                  const uint4 *sai_r, salt_result_t *results, const uint32_t *queue, unsigned long long *ctr,
                  uint32_t n_blocks, uint32_t gap_blocks, uint32_t cigar_blocks, void *lvtab, const GapBufs &g_in, uint32_t *ovq, QueueRange *ranges, uint8_t *pe_scr, hipEvent_t *ev3, hipStream_t st)
{
    if (!ap.n_reads) { if (ev3) for (int i = 0; i < 3; ++i) hipEventRecord(ev3[i], st); return; }
    uint32_t blocks = n_blocks < ap.n_reads ? n_blocks : ap.n_reads;
    LvTables *tab = static_cast<LvTables *>(lvtab);
    GapBufs g = g_in; g.ovq = ovq; g.ranges = ranges;
    // The usual shape (7.5 KB of LDS per block) when the batch fits it: at most 32 seed slots per strand and k_gap's buffers to hand gapped
    // reads to; the few reads it cannot finish (no k_gap slot left) wait in the overflow queue for the pass right behind it, which runs
    // the all-in-one shape (18.6 KB) and leaves at once when the queue is empty.  SALT_GPU_HEAVY_BIG=1: the all-in-one shape for everything.
    static const bool force_big = getenv("SALT_GPU_HEAVY_BIG") && atoi(getenv("SALT_GPU_HEAVY_BIG"));
    const bool se_glob = !ap.pe && pe_scr != nullptr;                  // single end, -m above the LDS list
    if (se_glob) {
        hipLaunchKernelGGL(k_heavy_glob, dim3(blocks), dim3(64), 0, st, ix, ap, pm, sai_c, sai_r, results, queue, ctr, tab, g, pe_scr, 0);
    }
    const bool small = !se_glob && !force_big && g.cap > 0 && ovq != nullptr && ap.spr <= (uint32_t)WaveLdsSmall::N_SLOTS;
    if (small) {
        if (ap.pe) hipLaunchKernelGGL(k_heavy_pe, dim3(blocks), dim3(64), 0, st, ix, ap, pm, sai_c, sai_r, results, queue, ctr, tab, g, pe_scr, 0);
        else     hipLaunchKernelGGL(k_heavy, dim3(blocks), dim3(64), 0, st, ix, ap, pm, sai_c, sai_r, results, queue, ctr, tab, g, pe_scr, 0);
    }
    // (the overflow pass on a small grid: it is empty nearly always, and 1 536 blocks of 18.6 KB each that only look at a counter cost 70 us)
    const uint32_t big_blocks = small && blocks > 256u ? 256u : blocks;
    if (se_glob) { }                                                    // (done above)
    else if (ap.pe) hipLaunchKernelGGL(k_heavy_pe_big, dim3(big_blocks), dim3(64), 0, st, ix, ap, pm, sai_c, sai_r, results, queue, ctr, tab, g, pe_scr, small ? 1 : 0);
    else     hipLaunchKernelGGL(k_heavy_big, dim3(big_blocks), dim3(64), 0, st, ix, ap, pm, sai_c, sai_r, results, queue, ctr, tab, g, pe_scr, small ? 1 : 0);
    if (ev3) hipEventRecord(ev3[0], st);
    if (!g.cap) { if (ev3) { hipEventRecord(ev3[1], st); hipEventRecord(ev3[2], st); } return; }
    // the deferred gapped passes: distances by (read, strand, 64 candidates), one finishing wave per read, one traceback per wave.
    // Grids (the workspace sets them): k_gap has many ~70 us items and wants every wave.  k_gapfin: a quarter of k_heavy's grid, about
    // three reads a block on the flagship step; two and four times the waves did not move it (its time is its longest block, not its
    // throughput).  k_cigar: cigar_blocks <= n_blocks (lvtab has n_blocks tables), by default all of them, 9.6 KB of LDS a block with
    // the traceback tables, 16 blocks a CU: a block's first item is its own index and costs no atomic (sw_pull), so with more blocks
    // than items nobody touches the queue head and nobody runs a second traceback (profiles/r19: 26 us alone against 84 on half the
    // blocks, where every block went through the head after its first item).
    if (cigar_blocks == 0 || cigar_blocks > n_blocks) cigar_blocks = n_blocks;
    hipLaunchKernelGGL(k_gap, dim3(gap_blocks), dim3(64), 0, st, ix, ap, pm, g);
    if (ev3) hipEventRecord(ev3[1], st);
    hipLaunchKernelGGL(k_gapfin, dim3((n_blocks + 3) / 4), dim3(64), 0, st, ix, ap, pm, results, g, ctr);
    if (ev3) hipEventRecord(ev3[2], st);
    hipLaunchKernelGGL(k_cigar, dim3(cigar_blocks), dim3(64), 0, st, ix, ap.pg, pm, results, g.cq, &g.gctl->cigar_items, &g.gctl->cigar_head, g.cap * (1u + SALT_MAX_HITS), tab);
}

GapBufs gap_bufs_layout(uint8_t *base, uint32_t cap, SeCtl *gctl, size_t *bytes)
{
    GapBufs g; size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off = (off + n + 255) & ~(size_t)255; return base ? base + o : nullptr; };
    // an SE read needs at most 2 x 1000 entries; PE mates share the pool.  Beyond 32 768 slots the pool stops growing with them
    // (64 M rows = 335 MB): a batch in which EVERY read needs the gapped pass still finds a slot per read, and rows for all of them
    // unless they are repeat reads throughout (then the rest takes the overflow pass)
    { const uint64_t want = (uint64_t)cap * 2u * (uint64_t)MAXLOC; g.pool = (uint32_t)(want < (1ull << 26) ? want : (1ull << 26)); }
    g.items_cap = g.pool / LLV_N + 2u * cap;
    g.gq = reinterpret_cast<uint32_t *>(take((size_t)cap * 4));
    g.gn = reinterpret_cast<uint32_t *>(take((size_t)cap * 2 * 4));
    g.goff = reinterpret_cast<uint32_t *>(take((size_t)cap * 2 * 4));
    g.gloci = reinterpret_cast<uint32_t *>(take((size_t)g.pool * 4));
    g.ge = take((size_t)g.pool);
    g.gitems = reinterpret_cast<uint32_t *>(take((size_t)g.items_cap * 4));
    g.cq = reinterpret_cast<uint32_t *>(take((size_t)cap * (1 + SALT_MAX_HITS) * 4));
    g.gctl = gctl; g.cap = cap; g.ovq = nullptr;
    if (bytes) *bytes = off;
    return g;
}


} // namespace salt
