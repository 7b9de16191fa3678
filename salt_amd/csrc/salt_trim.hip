// salt_amd/csrc/salt_trim.hip -- adapter and quality trimming of the parsed reads, on the device (gfx950).
//
// k_fq_trim stands between k_fq_parse and the scan of the lengths: it moves seq_off and qual_off of every FqRec forward, shortens len, and
// every later stage (k_fq_codes, the aligner, the SAM / BAM / polish writers, the tallies) sees the trimmed read.  No byte of the FASTQ moves.
// The rule is salt_trim_rule.h, the header the host twin compiles too; this file is the rule's wave-wide form.
//
// One wave per read.  The pieces of the rule are wave-uniform (the span, the counters) or one item per lane:
//   quality   lane k holds Q - q of base end - 1 - (64 t + k): an inclusive scan over the lanes gives the partial sums, a ballot finds the
//             first negative one, a max over the lanes in front of it and a second ballot find the argmax that comes first.
//   adapter   lane k is the start 64 t + k.  The read is never packed into memory: a ballot over the 64 lanes' codes IS the packed read, one
//             64-bit word (in scalar registers, the same for all lanes) per bit plane -- low bit, high bit, "not ACGT".  A lane's window of
//             up to 64 bases is this tile's word shifted right by its lane, joined with the next tile's: one XOR per plane against the
//             adapter's planes, an OR, a mask of ov bits and a popcount are the mismatches of the whole overlap.  A ballot over the verdicts
//             and its lowest bit are the leftmost accepted start.
// So a 150-base read costs three byte loads a lane and some forty vector instructions: no LDS, no loop over letters.
//
// k_fq_trim_pair takes k_fq_trim's place in a paired-end call when the pair rule (step 2p) is on: one wave per PAIR.  It runs the two steps
// above for both mates, then
//   pair      both reads as planes by the same ballots, mate 2 loaded back to front with its code complemented so that the ballots deliver
//             R; the words (four planes of 64 columns: lo, hi, nn and "inside the span") go to LDS, 512 bytes a wave.  Lane k of turn t is the
//             candidate I = (e1 + e2 - P) - (64 t + k): for every word of mate 1 it takes R's window at its own shift (two neighbouring
//             words joined) and counts mismatches and compared columns by popcount (trim_pair_eval, the host twin's).  A ballot of the
//             verdicts and its lowest lane are the largest accepted I; the scan ends at the first turn with one.
// then the adapter step for both mates on what is left, the floor, and the records.
#include <hip/hip_runtime.h>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_trim_rule.h"

namespace salt {

static constexpr uint32_t TRIM_BLOCKS = 2048;          // 8 blocks of 4 waves per CU: the kernel waits on byte loads, so all 32 wave slots of a CU are wanted

__device__ __forceinline__ uint32_t first_lane(unsigned long long m) { return (uint32_t)__ffsll((long long)m) - 1u; }
// letters [at, at + 64) of the span of n letters that starts at s: a lane each, the planes by ballot (behind the span: nn)
__device__ __forceinline__ TrimPlanes tile_planes(const uint8_t *s, uint32_t n, uint32_t at, uint32_t lane)
{
    const uint32_t j = at + lane;
    const uint32_t c = at < n && j < n ? trim_code(s[j]) : 4u;
    TrimPlanes p; p.lo = __ballot(c & 1u); p.hi = __ballot(c & 2u); p.nn = __ballot(c & 4u);
    return p;
}

// step 2 by a wave: the end the quality rule leaves of the span [beg, end)
__device__ __forceinline__ uint32_t wave_quality(const TrimRule &R, const uint8_t *qual, uint32_t beg, uint32_t end, uint32_t lane)
{
    long long carry = 0, best = 0;
    uint32_t cut = end;
    const uint32_t n = end - beg;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t step = base + lane;
        const bool valid = step < n;
        long long s = valid ? (long long)R.qual - trim_q(qual[end - 1u - step]) : 0;
        for (int o = 1; o < 64; o <<= 1) { const long long v = __shfl_up(s, o); if (lane >= (uint32_t)o) s += v; }
        s += carry;
        const unsigned long long neg = __ballot(valid && s < 0);
        const bool ok = valid && (!neg || lane < first_lane(neg));       // the sums the walk reaches before it stops
        long long m = ok ? s : 0;
        for (int o = 32; o > 0; o >>= 1) { const long long v = __shfl_xor(m, o); m = v > m ? v : m; }
        if (m > best) { best = m; cut = end - 1u - (base + first_lane(__ballot(ok && s == m))); }      // ties: the first the walk meets
        if (neg) break;
        carry = __shfl(s, 63);
    }
    return cut;
}

// step 3 by a wave: the end the adapter search leaves of the span [beg, end), end > beg, A = the adapter's length >= 1
__device__ __forceinline__ uint32_t wave_adapter(const TrimRule &R, uint32_t mate, const uint8_t *seq, uint32_t beg, uint32_t end, uint32_t lane)
{
    const uint32_t A = R.a_len[mate];
    const uint64_t a_lo = R.a_lo[mate], a_hi = R.a_hi[mate];
    const uint8_t *s = seq + beg;
    const uint32_t n = end - beg;
    TrimPlanes w0 = tile_planes(s, n, 0, lane);
    for (uint32_t at = 0; at < n; at += 64) {
        const TrimPlanes w1 = tile_planes(s, n, at + 64u, lane);
        const uint32_t p = at + lane;
        const uint32_t ov = p < n ? (n - p < A ? n - p : A) : 0u;
        const uint32_t mm = trim_window_mm(trim_window(w0.lo, w1.lo, lane), trim_window(w0.hi, w1.hi, lane), trim_window(w0.nn, w1.nn, lane), a_lo, a_hi, ov);
        const unsigned long long acc = __ballot(ov > 0 && trim_accept(R, mm, ov));
        if (acc) { end = beg + at + first_lane(acc); break; }
        if (n - at < 64u + R.min_overlap) break;             // every start of the next tile overlaps by less than M
        w0 = w1;
    }
    return end;
}

// rec[i], len[i] for i < n_rec, as k_fq_parse left them.  pe: records 2p and 2p + 1 are the mates of pair p; else every record is mate mate_se.
__global__ void __launch_bounds__(256) k_fq_trim(const uint8_t *__restrict__ raw, uint64_t n_raw, FqRec *__restrict__ rec, uint32_t *__restrict__ len, uint32_t n_rec,
                                                  uint32_t pe, uint32_t mate_se, TrimRule R, uint32_t *__restrict__ ctl /* [3]: longest trimmed read */,
                                                  unsigned long long *__restrict__ counts /* [16] */, uint32_t *__restrict__ spans /* [2 n_rec] or null */)
{
    __shared__ unsigned long long sh[2 * TRIM_N_COUNTS];
    if (threadIdx.x < 2 * TRIM_N_COUNTS) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t mate = pe ? (uint32_t)(wave & 1u) : mate_se;      // n_waves is even: a wave stays with one mate of the interleaved pairs
    uint64_t cnt[TRIM_N_COUNTS] = {};                    // wave-uniform
    uint32_t longest = 0;
    for (uint64_t i = wave; i < n_rec; i += n_waves) {
        const FqRec r = rec[i];
        const uint32_t L = r.len;
        // a record the parser refuses (empty, or its quality line is not L bytes): the call fails on the parser's word; nothing of it is read here
        if (L == 0 || (uint64_t)r.seq_off + L > n_raw || (uint64_t)r.qual_off + L > n_raw) {
            if (spans && lane == 0) { spans[2 * i] = 0; spans[2 * i + 1] = L; }
            longest = L > longest ? L : longest;
            continue;
        }
        const uint8_t *seq = raw + r.seq_off, *qual = raw + r.qual_off;
        uint32_t beg, end;
        trim_clip(R, L, &beg, &end);
        const uint32_t e1 = end;
        if (R.qual) end = wave_quality(R, qual, beg, end, lane);
        const uint32_t e2 = end;
        if (R.a_len[mate] && end > beg) end = wave_adapter(R, mate, seq, beg, end, lane);
        const uint32_t e3 = end;
        const bool floored = trim_floor(L, &beg, &end);
        trim_count(cnt, L, beg, end, e1, e2, e3, floored);
        const uint32_t out_len = end - beg;
        longest = out_len > longest ? out_len : longest;
        if (lane == 0) {
            rec[i].seq_off = r.seq_off + beg; rec[i].qual_off = r.qual_off + beg; rec[i].len = out_len;
            len[i] = out_len;
            if (spans) { spans[2 * i] = beg; spans[2 * i + 1] = end; }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < TRIM_N_COUNTS; ++k) if (cnt[k]) atomicAdd(&sh[mate * TRIM_N_COUNTS + k], (unsigned long long)cnt[k]);
        if (longest) atomicMax(ctl + 3, longest);
    }
    __syncthreads();
    if (threadIdx.x < 2 * TRIM_N_COUNTS && sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]);
}

// 64 columns of a read as a TrimPairWord, a lane a column: col = the column, c = its letter's code (4 outside the read), [vb, ve) = the span
__device__ __forceinline__ TrimPairWord pair_word(uint32_t c, uint32_t col, uint32_t vb, uint32_t ve)
{
    TrimPairWord w; w.lo = __ballot(c & 1u); w.hi = __ballot(c & 2u); w.nn = __ballot(c & 4u); w.va = __ballot(col >= vb && col < ve);
    return w;
}

// Records 2p and 2p + 1 are the mates of pair p, p < n_pairs, as k_fq_parse_mate left them.  A wave a pair: steps 1 and 2 for both mates,
// step 2p, step 3 for both, the floor.  spans: [4 n_pairs] (b1, e1, b2, e2) or null.
__global__ void __launch_bounds__(256) k_fq_trim_pair(const uint8_t *__restrict__ raw, uint64_t n_raw, FqRec *__restrict__ rec, uint32_t *__restrict__ len, uint32_t n_pairs,
                                                       TrimRule R, TrimPairRule P, uint32_t *__restrict__ ctl /* [3]: longest trimmed read */,
                                                       unsigned long long *__restrict__ counts /* [16] */, unsigned long long *__restrict__ pair_counts /* [8] */,
                                                       uint32_t *__restrict__ spans)
{
    constexpr uint32_t N_SH = 2 * TRIM_N_COUNTS + TRIM_PAIR_N_COUNTS;
    __shared__ unsigned long long sh[N_SH];
    __shared__ TrimPairWord planes[4][2][TRIM_PAIR_WORDS];          // a wave's own: mate 1's words, then R's (512 bytes a wave)
    if (threadIdx.x < N_SH) sh[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    // the wave's number through readfirstlane: the compiler then knows the pair, its spans and the counters to be the same in all lanes
    const uint32_t wave_in_block = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    TrimPairWord *m1 = planes[wave_in_block][0], *Rw = planes[wave_in_block][1];
    uint64_t cnt[2 * TRIM_N_COUNTS] = {}, pc[TRIM_PAIR_N_COUNTS] = {};          // wave-uniform
    uint32_t longest = 0;
    for (uint64_t p = wave; p < n_pairs; p += n_waves) {
        const FqRec r[2] = { rec[2 * p], rec[2 * p + 1] };
        const uint32_t L[2] = { r[0].len, r[1].len };
        // a record the parser refuses: the call fails on the parser's word; nothing of the pair is read here
        bool bad = false;
        for (uint32_t m = 0; m < 2; ++m) bad |= L[m] == 0 || (uint64_t)r[m].seq_off + L[m] > n_raw || (uint64_t)r[m].qual_off + L[m] > n_raw;
        if (bad) {
            if (spans && lane == 0) { spans[4 * p] = 0; spans[4 * p + 1] = L[0]; spans[4 * p + 2] = 0; spans[4 * p + 3] = L[1]; }
            longest = L[0] > longest ? L[0] : longest; longest = L[1] > longest ? L[1] : longest;
            continue;
        }
        const uint8_t *seq[2] = { raw + r[0].seq_off, raw + r[1].seq_off };
        uint32_t beg[2], end[2], e1[2], e2[2];
        for (uint32_t m = 0; m < 2; ++m) {
            trim_clip(R, L[m], &beg[m], &end[m]);
            e1[m] = end[m];
            if (R.qual) end[m] = __builtin_amdgcn_readfirstlane(wave_quality(R, raw + r[m].qual_off, beg[m], end[m], lane));
            e2[m] = end[m];
        }
        if (trim_pair_on(P)) {
            const bool skipped = L[0] > TRIM_PAIR_MAX_LEN || L[1] > TRIM_PAIR_MAX_LEN;
            const uint32_t first = skipped ? 0u : trim_pair_first(P, end[0], end[1]), n1 = trim_pair_words(end[0]);
            uint32_t I = 0;
            if (first) {
                // mate 1's words up to its span's end (the others are never read); all of R's, zero behind the read
                for (uint32_t t = 0; t < n1; ++t) {
                    const uint32_t col = 64u * t + lane;
                    const TrimPairWord w = pair_word(col < L[0] ? trim_code(seq[0][col]) : 4u, col, beg[0], end[0]);
                    if (lane == 0) m1[t] = w;
                }
                for (uint32_t t = 0; t < TRIM_PAIR_WORDS; ++t) {
                    const uint32_t col = 64u * t + lane;
                    TrimPairWord w = { 0, 0, 0, 0 };
                    if (64u * t < L[1]) w = pair_word(col < L[1] ? trim_code_rc(trim_code(seq[1][L[1] - 1u - col])) : 4u, col, L[1] - end[1], L[1] - beg[1]);
                    if (lane == 0) Rw[t] = w;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (uint32_t base = 0; base < first; base += 64) {
                    const uint32_t cand = base + lane;
                    uint32_t mm = 0, ov = 0;
                    if (cand < first) trim_pair_eval(m1, Rw, n1, L[1], first - cand, &mm, &ov);
                    const unsigned long long acc = __ballot(cand < first && trim_pair_accept(P, mm, ov));
                    if (acc) { I = first - (base + first_lane(acc)); break; }
                }
                __builtin_amdgcn_wave_barrier();             // the next pair's words are written behind this pair's reads
            }
            trim_pair_count(pc, I, end[0], end[1], skipped);
            if (I) { end[0] = end[0] < I ? end[0] : I; end[1] = end[1] < I ? end[1] : I; }
        }
        for (uint32_t m = 0; m < 2; ++m) {
            const uint32_t e2p = end[m];
            if (R.a_len[m] && end[m] > beg[m]) end[m] = wave_adapter(R, m, seq[m], beg[m], end[m], lane);
            const uint32_t e3 = end[m];
            const bool floored = trim_floor(L[m], &beg[m], &end[m]);
            trim_count_pair(cnt + TRIM_N_COUNTS * m, L[m], beg[m], end[m], e1[m], e2[m], e2p, e3, floored);
            const uint32_t out_len = end[m] - beg[m];
            longest = out_len > longest ? out_len : longest;
            if (lane == 0) {
                const uint64_t i = 2 * p + m;
                rec[i].seq_off = r[m].seq_off + beg[m]; rec[i].qual_off = r[m].qual_off + beg[m]; rec[i].len = out_len;
                len[i] = out_len;
                if (spans) { spans[2 * i] = beg[m]; spans[2 * i + 1] = end[m]; }
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < 2 * TRIM_N_COUNTS; ++k) if (cnt[k]) atomicAdd(&sh[k], (unsigned long long)cnt[k]);
#pragma unroll
        for (uint32_t k = 0; k < TRIM_PAIR_N_COUNTS; ++k) if (pc[k]) atomicAdd(&sh[2 * TRIM_N_COUNTS + k], (unsigned long long)pc[k]);
        if (longest) atomicMax(ctl + 3, longest);
    }
    __syncthreads();
    if (threadIdx.x < 2 * TRIM_N_COUNTS) { if (sh[threadIdx.x]) atomicAdd(&counts[threadIdx.x], sh[threadIdx.x]); }
    else if (threadIdx.x < N_SH && sh[threadIdx.x]) atomicAdd(&pair_counts[threadIdx.x - 2 * TRIM_N_COUNTS], sh[threadIdx.x]);
}

// behind k_fq_parse (both mates' launches for a pair), in front of the scan of len; ctl[3] = the longest trimmed read (ctl as launch_fq_ctl_init left it)
hipError_t launch_fq_trim(const uint8_t *raw, uint64_t n_raw, FqRec *rec, uint32_t *len, uint32_t n_rec, int pe, uint32_t mate, const TrimRule &rule,
                          uint32_t *ctl, unsigned long long *counts, uint32_t *spans, hipStream_t st)
{
    if (n_rec == 0) return hipSuccess;
    const uint64_t want = ((uint64_t)n_rec + 3) / 4;
    hipLaunchKernelGGL(k_fq_trim, dim3((uint32_t)(want < TRIM_BLOCKS ? want : TRIM_BLOCKS)), dim3(256), 0, st, raw, n_raw, rec, len, n_rec, pe ? 1u : 0u, mate & 1u, rule,
                       ctl, counts, spans);
    return hipGetLastError();
}

// in k_fq_trim's place for the interleaved mates of n_pairs pairs when the pair rule is on
hipError_t launch_fq_trim_pair(const uint8_t *raw, uint64_t n_raw, FqRec *rec, uint32_t *len, uint32_t n_pairs, const TrimRule &rule, const TrimPairRule &pair,
                               uint32_t *ctl, unsigned long long *counts, unsigned long long *pair_counts, uint32_t *spans, hipStream_t st)
{
    if (n_pairs == 0) return hipSuccess;
    const uint64_t want = ((uint64_t)n_pairs + 3) / 4;
    hipLaunchKernelGGL(k_fq_trim_pair, dim3((uint32_t)(want < TRIM_BLOCKS ? want : TRIM_BLOCKS)), dim3(256), 0, st, raw, n_raw, rec, len, n_pairs, rule, pair,
                       ctl, counts, pair_counts, spans);
    return hipGetLastError();
}

} // namespace salt
