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
        if (R.qual) {
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
            end = cut;
        }
        const uint32_t e2 = end, A = R.a_len[mate];
        if (A && end > beg) {
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
        }
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

} // namespace salt
