// salt_amd/csrc/salt_snp.hip -- allele counts at the index's SNP sites (salt --snp-counts).
//
// A site is a genome position whose mixRef mask lists two or more bases.  The site table holds one 16-byte record per 64 genome positions
// (SnpWin: which of them are sites, and how many sites lie in front of the window), so that "is g a site, and which one" is ONE request:
//     site(g) = rank + popc(bits & ((1 << (g & 63)) - 1))
// k_snp_count runs behind the kernels that finish a batch's result rows: a thread per record walks the row's CIGAR as the SAM / BAM
// writers lay it out and adds, for every site an M run covers, the read's base there to the site's row of counts[n_sites][4].
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_tally.h"

namespace salt {

// window w = positions [64 w, 64 w + 64): eight words of the 4-bit mixRef.  A position at or beyond ref_len is no site, whatever the
// words' padding holds; a word beyond the array is not read.
__global__ void __launch_bounds__(256) k_snp_bits(const uint32_t *__restrict__ ref, uint32_t ref_len, uint64_t n_win, SnpWin *__restrict__ tab, uint32_t *__restrict__ cnt)
{
    const uint64_t n_words = ((uint64_t)ref_len + 7) / 8;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_win; w += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long bits = 0;
        for (uint32_t k = 0; k < 8; ++k) {
            const uint64_t wi = w * 8 + k;
            if (wi >= n_words) break;
            const uint32_t x = ref[wi];
            for (uint32_t j = 0; j < 8; ++j) {
                const uint64_t g = wi * 8 + j;
                const uint32_t m = (x >> (4 * j)) & 15u;
                if (g < ref_len && (m & (m - 1u)) != 0) bits |= 1ull << (8 * k + j);      // two or more bits set
            }
        }
        SnpWin r; r.bits = bits; r.rank = 0; r.pad = 0;
        tab[w] = r;
        cnt[w] = (uint32_t)__popcll(bits);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[n_win] = 0;           // the scan's last entry: all sites
}

__global__ void __launch_bounds__(256) k_snp_rank(const uint32_t *__restrict__ rank, uint64_t n_win, SnpWin *__restrict__ tab)
{
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_win; w += (uint64_t)gridDim.x * blockDim.x) tab[w].rank = rank[w];
}

// pos[site] = genome position of the site, ascending
__global__ void __launch_bounds__(256) k_snp_pos(const SnpWin *__restrict__ tab, uint64_t n_win, uint32_t *__restrict__ pos)
{
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_win; w += (uint64_t)gridDim.x * blockDim.x) {
        const SnpWin r = tab[w];
        uint32_t k = r.rank;
        for (unsigned long long b = r.bits; b; b &= b - 1) pos[k++] = (uint32_t)(w * 64 + (uint64_t)(__ffsll(b) - 1));
    }
}

// One thread per record.  Loads: the row's first 24 bytes (a 16-byte and an 8-byte request), its CIGAR words one at a time (most rows have
// one), per M run the window records it touches (one 16-byte request each) and, per site found, one byte of the read's codes and one
// atomic.  Nothing is read beyond the read's own codes or beyond the table's n_win records: a row the align kernels got wrong cannot
// make this kernel fault.
__global__ void __launch_bounds__(256) k_snp_count(SnpCount c)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n_rec; i += (uint64_t)gridDim.x * blockDim.x) {
        const salt_result_t *q = c.res + i;
        const TallyRow r = tally_row(q, c.pe, c.min_mapq);
        if (r.fate != TALLY_COUNTED) continue;
        const bool rev = r.rev;
        const uint32_t o0 = c.offs[i], L = c.offs[i + 1] - o0;
        const uint8_t *sq = c.seqs + o0;
        tally_m_runs(q, r, [&](uint64_t g, uint32_t s, uint32_t len) {
            const uint64_t g_end = g + len;                                        // the run covers [g, g_end), read bases s + (x - g)
            for (uint64_t w = g >> 6; w < c.n_win && (w << 6) < g_end; ++w) {
                const SnpWin t = c.tab[w];
                unsigned long long bits = t.bits;
                if ((w << 6) < g) bits &= ~0ull << (g & 63u);
                if (g_end < (w << 6) + 64) bits &= ~(~0ull << (g_end & 63u));
                for (; bits; bits &= bits - 1) {
                    const uint32_t b = (uint32_t)__ffsll(bits) - 1u;
                    const uint64_t j = (uint64_t)s + ((w << 6) + b - g);           // index in SEQ as printed
                    if (j >= L) continue;
                    uint32_t code = sq[rev ? L - 1u - (uint32_t)j : (uint32_t)j];
                    if (code > 3u) continue;                                       // N counts nowhere
                    if (rev) code = 3u - code;
                    const uint64_t site = (uint64_t)t.rank + (uint32_t)__popcll(t.bits & ((1ull << b) - 1ull));
                    atomicAdd(c.counts + site * 4 + code, c.delta);
                }
            }
        });
    }
}

size_t snp_scan_bytes(uint64_t n_win)
{
    size_t b = 0;
    uint32_t *p = nullptr;
    (void)rocprim::exclusive_scan(nullptr, b, p, p, 0u, (size_t)n_win + 1, rocprim::plus<uint32_t>(), nullptr);
    return b;
}
// tab[0 .. n_win) from the mixRef; cnt: n_win + 1 words of scratch, cnt[n_win] = the number of sites afterwards
hipError_t launch_snp_table(const uint32_t *ref, uint32_t ref_len, uint64_t n_win, SnpWin *tab, uint32_t *cnt, void *tmp, size_t tmp_bytes, hipStream_t st)
{
    hipLaunchKernelGGL(k_snp_bits, dim3(tally_grid(n_win)), dim3(256), 0, st, ref, ref_len, n_win, tab, cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rocprim::exclusive_scan(tmp, tmp_bytes, cnt, cnt, 0u, (size_t)n_win + 1, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_snp_rank, dim3(tally_grid(n_win)), dim3(256), 0, st, cnt, n_win, tab);
    return hipGetLastError();
}
hipError_t launch_snp_pos(const SnpWin *tab, uint64_t n_win, uint32_t *pos, hipStream_t st)
{
    hipLaunchKernelGGL(k_snp_pos, dim3(tally_grid(n_win)), dim3(256), 0, st, tab, n_win, pos);
    return hipGetLastError();
}
hipError_t launch_snp_count(const SnpCount &c, hipStream_t st)
{
    if (c.n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(k_snp_count, dim3(tally_grid(c.n_rec)), dim3(256), 0, st, c);
    return hipGetLastError();
}

} // namespace salt
