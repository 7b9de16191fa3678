// salt_amd/csrc/salt_bgzf.hip -- text in device memory -> a contiguous run of BGZF blocks (`salt --bgzf`, salt_gpu_bgzf_deflate).
//
//   k_bgzf_deflate  one workgroup per BGZF_CUT bytes of text: the whole block (matches, Huffman codes, bit stream, CRC-32, container) in
//                   LDS, written into the block's fixed-stride slot; its size into sizes[] (salt_bgzf_block.h)
//   k_bgzf_scan     sizes -> byte offsets of the blocks in the output (one workgroup; 64-bit sums), offs[n_blocks] = all bytes
//   k_bgzf_pack     slots -> the output, blocks contiguous and in order
// Work is handed over at the kernel boundaries only.  The same text gives the same bytes on every run: nothing in a block depends on the
// order waves run in (the hash table takes the maximum position of a round, histograms and bit words are sums and ORs).
#include <hip/hip_runtime.h>
#include "salt_kernels.h"
#include "salt_bgzf_block.h"

namespace salt {

using namespace bgzf;
static_assert(BGZF_CUT == BGZF_CUT_BYTES && BGZF_SLOT == BGZF_SLOT_BYTES, "salt_kernels.h sizes the buffers");

__global__ __launch_bounds__(BGZF_THREADS) void k_bgzf_deflate(const uint8_t *text, uint64_t n, uint32_t *slots, uint32_t *sizes)
{
    __shared__ BlockLds s;
    const uint64_t at = (uint64_t)blockIdx.x * BGZF_CUT;
    const uint32_t len = n - at < BGZF_CUT ? (uint32_t)(n - at) : BGZF_CUT;
    deflate_block(s, text + at, len, slots + (size_t)blockIdx.x * (BGZF_SLOT / 4), sizes + blockIdx.x, threadIdx.x);
}

static const uint32_t SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void k_bgzf_scan(const uint32_t *sizes, uint32_t n_blocks, unsigned long long *offs)
{
    __shared__ unsigned long long part[SCAN_THREADS];
    const uint32_t per = (n_blocks + SCAN_THREADS - 1) / SCAN_THREADS;
    const uint32_t lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += sizes[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (uint32_t t = 0; t < SCAN_THREADS; ++t) { const unsigned long long v = part[t]; part[t] = run; run += v; }
        offs[n_blocks] = run;
    }
    __syncthreads();
    sum = part[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) { offs[i] = sum; sum += sizes[i]; }
}

static const uint32_t PACK_THREADS = 256;
__global__ __launch_bounds__(PACK_THREADS) void k_bgzf_pack(const uint32_t *slots, const uint32_t *sizes, const unsigned long long *offs, uint8_t *out)
{
    const uint32_t *src = slots + (size_t)blockIdx.x * (BGZF_SLOT / 4);
    const uint8_t *src8 = reinterpret_cast<const uint8_t *>(src);
    const uint32_t size = sizes[blockIdx.x];
    uint8_t *dst = out + offs[blockIdx.x];
    // bytes up to the output's next word boundary, whole output words (each from two slot words), the bytes left
    uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
    if (head > size) head = size;
    const uint32_t n_words = (size - head) / 4;
    if (threadIdx.x < head) dst[threadIdx.x] = src8[threadIdx.x];
    uint32_t *dw = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t w = threadIdx.x; w < n_words; w += PACK_THREADS) {
        const uint32_t j = head + 4 * w, sh = (j & 3) * 8;
        const uint32_t a = src[j >> 2];
        dw[w] = sh ? (a >> sh) | (src[(j >> 2) + 1] << (32 - sh)) : a;
    }
    const uint32_t done = head + 4 * n_words;
    if (done + threadIdx.x < size) dst[done + threadIdx.x] = src8[done + threadIdx.x];
}

hipError_t launch_bgzf_deflate(const uint8_t *text, uint64_t n, uint32_t *slots, uint32_t *sizes, unsigned long long *offs, uint8_t *out, hipStream_t st)
{
    const uint64_t n_blocks = bgzf_blocks(n);
    if (n_blocks == 0) return hipSuccess;
    if (n_blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    k_bgzf_deflate<<<(uint32_t)n_blocks, BGZF_THREADS, 0, st>>>(text, n, slots, sizes);
    k_bgzf_scan<<<1, SCAN_THREADS, 0, st>>>(sizes, (uint32_t)n_blocks, offs);
    k_bgzf_pack<<<(uint32_t)n_blocks, PACK_THREADS, 0, st>>>(slots, sizes, offs, out);
    return hipGetLastError();
}

} // namespace salt
