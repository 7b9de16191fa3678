// salt_amd/csrc/salt_vcf.hip -- SNP sites from a VCF, parsed on the device (`salt-idx --gpu --vcf`; the rule is DESIGN.md 2.2, the ABI
// salt_gpu_vcf_* in include/salt_gpu.h).
//   k_fq_count / k_fq_lines   (salt_text.hip) newline scan of a chunk -> start offset of every line
//   k_vcf_parse               one thread per line: vcf_line (salt_vcf_line.h, shared with the host twin) reads as far as ALT, or FILTER; a kept
//                             line ORs its allele mask into the position's byte of the genome-wide mask array (32-bit atomicOr on the
//                             word that holds it), so duplicates, unsorted input and chunk cuts need no sort.  Counters are summed per
//                             workgroup before one atomic each; malformed and unknown-contig lines go to an atomicMin on the line number.
//   k_vcf_advance             lines seen so far += this chunk's, on the device: no chunk waits for the host to count
//   k_vcf_count / k_vcf_emit  non-zero mask bytes per 1024-position tile, an exclusive scan, then (position in its contig, mask, reference
//                             code) of every site in genome order; k_vcf_bounds reads every contig's first site index off the scan.
// Chunks go through two page-locked buffers: the copy stream fills device buffer b while the run stream parses buffer 1 - b.
#include <hip/hip_runtime.h>
#include <string.h>
#include <string>
#include <vector>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include "salt_kernels.h"
#include "salt_vcf_line.h"

namespace salt {

int set_last_error(int code, const std::string &msg);        // salt_gpu.hip: what salt_gpu_last_error() returns

static const uint32_t VT = 1024;                              // positions per compaction tile: 256 threads x one word of 4 mask bytes
enum { VC_BAD = 0, VC_UNK = 1, VC_LINE = 2, VC_CNT = 3, VC_N = 10 };      // ctl words; VC_CNT + (status - 1) for kept .. filtered

__global__ void __launch_bounds__(256) k_vcf_parse(const uint8_t *__restrict__ raw, uint32_t n, const uint32_t *__restrict__ n_newlines,
                                                   const uint32_t *__restrict__ line_start, VcfTable T, uint32_t *__restrict__ mask_words,
                                                   unsigned long long *__restrict__ ctl)
{
    const uint32_t n_nl = *n_newlines;
    const uint32_t n_lines = n_nl + (line_start[n_nl] < n ? 1u : 0u);          // a last line without '\n' counts
    const unsigned long long base = ctl[VC_LINE];
    uint32_t cnt[6] = { 0, 0, 0, 0, 0, 0 };
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, s = (uint64_t)gridDim.x * blockDim.x; i < n_lines; i += s) {
        const uint64_t b = line_start[i], e = i < n_nl ? (uint64_t)line_start[i + 1] - 1 : (uint64_t)n;
        uint64_t g = 0; uint32_t m = 0;
        const int st = vcf_line(raw, b, e, T, &g, &m);
        if (st == VCF_KEPT) atomicOr(mask_words + (g >> 2), m << (8 * (uint32_t)(g & 3)));
        else if (st == VCF_MALFORMED) atomicMin(ctl + VC_BAD, base + i + 1);
        else if (st == VCF_UNKNOWN) atomicMin(ctl + VC_UNK, base + i + 1);
#pragma unroll
        for (int k = 0; k < 6; ++k) cnt[k] += st == k + 1 ? 1u : 0u;
    }
    __shared__ uint32_t part[4][6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        uint32_t c = cnt[k];
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const uint32_t c = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (c) atomicAdd(ctl + VC_CNT + threadIdx.x, (unsigned long long)c);
    }
}

__global__ void k_vcf_advance(uint32_t n, const uint32_t *__restrict__ n_newlines, const uint32_t *__restrict__ line_start, unsigned long long *__restrict__ ctl)
{
    const uint32_t n_nl = *n_newlines;
    ctl[VC_LINE] += n_nl + (line_start[n_nl] < n ? 1u : 0u);
}

__device__ __forceinline__ uint32_t nz_bytes(uint32_t w) { return (w & 0xFFu ? 1u : 0u) + (w & 0xFF00u ? 1u : 0u) + (w & 0xFF0000u ? 1u : 0u) + (w & 0xFF000000u ? 1u : 0u); }

// mask_words holds n_tiles * 256 words (the bytes behind the genome's end are zero)
__global__ void __launch_bounds__(256) k_vcf_count(const uint32_t *__restrict__ mask_words, uint64_t n_tiles, uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t part[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint32_t c = nz_bytes(mask_words[t * 256 + threadIdx.x]);
        for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[t] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

// tile_off: exclusive scan of tile_cnt.  start[0 .. n_contigs]: contig offsets; the contig of p is the last one with start <= p (empty contigs hold nothing)
__global__ void __launch_bounds__(256) k_vcf_emit(const uint32_t *__restrict__ mask_words, const uint8_t *__restrict__ genome, uint64_t n_tiles,
                                                  const uint32_t *__restrict__ tile_off, const uint64_t *__restrict__ start, uint32_t n_contigs,
                                                  uint32_t *__restrict__ pos, uint8_t *__restrict__ al, uint8_t *__restrict__ ref)
{
    __shared__ uint32_t wave_sum[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t w = mask_words[t * 256 + threadIdx.x];
        const uint32_t c = nz_bytes(w);
        uint32_t incl = c;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if ((threadIdx.x & 63) >= (uint32_t)o) incl += v; }
        if ((threadIdx.x & 63) == 63) wave_sum[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t k = tile_off[t] + incl - c;
        for (uint32_t v = 0; v < (threadIdx.x >> 6); ++v) k += wave_sum[v];
        if (c) {
            const uint64_t p0 = t * VT + threadIdx.x * 4;
            uint32_t lo = 0, hi = n_contigs;                  // the contig of p0: last start <= p0
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (start[mid] <= p0) lo = mid; else hi = mid; }
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t m = (w >> (8 * q)) & 0xFFu;
                if (!m) continue;
                const uint64_t p = p0 + q;
                while (lo + 1 < n_contigs && start[lo + 1] <= p) ++lo;      // a word may span a contig's end
                pos[k] = (uint32_t)(p - start[lo]); al[k] = (uint8_t)m; ref[k] = (uint8_t)vcf_base(genome[p]);
                ++k;
            }
        }
        __syncthreads();
    }
}

// first[c] = sites in front of contig c, c = 0 .. n_contigs (the last: all sites): the scan at the contig's tile plus the tile's bytes in front of it
__global__ void k_vcf_bounds(const uint8_t *__restrict__ mask, const uint32_t *__restrict__ tile_off, const uint64_t *__restrict__ start, uint32_t n_contigs,
                             uint32_t *__restrict__ first)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_contigs) return;
    const uint64_t s = start[c], t = s / VT;
    uint32_t k = tile_off[t];
    for (uint64_t p = t * VT; p < s; ++p) k += mask[p] ? 1u : 0u;
    first[c] = k;
}

} // namespace salt

using namespace salt;

struct salt_gpu_vcf {
    int device = 0;
    uint32_t n_contigs = 0;
    uint64_t total = 0, n_tiles = 0;
    std::vector<uint64_t> start;
    uint8_t *d_genome = nullptr, *d_mask = nullptr, *d_names = nullptr;      // the genome: the contigs' letters, concatenated
    const uint8_t **d_seq = nullptr;
    uint64_t *d_start = nullptr;
    uint32_t *d_key_off = nullptr, *d_slots = nullptr;
    int32_t *d_key_contig = nullptr;
    unsigned long long *d_ctl = nullptr;
    VcfTable tab;
    // chunks
    uint64_t chunk_bytes = 0, cap = 0;
    uint8_t *h_buf[2] = { nullptr, nullptr }, *d_buf[2] = { nullptr, nullptr };
    uint32_t *d_tile = nullptr, *d_lines = nullptr;
    void *d_tmp = nullptr; size_t tmp_bytes = 0;
    hipStream_t s_copy = nullptr, s_run = nullptr;
    hipEvent_t ev_copied[2] = { nullptr, nullptr }, ev_parsed[2] = { nullptr, nullptr };
    bool used[2] = { false, false };
    int turn = 0;
    // result
    bool finished = false;
    uint32_t *d_pos = nullptr; uint8_t *d_al = nullptr, *d_ref = nullptr;
    std::vector<uint32_t> first;
};

#define VCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return set_last_error(SALT_E_HIP, std::string("VCF: ") + #x + ": " + hipGetErrorString(e_)); } while (0)

static int vcf_alloc(void **p, uint64_t bytes, const char *what)
{
    if (hipMalloc(p, bytes ? bytes : 4) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return set_last_error(SALT_E_NOMEM, std::string("VCF: no device memory for ") + what + " (" + std::to_string(bytes) + " bytes)");
    }
    return SALT_OK;
}

static void vcf_free_chunks(salt_gpu_vcf *h)
{
    for (int b = 0; b < 2; ++b) { if (h->h_buf[b]) (void)hipHostFree(h->h_buf[b]); if (h->d_buf[b]) (void)hipFree(h->d_buf[b]); h->h_buf[b] = h->d_buf[b] = nullptr; }
    if (h->d_tile) (void)hipFree(h->d_tile);
    if (h->d_lines) (void)hipFree(h->d_lines);
    if (h->d_tmp) (void)hipFree(h->d_tmp);
    h->d_tile = h->d_lines = nullptr; h->d_tmp = nullptr; h->cap = 0;
}

// buffers for chunks of up to `bytes`: nothing is in flight when this is called
static int vcf_chunk_buffers(salt_gpu_vcf *h, uint64_t bytes)
{
    vcf_free_chunks(h);
    const uint64_t tiles = (bytes + FQ_TILE - 1) / FQ_TILE;
    for (int b = 0; b < 2; ++b) {
        if (hipHostMalloc((void **)&h->h_buf[b], bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); h->h_buf[b] = nullptr;
            return set_last_error(SALT_E_NOMEM, "VCF: no page-locked memory for a chunk of " + std::to_string(bytes) + " bytes");
        }
        if (int rc = vcf_alloc((void **)&h->d_buf[b], bytes, "a chunk of text")) return rc;
    }
    if (int rc = vcf_alloc((void **)&h->d_tile, (tiles + 1) * 4, "the newline counts")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_lines, (bytes + 2) * 4, "the line starts")) return rc;        // every byte may be a newline
    h->tmp_bytes = text_scan_bytes(tiles + 1);
    if (int rc = vcf_alloc(&h->d_tmp, h->tmp_bytes, "the scan")) return rc;
    h->cap = bytes;
    return SALT_OK;
}

extern "C" void salt_gpu_vcf_close(salt_gpu_vcf_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    vcf_free_chunks(h);
    void *ps[] = { h->d_genome, (void *)h->d_seq, h->d_mask, h->d_names, h->d_start, h->d_key_off, h->d_slots, h->d_key_contig, h->d_ctl, h->d_pos, h->d_al, h->d_ref };
    for (void *p : ps) if (p) (void)hipFree(p);
    for (int b = 0; b < 2; ++b) { if (h->ev_copied[b]) (void)hipEventDestroy(h->ev_copied[b]); if (h->ev_parsed[b]) (void)hipEventDestroy(h->ev_parsed[b]); }
    if (h->s_copy) (void)hipStreamDestroy(h->s_copy);
    if (h->s_run) (void)hipStreamDestroy(h->s_run);
    delete h;
}

static int vcf_open(salt_gpu_vcf *h, int32_t n_contigs, const char *const *seq, const uint64_t *len, int32_t n_keys, const char *const *keys,
                    const int32_t *key_contig, const salt_gpu_vcf_opt_t *opt)
{
    VCHK(hipSetDevice(h->device));
    h->n_contigs = (uint32_t)n_contigs;
    h->start.assign((size_t)n_contigs + 1, 0);
    for (int32_t i = 0; i < n_contigs; ++i) h->start[(size_t)i + 1] = h->start[(size_t)i] + len[i];
    h->total = h->start[(size_t)n_contigs];
    if (h->total == 0 || h->total >= 0xFFFFFFE0ull) return set_last_error(SALT_E_INVAL, "VCF: genome empty or too long for the 32-bit index");
    h->n_tiles = (h->total + VT - 1) / VT;
    // the key table: at most half full
    std::string names; std::vector<uint32_t> key_off((size_t)n_keys + 1, 0);
    for (int32_t k = 0; k < n_keys; ++k) {
        if (!keys[k] || key_contig[k] < 0 || key_contig[k] >= n_contigs) return set_last_error(SALT_E_INVAL, "VCF: key " + std::to_string(k) + " has no name or names no contig");
        names += keys[k]; key_off[(size_t)k + 1] = (uint32_t)names.size();
    }
    uint32_t n_slots = 16;
    while (n_slots < 2u * (uint32_t)n_keys + 2u) n_slots <<= 1;
    std::vector<uint32_t> slots(n_slots, 0);
    for (int32_t k = 0; k < n_keys; ++k) {
        uint32_t s = vcf_hash((const uint8_t *)names.data() + key_off[(size_t)k], key_off[(size_t)k + 1] - key_off[(size_t)k]) & (n_slots - 1);
        while (slots[s]) s = (s + 1) & (n_slots - 1);
        slots[s] = (uint32_t)k + 1;
    }
    if (int rc = vcf_alloc((void **)&h->d_genome, h->total, "the genome")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_seq, (size_t)n_contigs * sizeof(void *), "the contig table")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_mask, h->n_tiles * VT, "the mask array")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_names, names.size(), "the contig names")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_start, ((size_t)n_contigs + 1) * 8, "the contig table")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_key_off, ((size_t)n_keys + 1) * 4, "the contig names")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_key_contig, (size_t)n_keys * 4, "the contig names")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_slots, (size_t)n_slots * 4, "the contig names")) return rc;
    if (int rc = vcf_alloc((void **)&h->d_ctl, VC_N * 8, "the counters")) return rc;
    VCHK(hipStreamCreateWithFlags(&h->s_copy, hipStreamNonBlocking));
    VCHK(hipStreamCreateWithFlags(&h->s_run, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) { VCHK(hipEventCreateWithFlags(&h->ev_copied[b], hipEventDisableTiming)); VCHK(hipEventCreateWithFlags(&h->ev_parsed[b], hipEventDisableTiming)); }
    for (int32_t i = 0; i < n_contigs; ++i) if (len[i]) {
        if (!seq[i]) return set_last_error(SALT_E_INVAL, "VCF: contig " + std::to_string(i) + " without bases");
        VCHK(hipMemcpy(h->d_genome + h->start[(size_t)i], seq[i], len[i], hipMemcpyHostToDevice));
    }
    if (!names.empty()) VCHK(hipMemcpy(h->d_names, names.data(), names.size(), hipMemcpyHostToDevice));
    VCHK(hipMemcpy(h->d_start, h->start.data(), h->start.size() * 8, hipMemcpyHostToDevice));
    VCHK(hipMemcpy(h->d_key_off, key_off.data(), key_off.size() * 4, hipMemcpyHostToDevice));
    if (n_keys) VCHK(hipMemcpy(h->d_key_contig, key_contig, (size_t)n_keys * 4, hipMemcpyHostToDevice));
    VCHK(hipMemcpy(h->d_slots, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
    unsigned long long ctl[VC_N] = { ~0ull, ~0ull, 0, 0, 0, 0, 0, 0, 0, 0 };
    VCHK(hipMemcpy(h->d_ctl, ctl, sizeof ctl, hipMemcpyHostToDevice));
    VCHK(hipMemsetAsync(h->d_mask, 0, h->n_tiles * VT, h->s_run));
    VCHK(hipStreamSynchronize(h->s_run));
    std::vector<const uint8_t *> sp((size_t)n_contigs);
    for (int32_t i = 0; i < n_contigs; ++i) sp[(size_t)i] = h->d_genome + h->start[(size_t)i];
    VCHK(hipMemcpy(h->d_seq, sp.data(), sp.size() * sizeof(void *), hipMemcpyHostToDevice));
    h->tab.names = h->d_names; h->tab.key_off = h->d_key_off; h->tab.key_contig = h->d_key_contig; h->tab.slots = h->d_slots;
    h->tab.slot_mask = n_slots - 1; h->tab.pass_only = opt && opt->pass_only ? 1u : 0u; h->tab.start = h->d_start; h->tab.seq = h->d_seq;
    h->chunk_bytes = opt && opt->chunk_bytes ? opt->chunk_bytes : (16ull << 20);
    if (h->chunk_bytes > (1ull << 30)) h->chunk_bytes = 1ull << 30;
    return vcf_chunk_buffers(h, h->chunk_bytes);
}

extern "C" int salt_gpu_vcf_open(int device, int32_t n_contigs, const char *const *seq, const uint64_t *len, int32_t n_keys, const char *const *keys,
                                 const int32_t *key_contig, const salt_gpu_vcf_opt_t *opt, salt_gpu_vcf_t **out)
{
    if (!out || n_contigs <= 0 || !seq || !len || n_keys < 0 || (n_keys > 0 && (!keys || !key_contig))) return set_last_error(SALT_E_INVAL, "VCF: bad argument");
    salt_gpu_vcf *h = new salt_gpu_vcf;
    h->device = device;
    const int rc = vcf_open(h, n_contigs, seq, len, n_keys, keys, key_contig, opt);
    if (rc != SALT_OK) { const std::string m = salt_gpu_last_error(); salt_gpu_vcf_close(h); *out = nullptr; return set_last_error(rc, m); }
    *out = h;
    return SALT_OK;
}

// one chunk of whole lines, 0 < n < 2^31
static int vcf_submit(salt_gpu_vcf *h, const char *p, uint64_t n)
{
    if (n > h->cap) {                                          // a line longer than the chunk: drain, then larger buffers
        VCHK(hipStreamSynchronize(h->s_copy)); VCHK(hipStreamSynchronize(h->s_run));
        h->used[0] = h->used[1] = false;
        if (int rc = vcf_chunk_buffers(h, n + n / 4)) return rc;
    }
    const int b = h->turn;
    if (h->used[b]) VCHK(hipEventSynchronize(h->ev_copied[b]));                 // the page-locked buffer has left for the device
    memcpy(h->h_buf[b], p, n);
    if (h->used[b]) VCHK(hipStreamWaitEvent(h->s_copy, h->ev_parsed[b], 0));    // the device buffer's lines are parsed
    VCHK(hipMemcpyAsync(h->d_buf[b], h->h_buf[b], n, hipMemcpyHostToDevice, h->s_copy));
    VCHK(hipEventRecord(h->ev_copied[b], h->s_copy));
    VCHK(hipStreamWaitEvent(h->s_run, h->ev_copied[b], 0));
    const uint64_t tiles = (n + FQ_TILE - 1) / FQ_TILE;
    VCHK(launch_fq_count(h->d_buf[b], n, h->d_tile, h->d_tmp, h->tmp_bytes, h->s_run));
    VCHK(launch_fq_lines(h->d_buf[b], n, h->d_tile, h->d_lines, h->s_run));
    uint64_t blocks = (n / 64 + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks == 0) blocks = 1;
    hipLaunchKernelGGL(k_vcf_parse, dim3((uint32_t)blocks), dim3(256), 0, h->s_run, h->d_buf[b], (uint32_t)n, h->d_tile + tiles, h->d_lines, h->tab,
                       (uint32_t *)h->d_mask, h->d_ctl);
    hipLaunchKernelGGL(k_vcf_advance, dim3(1), dim3(1), 0, h->s_run, (uint32_t)n, h->d_tile + tiles, h->d_lines, h->d_ctl);
    VCHK(hipGetLastError());
    VCHK(hipEventRecord(h->ev_parsed[b], h->s_run));
    h->used[b] = true; h->turn ^= 1;
    return SALT_OK;
}

extern "C" int salt_gpu_vcf_add(salt_gpu_vcf_t *h, const char *text, uint64_t n)
{
    if (!h || (n && !text)) return set_last_error(SALT_E_INVAL, "VCF: bad argument");
    if (h->finished) return set_last_error(SALT_E_INVAL, "VCF: add after finish");
    VCHK(hipSetDevice(h->device));
    uint64_t off = 0;
    while (off < n) {
        uint64_t len = n - off < h->chunk_bytes ? n - off : h->chunk_bytes;
        if (off + len < n) {                                   // cut behind the last newline; a line longer than the chunk goes whole
            const void *q = memrchr(text + off, '\n', len);
            if (q) len = (uint64_t)((const char *)q - (text + off)) + 1;
            else { q = memchr(text + off + len, '\n', n - off - len); len = q ? (uint64_t)((const char *)q - (text + off)) + 1 : n - off; }
        }
        if (len >= (1ull << 31)) return set_last_error(SALT_E_INVAL, "VCF: a line of 2 GiB or more");
        if (int rc = vcf_submit(h, text + off, len)) return rc;
        off += len;
    }
    return SALT_OK;
}

extern "C" int salt_gpu_vcf_finish(salt_gpu_vcf_t *h, salt_vcf_counters_t *counters, uint32_t *n_per_contig)
{
    if (!h || !counters) return set_last_error(SALT_E_INVAL, "VCF: bad argument");
    VCHK(hipSetDevice(h->device));
    if (!h->finished) {
        VCHK(hipStreamSynchronize(h->s_copy)); VCHK(hipStreamSynchronize(h->s_run));
        unsigned long long ctl[VC_N];
        VCHK(hipMemcpy(ctl, h->d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl[VC_BAD] != ~0ull)
            return set_last_error(SALT_E_DATA, "VCF line " + std::to_string(ctl[VC_BAD]) + " is malformed (fewer than 5 fields, or POS is not 1 to 10 digits)");
        vcf_free_chunks(h);
        uint32_t *d_tile = nullptr, *d_first = nullptr; void *d_tmp = nullptr;
        auto done = [&](int rc) { if (d_tile) (void)hipFree(d_tile); if (d_first) (void)hipFree(d_first); if (d_tmp) (void)hipFree(d_tmp); return rc; };
#define VDONE(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return done(set_last_error(SALT_E_HIP, std::string("VCF: ") + #x + ": " + hipGetErrorString(e_))); } while (0)
        if (int rc = vcf_alloc((void **)&d_tile, (h->n_tiles + 1) * 4, "the tile counts")) return done(rc);
        if (int rc = vcf_alloc((void **)&d_first, ((size_t)h->n_contigs + 1) * 4, "the contig bounds")) return done(rc);
        size_t tmp_bytes = 0;
        VDONE(rocprim::exclusive_scan(nullptr, tmp_bytes, d_tile, d_tile, 0u, (size_t)h->n_tiles + 1, rocprim::plus<uint32_t>(), h->s_run));
        if (int rc = vcf_alloc(&d_tmp, tmp_bytes, "the scan")) return done(rc);
        VDONE(hipMemsetAsync(d_tile + h->n_tiles, 0, 4, h->s_run));
        const uint32_t blocks = (uint32_t)(h->n_tiles < 65536 ? h->n_tiles : 65536);
        hipLaunchKernelGGL(k_vcf_count, dim3(blocks), dim3(256), 0, h->s_run, (const uint32_t *)h->d_mask, h->n_tiles, d_tile);
        VDONE(rocprim::exclusive_scan(d_tmp, tmp_bytes, d_tile, d_tile, 0u, (size_t)h->n_tiles + 1, rocprim::plus<uint32_t>(), h->s_run));
        uint32_t n_sites = 0;
        VDONE(hipMemcpyAsync(&n_sites, d_tile + h->n_tiles, 4, hipMemcpyDeviceToHost, h->s_run));
        VDONE(hipStreamSynchronize(h->s_run));
        if (int rc = vcf_alloc((void **)&h->d_pos, (uint64_t)n_sites * 4, "the sites")) return done(rc);
        if (int rc = vcf_alloc((void **)&h->d_al, n_sites, "the sites")) return done(rc);
        if (int rc = vcf_alloc((void **)&h->d_ref, n_sites, "the sites")) return done(rc);
        if (n_sites) hipLaunchKernelGGL(k_vcf_emit, dim3(blocks), dim3(256), 0, h->s_run, (const uint32_t *)h->d_mask, h->d_genome, h->n_tiles, d_tile, h->d_start, h->n_contigs,
                                        h->d_pos, h->d_al, h->d_ref);
        hipLaunchKernelGGL(k_vcf_bounds, dim3((h->n_contigs + 1 + 255) / 256), dim3(256), 0, h->s_run, h->d_mask, d_tile, h->d_start, h->n_contigs, d_first);
        VDONE(hipGetLastError());
        h->first.assign((size_t)h->n_contigs + 1, 0);
        VDONE(hipMemcpyAsync(h->first.data(), d_first, h->first.size() * 4, hipMemcpyDeviceToHost, h->s_run));
        VDONE(hipStreamSynchronize(h->s_run));
#undef VDONE
        done(0);
        h->finished = true;
    }
    unsigned long long ctl[VC_N];
    VCHK(hipMemcpy(ctl, h->d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
    counters->kept = ctl[VC_CNT + VCF_KEPT - 1]; counters->unknown_contig = ctl[VC_CNT + VCF_UNKNOWN - 1]; counters->out_of_range = ctl[VC_CNT + VCF_RANGE - 1];
    counters->not_snv = ctl[VC_CNT + VCF_NOT_SNV - 1]; counters->ref_mismatch = ctl[VC_CNT + VCF_REF - 1]; counters->filtered = ctl[VC_CNT + VCF_FILTERED - 1];
    counters->lines = counters->kept + counters->unknown_contig + counters->out_of_range + counters->not_snv + counters->ref_mismatch + counters->filtered;
    counters->sites = h->first[h->n_contigs];
    counters->first_unknown_line = ctl[VC_UNK] == ~0ull ? 0 : ctl[VC_UNK];
    if (n_per_contig) for (uint32_t c = 0; c < h->n_contigs; ++c) n_per_contig[c] = h->first[(size_t)c + 1] - h->first[c];
    return SALT_OK;
}

extern "C" int salt_gpu_vcf_fetch(salt_gpu_vcf_t *h, int32_t contig, uint32_t *pos, uint8_t *alleles, uint8_t *ref)
{
    if (!h || !h->finished) return set_last_error(SALT_E_INVAL, "VCF: fetch before finish");
    if (contig < 0 || (uint32_t)contig >= h->n_contigs) return set_last_error(SALT_E_INVAL, "VCF: contig " + std::to_string(contig) + " outside 0 .. " + std::to_string(h->n_contigs));
    VCHK(hipSetDevice(h->device));
    const uint64_t a = h->first[(size_t)contig], n = h->first[(size_t)contig + 1] - a;
    if (n == 0) return SALT_OK;
    if (!pos || !alleles || !ref) return set_last_error(SALT_E_INVAL, "VCF: bad argument");
    VCHK(hipMemcpy(pos, h->d_pos + a, n * 4, hipMemcpyDeviceToHost));
    VCHK(hipMemcpy(alleles, h->d_al + a, n, hipMemcpyDeviceToHost));
    VCHK(hipMemcpy(ref, h->d_ref + a, n, hipMemcpyDeviceToHost));
    return SALT_OK;
}
