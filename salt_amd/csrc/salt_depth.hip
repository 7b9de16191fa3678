// salt_amd/csrc/salt_depth.hip -- coverage: per-base and windowed depth (salt --depth; the definition is in include/salt_gpu.h).
//
// Counting: diff is uint32[ref_len + 1].  k_depth_mark runs behind the kernels that finish a batch's result rows: a thread per record walks
// the row's CIGAR and, for every M run [g, end) cut at ref_len, adds delta at g and takes it at end -- two atomics a read for most reads.
// Finishing (DepthText): the genome goes by in tiles of tile_positions.  A tile of diff is scanned into a tile-sized scratch (rocprim) and
// the carry of the tiles in front is added; diff itself is only read.  Per base: run starts are flagged (diff != 0, or a contig's first
// position), compacted to their positions (rocprim::select), and every pair of neighbouring starts is one line -- the run that is still
// open at the tile's end is carried (start, depth) into the next tile, so a run over a tile edge is ONE line.  Lines are measured, the
// lengths scanned, the lines written (the k_sam_len / k_sam_write pattern) and copied out; lines that outgrow the text buffer leave in
// several pieces.  Windows: every tile adds its depths into one uint64 per window (a window over a tile edge gets both parts); the lines
// are written once the last tile is in, a tile's worth of windows at a time.  With bgzf the pieces pass k_bgzf_deflate first.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/functional.hpp>
#include <algorithm>
#include <string>
#include <vector>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_tally.h"

namespace salt {

// One thread per record.  Loads: the row's first 24 bytes (a 16-byte and an 8-byte request) and its CIGAR words one at a time (most rows
// have one); per M run two atomics.  An index is at most ref_len and no more than SALT_MAX_CIGAR_OPS words are read: a row the align
// kernels got wrong cannot make this kernel fault.
__global__ void __launch_bounds__(256) k_depth_mark(DepthMark c)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n_rec; i += (uint64_t)gridDim.x * blockDim.x) {
        const salt_result_t *q = c.res + i;
        const TallyRow r = tally_row(q, 0, c.min_mapq);                            // (a leading soft clip moves in the read only)
        if (r.fate != TALLY_COUNTED) continue;
        tally_m_runs(q, r, [&](uint64_t g, uint32_t, uint32_t len) { tally_diff_mark(c.diff, c.ref_len, g, len, c.delta); });      // cut at the genome's end
    }
}

__global__ void __launch_bounds__(256) k_depth_add(uint32_t *__restrict__ diff, const uint32_t *__restrict__ in, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) if (in[i]) atomicAdd(diff + i, in[i]);
}

hipError_t launch_depth_mark(const DepthMark &c, hipStream_t st)
{
    if (c.n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(k_depth_mark, dim3(tally_grid(c.n_rec)), dim3(256), 0, st, c);
    return hipGetLastError();
}
hipError_t launch_depth_add(uint32_t *diff, const uint32_t *in, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_depth_add, dim3(tally_grid(n)), dim3(256), 0, st, diff, in, n);
    return hipGetLastError();
}

// ---- finishing ----
// What the tile and line kernels read (by value).  A tile is positions [t0, t0 + n); dep[i] = depth[t0 + i].
struct DepthJob {
    const uint32_t *diff; uint32_t *dep; uint8_t *flag; uint32_t t0, n, carry, ref_len;
    const int64_t *c_off; const uint32_t *c_name_off; const char *c_names; int32_t n_contigs;
    // per-base lines: line i is the run [start[i], start[i + 1]); its depth is open_depth for the carried run (i == 0 with have_open), else dep[start[i] - t0]
    const uint32_t *start; uint32_t have_open, open_depth;
    // windows: sums[w], w = win_base[contig] + (position in the contig) / window; lines for the windows [w0, w0 + n_lines)
    unsigned long long *sums; const unsigned long long *win_base; uint32_t window; uint64_t w0;
    uint64_t n_lines;
};

// dep[i] (the scan of the tile's diff alone) += carry; flag[i] = a run starts here as far as the depth says
__global__ void __launch_bounds__(256) k_depth_flags(DepthJob j)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < j.n; i += (uint64_t)gridDim.x * blockDim.x) {
        j.dep[i] += j.carry;
        j.flag[i] = j.diff[(uint64_t)j.t0 + i] != 0u;
    }
}
// ... and where a contig begins, whatever the depth on both sides
__global__ void __launch_bounds__(256) k_depth_contig_flags(DepthJob j)
{
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < (uint32_t)j.n_contigs; c += gridDim.x * blockDim.x) {
        const int64_t o = j.c_off[c];
        if (o >= (int64_t)j.t0 && o < (int64_t)j.t0 + (int64_t)j.n) j.flag[o - (int64_t)j.t0] = 1;
    }
}

// the last contig that begins at or in front of g (an empty contig shares its offset with the next one and is never the answer)
__device__ __forceinline__ int32_t depth_contig(const DepthJob &j, uint64_t g)
{
    int32_t lo = 0, hi = j.n_contigs - 1;
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if ((uint64_t)j.c_off[mid] <= g) lo = mid; else hi = mid - 1; }
    return lo;
}
__device__ __forceinline__ uint64_t depth_contig_end(const DepthJob &j, int32_t c)
{
    const uint64_t e = c + 1 < j.n_contigs ? (uint64_t)j.c_off[c + 1] : (uint64_t)j.ref_len;
    return e < j.ref_len ? e : (uint64_t)j.ref_len;
}

// A thread takes 64 positions of the tile and adds their depths to the windows they lie in: one atomic per window touched.
__global__ void __launch_bounds__(256) k_depth_win_sum(DepthJob j)
{
    const uint64_t n_chunks = ((uint64_t)j.n + 63) / 64;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_chunks; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i1 = k * 64 + 64 < j.n ? k * 64 + 64 : (uint64_t)j.n;
        uint64_t i = k * 64;
        while (i < i1) {
            const uint64_t g = (uint64_t)j.t0 + i;
            const int32_t c = depth_contig(j, g);
            const uint64_t c0 = (uint64_t)j.c_off[c], wk = (g - c0) / j.window;
            uint64_t w_end = c0 + (wk + 1) * j.window;                                  // the window ends here, or with its contig
            const uint64_t c_end = depth_contig_end(j, c);
            if (w_end > c_end) w_end = c_end;
            uint64_t stop = w_end - j.t0 < i1 ? w_end - j.t0 : i1;
            if (stop <= i) stop = i + 1;                                               // (a position beyond every contig's end: none exists below ref_len)
            unsigned long long acc = 0;
            for (; i < stop; ++i) acc += j.dep[i];
            if (acc) atomicAdd(j.sums + j.win_base[c] + wk, acc);
        }
    }
}

// Counts the bytes of a line, or writes them: the same code measures and writes, so the two cannot disagree.
struct DepthEmit {
    char *p; uint64_t n;
    __device__ __forceinline__ void put(char ch) { if (p) p[n] = ch; ++n; }
    __device__ __forceinline__ void putu(uint64_t v)
    {
        char b[20]; int k = 0;
        do { b[k++] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v);
        while (k) put(b[--k]);
    }
    __device__ __forceinline__ void name(const DepthJob &j, int32_t c) { for (uint32_t a = j.c_name_off[c]; a < j.c_name_off[c + 1]; ++a) put(j.c_names[a]); }
};

__device__ __forceinline__ void depth_line(const DepthJob &j, uint64_t i, DepthEmit &o)
{
    if (j.window == 0) {
        const uint32_t a = j.start[i], b = j.start[i + 1];
        const uint32_t d = (i == 0 && j.have_open) ? j.open_depth : j.dep[a - j.t0];
        const int32_t c = depth_contig(j, a);
        const uint64_t c0 = (uint64_t)j.c_off[c];
        o.name(j, c); o.put('\t'); o.putu(a - c0); o.put('\t'); o.putu(b - c0); o.put('\t'); o.putu(d); o.put('\n');
    } else {
        const uint64_t w = j.w0 + i;
        int32_t lo = 0, hi = j.n_contigs - 1;                                          // the last contig whose first window is w or in front of it
        while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (j.win_base[mid] <= w) lo = mid; else hi = mid - 1; }
        const uint64_t c_len = depth_contig_end(j, lo) - (uint64_t)j.c_off[lo];
        const uint64_t a = (w - j.win_base[lo]) * j.window, b = a + j.window < c_len ? a + j.window : c_len, len = b - a;
        const uint64_t sum = j.sums[w];
        const uint64_t h = 100u * (sum / len) + (100u * (sum % len) + len / 2) / len;   // (100 sum + len / 2) / len inside 64 bits
        o.name(j, lo); o.put('\t'); o.putu(a); o.put('\t'); o.putu(b); o.put('\t'); o.putu(h / 100u); o.put('.');
        o.put((char)('0' + (int)(h % 100u) / 10)); o.put((char)('0' + (int)(h % 100u) % 10)); o.put('\n');
    }
}

// len[i] = bytes of line i; len[n_lines] = 0 (the scan's last entry: all bytes)
__global__ void __launch_bounds__(256) k_depth_len(DepthJob j, unsigned long long *__restrict__ len)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < j.n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
        DepthEmit o{ nullptr, 0 };
        depth_line(j, i, o);
        len[i] = o.n;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[j.n_lines] = 0;
}
// lines [i0, i1) to out + off[i] - off[i0]
__global__ void __launch_bounds__(256) k_depth_write(DepthJob j, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ out)
{
    for (uint64_t i = i0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * blockDim.x) {
        DepthEmit o{ out + (off[i] - off[i0]), 0 };
        depth_line(j, i, o);
    }
}

namespace {
template <class T> struct Dev {                                        // a device buffer freed with its owner
    T *p = nullptr;
    Dev() = default; Dev(const Dev &) = delete; Dev &operator=(const Dev &) = delete;
    ~Dev() { if (p) hipFree(p); }
    hipError_t alloc(uint64_t n) { if (p) hipFree(p); p = nullptr; const hipError_t e = hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)); if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); } return e; }
};
}

struct DepthText {
    // what begin was given
    const uint32_t *diff = nullptr; uint32_t ref_len = 0, window = 0, tile = 0; bool bgzf = false;
    DepthJob job{};
    std::vector<int64_t> c_off;
    // buffers, sized by begin for a tile; kept from one text to the next while the sizes hold
    uint64_t buf_tile = 0, text_cap = 0, n_win = 0, sums_cap = 0;
    Dev<uint32_t> dep, start, cnt; Dev<uint8_t> flag, tmp, text; Dev<unsigned long long> len, sums, win_base;
    size_t tmp_bytes = 0;
    Dev<uint32_t> bz_slots, bz_sizes; Dev<unsigned long long> bz_offs; Dev<uint8_t> bz_out;
    char *host = nullptr; uint64_t host_cap = 0;
    // progress
    enum { TILES, WINDOWS, DONE } phase = DONE;
    uint64_t g0 = 0, w_next = 0; uint32_t carry = 0, open_start = 0, open_depth = 0; bool have_open = false;
    std::vector<unsigned long long> h_off; uint64_t line_at = 0; bool lines_pending = false, whole = false;      // the lines of job not yet handed out; whole: they fit one piece
    ~DepthText() { if (host) hipHostFree(host); }
};

DepthText *depth_text_new() { return new DepthText; }
void depth_text_free(DepthText *t) { delete t; }

#define DT_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string("depth text: " #x ": ") + hipGetErrorString(e_); return SALT_E_HIP; } } while (0)

static const uint32_t DEPTH_TILE_DEFAULT = 1u << 22, DEPTH_TILE_MAX = 1u << 26;

int depth_text_begin(DepthText *t, const uint32_t *d_diff, uint32_t ref_len, const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names,
                     const std::vector<int64_t> &h_c_off, uint32_t max_name, uint32_t window, uint32_t tile_positions, int bgzf, std::string &err)
{
    t->phase = DepthText::DONE;
    uint64_t tile = tile_positions ? tile_positions : DEPTH_TILE_DEFAULT;
    if (tile > DEPTH_TILE_MAX) tile = DEPTH_TILE_MAX;
    const uint64_t max_line = (uint64_t)max_name + 40;                 // name, three tabs, three numbers of at most ten digits (a mean: 13 bytes), newline
    const uint64_t text_cap = tile * 16 + max_line;                    // a tile whose lines need more leaves in several pieces
    if (tile != t->buf_tile || text_cap != t->text_cap) {
        t->buf_tile = 0;
        size_t b_scan = 0, b_sel = 0, b_len = 0;
        uint32_t *u = nullptr; uint8_t *f = nullptr; unsigned long long *l = nullptr;
        DT_HIP(rocprim::inclusive_scan(nullptr, b_scan, u, u, (size_t)tile, rocprim::plus<uint32_t>(), nullptr));
        DT_HIP(rocprim::select(nullptr, b_sel, rocprim::counting_iterator<uint32_t>(0), f, u, u, (size_t)tile, (hipStream_t) nullptr));
        DT_HIP(rocprim::exclusive_scan(nullptr, b_len, l, l, 0ull, (size_t)tile + 2, rocprim::plus<unsigned long long>(), nullptr));
        t->tmp_bytes = std::max(b_scan, std::max(b_sel, b_len));
        const uint64_t n_blocks = bgzf_blocks(text_cap);
        const uint64_t bytes = tile * (4 + 4 + 1 + 8) + t->tmp_bytes + text_cap;
        if (t->dep.alloc(tile) != hipSuccess || t->start.alloc(tile + 2) != hipSuccess || t->cnt.alloc(4) != hipSuccess || t->flag.alloc(tile) != hipSuccess ||
            t->tmp.alloc(t->tmp_bytes) != hipSuccess || t->text.alloc(text_cap + 64) != hipSuccess || t->len.alloc(tile + 2) != hipSuccess ||
            t->bz_slots.alloc(n_blocks * (BGZF_SLOT_BYTES / 4)) != hipSuccess || t->bz_sizes.alloc(n_blocks) != hipSuccess || t->bz_offs.alloc(n_blocks + 1) != hipSuccess ||
            t->bz_out.alloc(n_blocks * (BGZF_CUT_BYTES + 31)) != hipSuccess) {
            err = "depth text: no room for the buffers of a tile of " + std::to_string(tile) + " positions: about " + std::to_string(bytes + n_blocks * 2 * BGZF_SLOT_BYTES) + " bytes";
            return SALT_E_NOMEM;
        }
        const uint64_t host_cap = std::max<uint64_t>(text_cap, bgzf_bound(text_cap));
        if (t->host) { hipHostFree(t->host); t->host = nullptr; }
        DT_HIP(hipHostMalloc((void **)&t->host, host_cap, hipHostMallocDefault));
        t->host_cap = host_cap; t->buf_tile = tile; t->text_cap = text_cap;
    }
    const int32_t n_contigs = (int32_t)h_c_off.size();
    uint64_t n_win = 0;
    if (window) {
        std::vector<unsigned long long> base((size_t)n_contigs + 1, 0);
        for (int32_t c = 0; c < n_contigs; ++c) {
            const uint64_t c0 = (uint64_t)h_c_off[(size_t)c], c1 = std::min<uint64_t>(c + 1 < n_contigs ? (uint64_t)h_c_off[(size_t)c + 1] : ref_len, ref_len);
            base[(size_t)c + 1] = base[(size_t)c] + (c1 > c0 ? (c1 - c0 + window - 1) / window : 0);
        }
        n_win = base[(size_t)n_contigs];
        if (n_win + 1 > t->sums_cap) {
            t->sums_cap = 0;
            if (t->sums.alloc(n_win + 1) != hipSuccess) { err = "depth text: no room for the window sums: " + std::to_string((n_win + 1) * 8) + " bytes (8 per window, " + std::to_string(n_win) + " windows of " + std::to_string(window) + " positions)"; return SALT_E_NOMEM; }
            t->sums_cap = n_win + 1;
        }
        if (t->win_base.alloc((uint64_t)n_contigs + 1) != hipSuccess) { err = "depth text: no room for the contigs' window offsets"; return SALT_E_NOMEM; }
        DT_HIP(hipMemcpy(t->win_base.p, base.data(), base.size() * 8, hipMemcpyHostToDevice));
        DT_HIP(hipMemset(t->sums.p, 0, (n_win + 1) * 8));
    }
    t->diff = d_diff; t->ref_len = ref_len; t->window = window; t->tile = (uint32_t)tile; t->bgzf = bgzf != 0; t->c_off = h_c_off; t->n_win = n_win;
    DepthJob &j = t->job;
    j = DepthJob{};
    j.diff = d_diff; j.dep = t->dep.p; j.flag = t->flag.p; j.ref_len = ref_len;
    j.c_off = d_c_off; j.c_name_off = d_c_name_off; j.c_names = d_c_names; j.n_contigs = n_contigs;
    j.start = t->start.p; j.sums = t->sums.p; j.win_base = t->win_base.p; j.window = window;
    t->g0 = 0; t->w_next = 0; t->carry = 0; t->have_open = false; t->open_start = t->open_depth = 0; t->lines_pending = false; t->line_at = 0;
    t->phase = DepthText::TILES;
    return SALT_OK;
}

// the lengths of job's n_lines lines, scanned; the offsets come to the host only when the lines have to leave in pieces
static int depth_lines_measure(DepthText *t, std::string &err)
{
    DepthJob &j = t->job;
    t->lines_pending = false; t->line_at = 0; t->h_off.clear();
    if (j.n_lines == 0) return SALT_OK;
    hipLaunchKernelGGL(k_depth_len, dim3(tally_grid(j.n_lines)), dim3(256), 0, nullptr, j, t->len.p);
    DT_HIP(hipGetLastError());
    DT_HIP(rocprim::exclusive_scan(t->tmp.p, t->tmp_bytes, t->len.p, t->len.p, 0ull, (size_t)j.n_lines + 1, rocprim::plus<unsigned long long>(), nullptr));
    unsigned long long total = 0;
    DT_HIP(hipMemcpy(&total, t->len.p + j.n_lines, 8, hipMemcpyDeviceToHost));
    if (total > t->text_cap) {
        t->h_off.resize((size_t)j.n_lines + 1);
        DT_HIP(hipMemcpy(t->h_off.data(), t->len.p, t->h_off.size() * 8, hipMemcpyDeviceToHost));
    } else t->h_off = { 0ull, total };                                 // one piece: first and last offset
    t->whole = total <= t->text_cap;
    t->lines_pending = true;
    return SALT_OK;
}

// the next piece of the measured lines into the host buffer
static int depth_lines_piece(DepthText *t, const char **data, uint64_t *n_bytes, std::string &err)
{
    DepthJob &j = t->job;
    uint64_t i0 = t->line_at, i1; unsigned long long bytes;
    if (t->whole) { i1 = j.n_lines; bytes = t->h_off[1]; }
    else {
        i1 = i0;
        while (i1 < j.n_lines && t->h_off[(size_t)i1 + 1] - t->h_off[(size_t)i0] <= t->text_cap) ++i1;      // (a single line always fits: text_cap >= max_line)
        if (i1 == i0) { err = "depth text: a line longer than the text buffer"; return SALT_E_HIP; }
        bytes = t->h_off[(size_t)i1] - t->h_off[(size_t)i0];
    }
    hipLaunchKernelGGL(k_depth_write, dim3(tally_grid(i1 - i0)), dim3(256), 0, nullptr, j, t->len.p, i0, i1, reinterpret_cast<char *>(t->text.p));
    DT_HIP(hipGetLastError());
    t->line_at = i1;
    if (i1 == j.n_lines) t->lines_pending = false;
    if (!t->bgzf) {
        DT_HIP(hipMemcpy(t->host, t->text.p, bytes, hipMemcpyDeviceToHost));
        *data = t->host; *n_bytes = bytes;
        return SALT_OK;
    }
    const uint64_t n_blocks = bgzf_blocks(bytes);
    DT_HIP(launch_bgzf_deflate(t->text.p, bytes, t->bz_slots.p, t->bz_sizes.p, t->bz_offs.p, t->bz_out.p, nullptr));
    unsigned long long zbytes = 0;
    DT_HIP(hipMemcpy(&zbytes, t->bz_offs.p + n_blocks, 8, hipMemcpyDeviceToHost));
    if (zbytes > bgzf_bound(bytes) || zbytes > t->host_cap) { err = "depth text: BGZF blocks larger than their bound"; return SALT_E_HIP; }
    DT_HIP(hipMemcpy(t->host, t->bz_out.p, zbytes, hipMemcpyDeviceToHost));
    *data = t->host; *n_bytes = zbytes;
    return SALT_OK;
}

// the next tile: its depths, then its run starts and lines, or its part of the window sums
static int depth_tile(DepthText *t, std::string &err)
{
    DepthJob &j = t->job;
    const uint32_t n = (uint32_t)std::min<uint64_t>(t->tile, (uint64_t)t->ref_len - t->g0);
    j.t0 = (uint32_t)t->g0; j.n = n; j.carry = t->carry; j.n_lines = 0;
    DT_HIP(rocprim::inclusive_scan(t->tmp.p, t->tmp_bytes, t->diff + t->g0, t->dep.p, (size_t)n, rocprim::plus<uint32_t>(), nullptr));
    hipLaunchKernelGGL(k_depth_flags, dim3(tally_grid(n)), dim3(256), 0, nullptr, j);
    DT_HIP(hipGetLastError());
    uint32_t carry_out = 0;
    const bool last = t->g0 + n == t->ref_len;
    if (t->window) {
        hipLaunchKernelGGL(k_depth_win_sum, dim3(tally_grid(((uint64_t)n + 63) / 64)), dim3(256), 0, nullptr, j);
        DT_HIP(hipGetLastError());
        DT_HIP(hipMemcpy(&carry_out, t->dep.p + (n - 1), 4, hipMemcpyDeviceToHost));
    } else {
        hipLaunchKernelGGL(k_depth_contig_flags, dim3(tally_grid((uint64_t)j.n_contigs)), dim3(256), 0, nullptr, j);
        DT_HIP(hipGetLastError());
        const uint32_t lead = t->have_open ? 1u : 0u;
        DT_HIP(rocprim::select(t->tmp.p, t->tmp_bytes, rocprim::counting_iterator<uint32_t>(j.t0), t->flag.p, t->start.p + lead, t->cnt.p, (size_t)n, (hipStream_t) nullptr));
        uint32_t count = 0;
        DT_HIP(hipMemcpy(&count, t->cnt.p, 4, hipMemcpyDeviceToHost));
        DT_HIP(hipMemcpy(&carry_out, t->dep.p + (n - 1), 4, hipMemcpyDeviceToHost));
        if (count > n) { err = "depth text: more run starts than positions"; return SALT_E_HIP; }
        if (lead) DT_HIP(hipMemcpy(t->start.p, &t->open_start, 4, hipMemcpyHostToDevice));
        uint32_t m = lead + count;                                     // starts in hand; every pair of neighbours is a line
        uint32_t new_open = t->open_start;
        if (count) DT_HIP(hipMemcpy(&new_open, t->start.p + (m - 1), 4, hipMemcpyDeviceToHost));
        if (last) { DT_HIP(hipMemcpy(t->start.p + m, &t->ref_len, 4, hipMemcpyHostToDevice)); ++m; }
        j.have_open = lead; j.open_depth = t->open_depth;
        j.n_lines = m ? m - 1 : 0;
        // the run that is open at the tile's end goes on into the next tile: its depth is the depth of the tile's last position
        t->have_open = m > 0; t->open_start = new_open; t->open_depth = carry_out;
        const int rc = depth_lines_measure(t, err);
        if (rc) return rc;
    }
    t->carry = carry_out; t->g0 += n;
    return SALT_OK;
}

int depth_text_next(DepthText *t, const char **data, uint64_t *n_bytes, std::string &err)
{
    *data = nullptr; *n_bytes = 0;
    for (;;) {
        if (t->lines_pending) return depth_lines_piece(t, data, n_bytes, err);
        if (t->phase == DepthText::TILES) {
            if (t->g0 < t->ref_len) { const int rc = depth_tile(t, err); if (rc) { t->phase = DepthText::DONE; return rc; } continue; }
            t->phase = t->window ? DepthText::WINDOWS : DepthText::DONE;
            continue;
        }
        if (t->phase == DepthText::WINDOWS) {
            if (t->w_next >= t->n_win) { t->phase = DepthText::DONE; continue; }
            DepthJob &j = t->job;
            j.w0 = t->w_next; j.n_lines = std::min<uint64_t>(t->tile, t->n_win - t->w_next);
            t->w_next += j.n_lines;
            const int rc = depth_lines_measure(t, err);
            if (rc) { t->phase = DepthText::DONE; return rc; }
            continue;
        }
        return SALT_OK;                                               // complete: *n_bytes == 0
    }
}

} // namespace salt
