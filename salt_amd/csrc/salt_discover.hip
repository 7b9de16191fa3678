// salt_amd/csrc/salt_discover.hip -- SNP candidates off the index's sites (salt --discover; the definition is in include/salt_gpu.h).
//
// Counting: alt is uint64[ref_len], three 21-bit fields a position (the bases outside the position's mixRef mask, in A C G T order); diff is
// this tally's own uint32[ref_len + 1] difference array.  k_disc_add runs behind the kernels that finish a batch's result rows: a thread per
// record walks the row's CIGAR; per M run it marks diff (tally_diff_mark, k_depth_mark's two atomics) and then compares the run's columns
// with the mixRef a 32-bit word -- eight positions -- at a time: the read's eight codes become one-hot nibbles, and a nibble is an event iff
// the mask nibble is not 0, the code is a base and onehot & mask is 0 there.  The run's first and last word and the cut at ref_len are
// masks on that word; nothing branches per base.  Only an event (about 1 in 100 columns) loads its quality byte, ranks its base among
// those outside the mask and does one 64-bit atomic.  The job carries its sign in delta: 2^64 - 1 takes a batch's adds back.
// Finishing (DiscText): the genome goes by in tiles of tile_positions.  A tile of diff is scanned into a tile-sized scratch (rocprim) and
// the carry of the tiles in front is added where it is read; k_disc_flag applies the call rule to every position (leaving at once on a
// zero word unless all_sites); rocprim::select compacts the flagged positions; k_disc_len / scan / k_disc_write measure and write the
// lines with one disc_line (the k_sam_len / k_sam_write pattern).  Lines that outgrow the text buffer leave in several pieces; with bgzf
// the pieces pass k_bgzf_deflate first.  A tile without a line yields no piece.  alt and diff are only read.
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

static constexpr uint32_t DISC_Q_ROWS = 94;                                        // the qualities of the bytes 33 .. 126

// bit 4 j of the result = nibble j of x is not 0
__device__ __forceinline__ uint32_t disc_nz(uint32_t x) { return (x | x >> 1 | x >> 2 | x >> 3) & 0x11111111u; }
__device__ __forceinline__ uint32_t disc_sel4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t k) { return k & 2u ? (k & 1u ? a3 : a2) : (k & 1u ? a1 : a0); }

// The read's codes and the mixRef come in aligned 16-byte pieces, kept in registers from one word of eight columns to the next: a read of
// 100 bases takes about 7 + 4 requests for them.  Only a piece that holds a byte of the read's own (a word of the mixRef's own) is loaded:
// no byte of another allocation is touched.
struct DiscPiece { uintptr_t at; uint4 v; };
__device__ __forceinline__ uint4 disc_piece(uintptr_t a, uintptr_t own_lo, uintptr_t own_hi, DiscPiece &c0, DiscPiece &c1)
{
    if (a + 16 <= own_lo || a >= own_hi) return make_uint4(0, 0, 0, 0);
    if (c0.at == a) return c0.v;
    if (c1.at != a) { c1.at = a; c1.v = *reinterpret_cast<const uint4 *>(a); }
    const DiscPiece t = c0; c0 = c1; c1 = t;
    return c0.v;
}
// the eight bytes at address p (any alignment), those outside [own_lo, own_hi) as they come (the caller masks them)
__device__ __forceinline__ unsigned long long disc_bytes8(uintptr_t p, uintptr_t own_lo, uintptr_t own_hi, DiscPiece &c0, DiscPiece &c1)
{
    const uint32_t sh = (uint32_t)(p & 15u), ws = sh >> 2, bs = (sh & 3u) * 8u;
    const uint4 A = disc_piece(p - sh, own_lo, own_hi, c0, c1);
    uint4 B = make_uint4(0, 0, 0, 0);
    if (sh > 8u) B = disc_piece(p - sh + 16, own_lo, own_hi, c0, c1);
    const uint32_t x0 = disc_sel4(A.x, A.y, A.z, A.w, ws), x1 = disc_sel4(A.y, A.z, A.w, B.x, ws), x2 = disc_sel4(A.z, A.w, B.x, B.y, ws);
    return (unsigned long long)__funnelshift_r(x0, x1, bs) | (unsigned long long)__funnelshift_r(x1, x2, bs) << 32;
}

// One thread per record.  Loads: the row's first 24 bytes and its CIGAR words (tally_row, tally_m_runs), two offsets, on the text path the
// record's quality offset; per M run the read's codes and the mixRef in 16-byte pieces; per event one quality byte.  Nothing is read
// beyond the 16-byte pieces that hold one of the read's own L codes, beyond the q_bytes behind quals or beyond the (ref_len + 7) / 8 words
// of the mixRef, and no position at or beyond ref_len is added to (diff: at most ref_len itself): a row the align kernels got wrong cannot
// make this kernel fault.
__global__ void __launch_bounds__(256) k_disc_add(DiscAdd c)
{
    const uint64_t n_words = ((uint64_t)c.ref_len + 7) / 8;
    const bool ref16 = (reinterpret_cast<uintptr_t>(c.ref) & 15u) == 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n_rec; i += (uint64_t)gridDim.x * blockDim.x) {
        const salt_result_t *q = c.res + i;
        const TallyRow r = tally_row(q, c.pe, c.min_mapq);
        if (r.fate != TALLY_COUNTED) continue;
        const bool rev = r.rev;
        const uint32_t o0 = c.offs[i], L = c.offs[i + 1] - o0;
        const uintptr_t sq = reinterpret_cast<uintptr_t>(c.seqs + o0);
        const uint8_t *qp = nullptr;                                               // the read's L quality bytes, when all of them lie inside q_bytes
        if (c.quals) {
            const uint64_t qo = c.rec ? c.rec[i].qual_off : o0;
            if (qo <= c.q_bytes && L <= c.q_bytes - qo) qp = c.quals + qo;
        }
        DiscPiece s0{ 1, make_uint4(0, 0, 0, 0) }, s1 = s0;                        // (no piece is at an odd address)
        uint64_t r_at = ~0ull; uint4 rv = make_uint4(0, 0, 0, 0);                  // the four mixRef words [4 r_at, 4 r_at + 4)
        tally_m_runs(q, r, [&](uint64_t g, uint32_t s, uint32_t len) {
            const uint64_t end = tally_diff_mark(c.diff, c.ref_len, g, len, (uint32_t)c.delta);      // the run in the genome: [g, end)
            if (g >= end || L == 0u) return;
            for (uint64_t w = g >> 3; w <= (end - 1) >> 3; ++w) {                  // (end <= ref_len: w is one of the mixRef's words)
                const uint64_t p0 = w << 3;
                const uint32_t lo = g > p0 ? (uint32_t)(g - p0) : 0u, hi = end - p0 < 8u ? (uint32_t)(end - p0) : 8u;      // the run's columns of this word: [lo, hi)
                uint32_t valid = (hi == 8u ? ~0u : (1u << (4u * hi)) - 1u) & ~((1u << (4u * lo)) - 1u);
                const int64_t s_base = (int64_t)s + (int64_t)p0 - (int64_t)g;      // column j shows base s_base + j of SEQ as printed
                if (s_base >= (int64_t)L || s_base + 8 <= 0) continue;             // (a run the CIGAR lays outside the read)
                // ... which is the sequenced base at s_base + j, or at L - 1 - (s_base + j) complemented: eight bytes that lie side by side
                const int64_t first = rev ? (int64_t)L - 8 - s_base : s_base;
                unsigned long long b8 = disc_bytes8(sq + first, sq, sq + L, s0, s1);
                if (rev) b8 = __builtin_bswap64(b8);
                uint32_t oh = 0;                                                   // nibble j: the one-hot of that base; 0 for N and outside the read
#pragma unroll
                for (uint32_t j = 0; j < 8; ++j) {
                    uint32_t code = (uint32_t)(b8 >> (8u * j)) & 0xFFu;
                    if (rev) code = 3u - code;                                     // (an N wraps to a code above 3)
                    oh |= (code <= 3u ? 1u << code : 0u) << (4u * j);
                }
                // the columns inside the read: 0 <= s_base + j < L
                if (s_base < 0) valid &= ~((1u << (4u * (uint32_t)-s_base)) - 1u);
                if (s_base + 8 > (int64_t)L) valid &= (1u << (4u * (uint32_t)((int64_t)L - s_base))) - 1u;
                if ((w >> 2) != r_at) {
                    r_at = w >> 2;
                    const uint64_t w4 = r_at << 2;
                    if (ref16 && w4 + 3 < n_words) rv = reinterpret_cast<const uint4 *>(c.ref)[r_at];
                    else rv = make_uint4(c.ref[w4], w4 + 1 < n_words ? c.ref[w4 + 1] : 0u, w4 + 2 < n_words ? c.ref[w4 + 2] : 0u, w4 + 3 < n_words ? c.ref[w4 + 3] : 0u);
                }
                const uint32_t mk = disc_sel4(rv.x, rv.y, rv.z, rv.w, (uint32_t)w & 3u);
                uint32_t ev = disc_nz(mk) & disc_nz(oh) & ~disc_nz(oh & mk) & valid;
                for (; ev; ev &= ev - 1u) {
                    const uint32_t j = ((uint32_t)__ffs(ev) - 1u) >> 2;
                    const uint32_t m = (mk >> (4u * j)) & 15u, b = (uint32_t)__ffs((oh >> (4u * j)) & 15u) - 1u;
                    if (qp) {
                        const uint32_t x = (uint32_t)(s_base + (int64_t)j);
                        const uint32_t qv = (uint32_t)qp[rev ? L - 1u - x : x] - 33u;
                        if (qv < DISC_Q_ROWS && qv < c.min_baseq) continue;       // a usable quality below the floor
                    }
                    const uint32_t k = (uint32_t)__popc(~m & 15u & ((1u << b) - 1u));
                    atomicAdd(c.alt + p0 + j, (1ull << (SALT_DISC_FIELD_BITS * k)) * c.delta);
                }
            }
        });
    }
}

hipError_t launch_disc_add(const DiscAdd &c, hipStream_t st)
{
    if (c.n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(k_disc_add, dim3(tally_grid(c.n_rec)), dim3(256), 0, st, c);
    return hipGetLastError();
}

// ---- finishing ----
// What the tile and line kernels read (by value).  A tile is positions [t0, t0 + n); depth[t0 + i] = dep[i] + carry.
struct DiscJob {
    const unsigned long long *alt; const uint32_t *diff; uint32_t *dep; uint8_t *flag; uint32_t t0, n, carry;
    const uint32_t *ref, *text; uint32_t ref_len, text_len;                        // the 4-bit mixRef, the 2-bit genome and the positions each holds
    const int64_t *c_off; const uint32_t *c_name_off; const char *c_names; int32_t n_contigs;
    uint32_t min_alt, min_pct, all_sites;
    const uint32_t *cand; uint32_t *seen; uint64_t n_lines;                        // line i is position cand[i]; seen[c] = contig c has a line
};

__device__ __forceinline__ uint32_t disc_mask(const DiscJob &j, uint32_t g) { return (j.ref[g >> 3] >> (4u * (g & 7u))) & 15u; }

// the bases called at a position with the word w, the mask m and the depth given, as a set of four bits
__device__ __forceinline__ uint32_t disc_called(unsigned long long w, uint32_t m, uint32_t depth, uint32_t min_alt, uint32_t min_pct)
{
    if (m == 0u) return 0u;
    uint32_t called = 0, k = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
        if ((m >> b) & 1u) continue;
        const unsigned long long n = (w >> (SALT_DISC_FIELD_BITS * k)) & SALT_DISC_FIELD_MAX;
        if (n >= min_alt && 100ull * n >= (unsigned long long)min_pct * depth) called |= 1u << b;
        ++k;
    }
    return called;
}

// flag[i] = position t0 + i gets a line
__global__ void __launch_bounds__(256) k_disc_flag(DiscJob j)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < j.n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t g = j.t0 + (uint32_t)i;
        const unsigned long long w = j.alt[g];
        if (w == 0ull && !j.all_sites) { j.flag[i] = 0; continue; }
        const uint32_t m = disc_mask(j, g);
        j.flag[i] = disc_called(w, m, j.dep[i] + j.carry, j.min_alt, j.min_pct) != 0u || (j.all_sites && (m & (m - 1u)) != 0u);
    }
}

// Counts the bytes of a line, or writes them: the same code measures and writes, so the two cannot disagree.
struct DiscEmit {
    char *p; uint64_t n;
    __device__ __forceinline__ void put(char ch) { if (p) p[n] = ch; ++n; }
    __device__ __forceinline__ void putu(uint64_t v)
    {
        char b[20]; int k = 0;
        do { b[k++] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v);
        while (k) put(b[--k]);
    }
};

// the line of candidate i of the tile; returns its contig
__device__ __forceinline__ int32_t disc_line(const DiscJob &j, uint64_t i, DiscEmit &o)
{
    const uint32_t g = j.cand[i];
    const uint32_t depth = j.dep[g - j.t0] + j.carry, m = disc_mask(j, g);
    const unsigned long long w = j.alt[g];
    const uint32_t al = m | disc_called(w, m, depth, j.min_alt, j.min_pct);
    const uint32_t r = g < j.text_len ? (j.text[g >> 4] >> (30u - 2u * (g & 15u))) & 3u : 0u;
    int32_t lo = 0, hi = j.n_contigs - 1;                                          // the last contig that begins at or in front of g
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if ((uint64_t)j.c_off[mid] <= g) lo = mid; else hi = mid - 1; }
    const char NT[4] = { 'A', 'C', 'G', 'T' };
    for (uint32_t a = j.c_name_off[lo]; a < j.c_name_off[lo + 1]; ++a) o.put(j.c_names[a]);
    o.put('\t'); o.putu((uint64_t)g - (uint64_t)j.c_off[lo] + 1u); o.put('\t');
    bool first = true;
    for (uint32_t b = 0; b < 4; ++b) if ((al >> b) & 1u) { if (!first) o.put('/'); o.put(NT[b]); first = false; }
    o.put('\t'); o.put(NT[r]); o.put('\t'); o.putu(depth); o.put('\t');
    uint32_t k = 0;
    for (uint32_t b = 0; b < 4; ++b) {
        if (b) o.put(',');
        if ((m >> b) & 1u) o.put('.');
        else { o.putu((w >> (SALT_DISC_FIELD_BITS * k)) & SALT_DISC_FIELD_MAX); ++k; }
    }
    o.put('\n');
    return lo;
}

// len[i] = bytes of line i; len[n_lines] = 0 (the scan's last entry: all bytes); the lines' contigs are marked
__global__ void __launch_bounds__(256) k_disc_len(DiscJob j, unsigned long long *__restrict__ len)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < j.n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
        DiscEmit o{ nullptr, 0 };
        const int32_t c = disc_line(j, i, o);
        len[i] = o.n;
        j.seen[c] = 1u;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[j.n_lines] = 0;
}
// lines [i0, i1) to out + off[i] - off[i0]
__global__ void __launch_bounds__(256) k_disc_write(DiscJob j, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ out)
{
    for (uint64_t i = i0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * blockDim.x) {
        DiscEmit o{ out + (off[i] - off[i0]), 0 };
        disc_line(j, i, o);
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

struct DiscText {
    DiscJob job{};
    uint32_t ref_len = 0, tile = 0; bool bgzf = false;
    // buffers, sized by begin for a tile; kept from one text to the next while the sizes hold
    uint64_t buf_tile = 0, text_cap = 0; int32_t seen_contigs = -1;
    Dev<uint32_t> dep, cand, cnt, seen; Dev<uint8_t> flag, tmp, text; Dev<unsigned long long> len;
    size_t tmp_bytes = 0;
    Dev<uint32_t> bz_slots, bz_sizes; Dev<unsigned long long> bz_offs; Dev<uint8_t> bz_out;
    char *host = nullptr; uint64_t host_cap = 0;
    // progress
    uint64_t g0 = 0; uint32_t carry = 0; bool active = false, complete = false;
    std::vector<unsigned long long> h_off; uint64_t line_at = 0; bool lines_pending = false, whole = false;      // the lines of job not yet handed out; whole: they fit one piece
    ~DiscText() { if (host) hipHostFree(host); }
};

DiscText *disc_text_new() { return new DiscText; }
void disc_text_free(DiscText *t) { delete t; }

#define DC_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string("discover text: " #x ": ") + hipGetErrorString(e_); return SALT_E_HIP; } } while (0)

static const uint32_t DISC_TILE_DEFAULT = 1u << 22, DISC_TILE_MAX = 1u << 26;

int disc_text_begin(DiscText *t, const unsigned long long *d_alt, const uint32_t *d_diff, const uint32_t *d_ref, const uint32_t *d_text, uint32_t ref_len, uint32_t text_len,
                    const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names, int32_t n_contigs, uint32_t max_name,
                    uint32_t min_alt, uint32_t min_pct, int all_sites, uint32_t tile_positions, int bgzf, std::string &err)
{
    t->active = false; t->complete = false;
    uint64_t tile = tile_positions ? tile_positions : DISC_TILE_DEFAULT;
    if (tile > DISC_TILE_MAX) tile = DISC_TILE_MAX;
    const uint64_t max_line = (uint64_t)max_name + 80;                 // name, five tabs, two numbers of ten digits, seven bytes of alleles, a letter, four counts of seven digits, three commas, newline
    const uint64_t text_cap = tile * 8 + max_line;                     // candidates are sparse; a tile whose lines need more leaves in several pieces
    if (tile != t->buf_tile || text_cap != t->text_cap) {
        t->buf_tile = 0;
        size_t b_scan = 0, b_sel = 0, b_len = 0;
        uint32_t *u = nullptr; uint8_t *f = nullptr; unsigned long long *l = nullptr;
        DC_HIP(rocprim::inclusive_scan(nullptr, b_scan, u, u, (size_t)tile, rocprim::plus<uint32_t>(), nullptr));
        DC_HIP(rocprim::select(nullptr, b_sel, rocprim::counting_iterator<uint32_t>(0), f, u, u, (size_t)tile, (hipStream_t) nullptr));
        DC_HIP(rocprim::exclusive_scan(nullptr, b_len, l, l, 0ull, (size_t)tile + 1, rocprim::plus<unsigned long long>(), nullptr));
        t->tmp_bytes = std::max(b_scan, std::max(b_sel, b_len));
        const uint64_t n_blocks = bgzf_blocks(text_cap);
        const uint64_t bytes = tile * (4 + 4 + 1 + 8) + t->tmp_bytes + text_cap;
        if (t->dep.alloc(tile) != hipSuccess || t->cand.alloc(tile) != hipSuccess || t->cnt.alloc(4) != hipSuccess || t->flag.alloc(tile) != hipSuccess ||
            t->tmp.alloc(t->tmp_bytes) != hipSuccess || t->text.alloc(text_cap + 64) != hipSuccess || t->len.alloc(tile + 1) != hipSuccess ||
            t->bz_slots.alloc(n_blocks * (BGZF_SLOT_BYTES / 4)) != hipSuccess || t->bz_sizes.alloc(n_blocks) != hipSuccess || t->bz_offs.alloc(n_blocks + 1) != hipSuccess ||
            t->bz_out.alloc(n_blocks * (BGZF_CUT_BYTES + 31)) != hipSuccess) {
            err = "discover text: no room for the buffers of a tile of " + std::to_string(tile) + " positions: about " + std::to_string(bytes + n_blocks * 2 * BGZF_SLOT_BYTES) + " bytes";
            return SALT_E_NOMEM;
        }
        const uint64_t host_cap = std::max<uint64_t>(text_cap, bgzf_bound(text_cap));
        if (t->host) { hipHostFree(t->host); t->host = nullptr; }
        DC_HIP(hipHostMalloc((void **)&t->host, host_cap, hipHostMallocDefault));
        t->host_cap = host_cap; t->buf_tile = tile; t->text_cap = text_cap;
    }
    if (t->seen_contigs != n_contigs) {
        t->seen_contigs = -1;
        if (t->seen.alloc((uint64_t)n_contigs) != hipSuccess) { err = "discover text: no room for the contigs' marks"; return SALT_E_NOMEM; }
        t->seen_contigs = n_contigs;
    }
    DC_HIP(hipMemset(t->seen.p, 0, (size_t)n_contigs * 4));
    DiscJob &j = t->job;
    j = DiscJob{};
    j.alt = d_alt; j.diff = d_diff; j.dep = t->dep.p; j.flag = t->flag.p; j.ref = d_ref; j.text = d_text; j.ref_len = ref_len; j.text_len = text_len;
    j.c_off = d_c_off; j.c_name_off = d_c_name_off; j.c_names = d_c_names; j.n_contigs = n_contigs;
    j.min_alt = min_alt; j.min_pct = min_pct; j.all_sites = all_sites ? 1u : 0u; j.cand = t->cand.p; j.seen = t->seen.p;
    t->ref_len = ref_len; t->tile = (uint32_t)tile; t->bgzf = bgzf != 0;
    t->g0 = 0; t->carry = 0; t->lines_pending = false; t->line_at = 0;
    t->active = true;
    return SALT_OK;
}

// the next tile: its depths, its flagged positions, the lengths of their lines, scanned; the offsets come to the host only when the lines
// have to leave in pieces
static int disc_tile(DiscText *t, std::string &err)
{
    DiscJob &j = t->job;
    const uint32_t n = (uint32_t)std::min<uint64_t>(t->tile, (uint64_t)t->ref_len - t->g0);
    j.t0 = (uint32_t)t->g0; j.n = n; j.carry = t->carry; j.n_lines = 0;
    t->lines_pending = false; t->line_at = 0; t->h_off.clear();
    DC_HIP(rocprim::inclusive_scan(t->tmp.p, t->tmp_bytes, j.diff + t->g0, t->dep.p, (size_t)n, rocprim::plus<uint32_t>(), nullptr));
    hipLaunchKernelGGL(k_disc_flag, dim3(tally_grid(n)), dim3(256), 0, nullptr, j);
    DC_HIP(hipGetLastError());
    DC_HIP(rocprim::select(t->tmp.p, t->tmp_bytes, rocprim::counting_iterator<uint32_t>(j.t0), t->flag.p, t->cand.p, t->cnt.p, (size_t)n, (hipStream_t) nullptr));
    uint32_t count = 0, last = 0;
    DC_HIP(hipMemcpy(&count, t->cnt.p, 4, hipMemcpyDeviceToHost));
    DC_HIP(hipMemcpy(&last, t->dep.p + (n - 1), 4, hipMemcpyDeviceToHost));
    if (count > n) { err = "discover text: more candidates than positions"; return SALT_E_HIP; }
    t->carry += last; t->g0 += n;                                      // (j.carry stays this tile's while its lines are written)
    if (count == 0) return SALT_OK;
    j.n_lines = count;
    hipLaunchKernelGGL(k_disc_len, dim3(tally_grid(count)), dim3(256), 0, nullptr, j, t->len.p);
    DC_HIP(hipGetLastError());
    DC_HIP(rocprim::exclusive_scan(t->tmp.p, t->tmp_bytes, t->len.p, t->len.p, 0ull, (size_t)count + 1, rocprim::plus<unsigned long long>(), nullptr));
    unsigned long long total = 0;
    DC_HIP(hipMemcpy(&total, t->len.p + count, 8, hipMemcpyDeviceToHost));
    t->whole = total <= t->text_cap;
    if (!t->whole) {
        t->h_off.resize((size_t)count + 1);
        DC_HIP(hipMemcpy(t->h_off.data(), t->len.p, t->h_off.size() * 8, hipMemcpyDeviceToHost));
    } else t->h_off = { 0ull, total };                                 // one piece: first and last offset
    t->lines_pending = true;
    return SALT_OK;
}

// the next piece of the measured lines into the host buffer
static int disc_piece(DiscText *t, const char **data, uint64_t *n_bytes, std::string &err)
{
    DiscJob &j = t->job;
    uint64_t i0 = t->line_at, i1; unsigned long long bytes;
    if (t->whole) { i1 = j.n_lines; bytes = t->h_off[1]; }
    else {
        i1 = i0;
        while (i1 < j.n_lines && t->h_off[(size_t)i1 + 1] - t->h_off[(size_t)i0] <= t->text_cap) ++i1;      // (a single line always fits: text_cap >= max_line)
        if (i1 == i0) { err = "discover text: a line longer than the text buffer"; return SALT_E_HIP; }
        bytes = t->h_off[(size_t)i1] - t->h_off[(size_t)i0];
    }
    hipLaunchKernelGGL(k_disc_write, dim3(tally_grid(i1 - i0)), dim3(256), 0, nullptr, j, t->len.p, i0, i1, reinterpret_cast<char *>(t->text.p));
    DC_HIP(hipGetLastError());
    t->line_at = i1;
    if (i1 == j.n_lines) t->lines_pending = false;
    if (!t->bgzf) {
        DC_HIP(hipMemcpy(t->host, t->text.p, bytes, hipMemcpyDeviceToHost));
        *data = t->host; *n_bytes = bytes;
        return SALT_OK;
    }
    const uint64_t n_blocks = bgzf_blocks(bytes);
    DC_HIP(launch_bgzf_deflate(t->text.p, bytes, t->bz_slots.p, t->bz_sizes.p, t->bz_offs.p, t->bz_out.p, nullptr));
    unsigned long long zbytes = 0;
    DC_HIP(hipMemcpy(&zbytes, t->bz_offs.p + n_blocks, 8, hipMemcpyDeviceToHost));
    if (zbytes > bgzf_bound(bytes) || zbytes > t->host_cap) { err = "discover text: BGZF blocks larger than their bound"; return SALT_E_HIP; }
    DC_HIP(hipMemcpy(t->host, t->bz_out.p, zbytes, hipMemcpyDeviceToHost));
    *data = t->host; *n_bytes = zbytes;
    return SALT_OK;
}

int disc_text_next(DiscText *t, const char **data, uint64_t *n_bytes, std::string &err)
{
    *data = nullptr; *n_bytes = 0;
    while (t->active) {
        if (t->lines_pending) { const int rc = disc_piece(t, data, n_bytes, err); if (rc) t->active = false; return rc; }
        if (t->g0 >= t->ref_len) { t->active = false; t->complete = true; break; }      // complete: *n_bytes == 0
        const int rc = disc_tile(t, err);
        if (rc) { t->active = false; return rc; }
    }
    return SALT_OK;
}

int disc_text_seen(DiscText *t, uint8_t *seen, uint64_t cap, std::string &err)
{
    if (!t->complete) { err = "discover text: the contigs' marks stand once the text is complete"; return SALT_E_INVAL; }
    if (cap < (uint64_t)t->seen_contigs) { err = "discover text: room for " + std::to_string(cap) + " marks, the index has " + std::to_string(t->seen_contigs) + " contigs"; return SALT_E_INVAL; }
    std::vector<uint32_t> h((size_t)t->seen_contigs);
    DC_HIP(hipMemcpy(h.data(), t->seen.p, h.size() * 4, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < h.size(); ++c) seen[c] = h[c] ? 1 : 0;
    return SALT_OK;
}

} // namespace salt
