// salt_amd/csrc/salt_gt.hip -- genotypes at the index's SNP sites (salt --genotype; the definition is in include/salt_gpu.h).
//
// Counting: sums is salt_gt_site_t[n_sites], per base A C G T the four uint64 words { n, sm, sx, sh }.  k_gt_add runs behind the kernels
// that finish a batch's result rows and has the shape of k_snp_count: a thread per record walks the row's CIGAR over the index's site
// table; every site an M run covers with a base of the read's is one event, which adds 1 and the three penalties of the base's quality
// (SALT_GT_TABLE, held in LDS) to the base's words: four 64-bit atomics into one 32-byte sector.  The qualities are read the way k_errprof
// reads them (quals, rec, q_bytes of the call's source).  The job carries its sign in delta: 2^64 - 1 takes a batch's adds back.
// Finishing (GtText): the sites go by in tiles of tile_sites.  A thread per site makes the call from the site's sums, its mixRef mask and the
// genome's base, and measures its line (k_gt_len); the lengths are scanned (rocprim); k_gt_write makes the call again and writes the line
// (the k_sam_len / k_sam_write pattern: the same code measures and writes).  Lines that outgrow the text buffer leave in several pieces.
// With bgzf the pieces pass k_bgzf_deflate first.  The sums are only read.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/salt_gt_table.h"
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_tally.h"

namespace salt {

static_assert(sizeof(salt_gt_site_t) == 128 && sizeof(salt_gt_base_t) == 32, "a base's four words are one 32-byte sector");

__constant__ uint32_t GT_TABLE_DEV[SALT_GT_Q_ROWS][3] = { SALT_GT_TABLE_ROWS };

// One thread per record.  Loads: those of k_snp_count and, per event, one quality byte.  Nothing is read beyond the read's own codes, beyond
// the q_bytes behind quals or beyond the table's n_win records, and no site at or beyond n_sites is added to: a row the align kernels got
// wrong cannot make this kernel fault.
__global__ void __launch_bounds__(256) k_gt_add(GtAdd c)
{
    __shared__ uint32_t pen[SALT_GT_Q_ROWS * 3];
    for (uint32_t x = threadIdx.x; x < SALT_GT_Q_ROWS * 3; x += blockDim.x) pen[x] = GT_TABLE_DEV[x / 3][x % 3];
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n_rec; i += (uint64_t)gridDim.x * blockDim.x) {
        const salt_result_t *q = c.res + i;
        const TallyRow r = tally_row(q, c.pe, c.min_mapq);
        if (r.fate != TALLY_COUNTED) continue;
        const bool rev = r.rev;
        const uint32_t o0 = c.offs[i], L = c.offs[i + 1] - o0;
        const uint8_t *sq = c.seqs + o0;
        const uint8_t *qp = nullptr;                                               // the read's L quality bytes, when all of them lie inside q_bytes
        if (c.quals) {
            const uint64_t qo = c.rec ? c.rec[i].qual_off : o0;
            if (qo <= c.q_bytes && L <= c.q_bytes - qo) qp = c.quals + qo;
        }
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
                    const uint32_t at = rev ? L - 1u - (uint32_t)j : (uint32_t)j;  // the same base as sequenced: its code and its quality
                    uint32_t code = sq[at];
                    if (code > 3u) continue;                                       // N is no event
                    if (rev) code = 3u - code;
                    const uint64_t site = (uint64_t)t.rank + (uint32_t)__popcll(t.bits & ((1ull << b) - 1ull));
                    if (site >= c.n_sites) continue;
                    uint32_t qv = SALT_GT_Q_NONE;
                    if (qp) { const uint32_t qb = qp[at]; if (qb - 33u < (uint32_t)SALT_GT_Q_ROWS) qv = qb - 33u; }
                    unsigned long long *cell = c.sums + site * 16 + code * 4;
                    atomicAdd(cell + 0, c.delta);
                    atomicAdd(cell + 1, (unsigned long long)pen[qv * 3 + 0] * c.delta);
                    atomicAdd(cell + 2, (unsigned long long)pen[qv * 3 + 1] * c.delta);
                    atomicAdd(cell + 3, (unsigned long long)pen[qv * 3 + 2] * c.delta);
                }
            }
        });
    }
}

__global__ void __launch_bounds__(256) k_gt_sum(unsigned long long *__restrict__ sums, const unsigned long long *__restrict__ in, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) if (in[i]) atomicAdd(sums + i, in[i]);
}

hipError_t launch_gt_add(const GtAdd &c, hipStream_t st)
{
    if (c.n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gt_add, dim3(tally_grid(c.n_rec)), dim3(256), 0, st, c);
    return hipGetLastError();
}
hipError_t launch_gt_sum(unsigned long long *sums, const unsigned long long *in, uint64_t n_words, hipStream_t st)
{
    if (n_words == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gt_sum, dim3(tally_grid(n_words)), dim3(256), 0, st, sums, in, n_words);
    return hipGetLastError();
}

// ---- finishing ----
// What the call and line kernels read (by value).  A tile is sites [s0, s0 + n).
struct GtJob {
    const unsigned long long *sums; const uint32_t *pos;                           // sums[n_sites][16], pos[n_sites]: the sites' genome positions
    const uint32_t *ref, *text; uint32_t ref_len, text_len;                        // the 4-bit mixRef, the 2-bit genome and the positions each holds
    const int64_t *c_off; const uint32_t *c_name_off; const char *c_names; int32_t n_contigs;
    uint64_t s0; uint32_t n;
};

// Counts the bytes of a line, or writes them: the same code measures and writes, so the two cannot disagree.
struct GtEmit {
    char *p; uint64_t n;
    __device__ __forceinline__ void put(char ch) { if (p) p[n] = ch; ++n; }
    __device__ __forceinline__ void puts(const char *s) { while (*s) put(*s++); }
    __device__ __forceinline__ void putu(uint64_t v)
    {
        char b[20]; int k = 0;
        do { b[k++] = (char)('0' + (int)(v % 10u)); v /= 10u; } while (v);
        while (k) put(b[--k]);
    }
};

// the record of site i of the tile
__device__ __forceinline__ void gt_line(const GtJob &j, uint64_t i, GtEmit &o)
{
    const uint64_t site = j.s0 + i;
    const uint32_t g = j.pos[site];
    const uint32_t mask = g < j.ref_len ? (j.ref[g >> 3] >> (4u * (g & 7u))) & 15u : 0u;
    const uint32_t r = g < j.text_len ? (j.text[g >> 4] >> (30u - 2u * (g & 15u))) & 3u : 0u;
    unsigned long long n[4], sm[4], sx[4], sh[4], all_x = 0, dp = 0;
    const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(j.sums + site * 16);
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
        const ulonglong2 lo = row[2 * b], hi = row[2 * b + 1];
        n[b] = lo.x; sm[b] = lo.y; sx[b] = hi.x; sh[b] = hi.y;
        all_x += sx[b]; dp += n[b];
    }
    // alleles: the genome's base, then the mask's other letters in A C G T order; al[] as one word, four bits an allele
    uint32_t al = r, n_al = 1;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) if (((mask >> b) & 1u) && b != r) { al |= b << (4u * n_al); ++n_al; }
    auto allele = [&](uint32_t k) { return (al >> (4u * k)) & 3u; };
    auto pick = [](const unsigned long long v[4], uint32_t b) { return b & 2u ? (b & 1u ? v[3] : v[2]) : (b & 1u ? v[1] : v[0]); };
    // raw penalties in VCF order k = b (b + 1) / 2 + a, a <= b
    unsigned long long raw[10], min_raw = ~0ull;
    uint32_t n_gt = 0, best = 0, best_a = 0, best_b = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b)
#pragma unroll
        for (uint32_t a = 0; a <= b; ++a) {
            const uint32_t k = b * (b + 1) / 2 + a;
            raw[k] = 0;
            if (b >= n_al) continue;
            const uint32_t ca = allele(a), cb = allele(b);
            raw[k] = a == b ? pick(sm, ca) + (all_x - pick(sx, ca)) : pick(sh, ca) + pick(sh, cb) + (all_x - pick(sx, ca) - pick(sx, cb));
            if (raw[k] < min_raw) { min_raw = raw[k]; best = k; best_a = a; best_b = b; }
            ++n_gt;
        }
    // the contig that contains g: the last one that begins at or in front of it
    int32_t lo = 0, hi = j.n_contigs - 1;
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if ((uint64_t)j.c_off[mid] <= g) lo = mid; else hi = mid - 1; }
    for (uint32_t a = j.c_name_off[lo]; a < j.c_name_off[lo + 1]; ++a) o.put(j.c_names[a]);
    o.put('\t'); o.putu((uint64_t)g - (uint64_t)j.c_off[lo] + 1u); o.puts("\t.\t");
    const char NT[4] = { 'A', 'C', 'G', 'T' };
    o.put(NT[r]); o.put('\t');
    for (uint32_t k = 1; k < n_al; ++k) { if (k > 1) o.put(','); o.put(NT[allele(k)]); }
    o.put('\t');
    if (dp == 0) {
        o.puts(".\t.\tDP=0\tGT:AD:DP:GQ:PL\t./.:");
        for (uint32_t k = 0; k < n_al; ++k) { if (k) o.put(','); o.put('0'); }
        o.puts(":0:.:.\n");
        return;
    }
    unsigned long long gq = ~0ull;
    for (uint32_t k = 0; k < n_gt; ++k) { const unsigned long long pl = (raw[k] - min_raw + 2048u) >> 12; if (k != best && pl < gq) gq = pl; }
    if (gq > 99u) gq = 99u;
    o.putu((raw[0] - min_raw + 2048u) >> 12); o.puts("\t.\tDP="); o.putu(dp); o.puts("\tGT:AD:DP:GQ:PL\t");
    o.putu(best_a); o.put('/'); o.putu(best_b); o.put(':');
    for (uint32_t k = 0; k < n_al; ++k) { if (k) o.put(','); o.putu(pick(n, allele(k))); }
    o.put(':'); o.putu(dp); o.put(':'); o.putu(gq); o.put(':');
    for (uint32_t k = 0; k < n_gt; ++k) { if (k) o.put(','); o.putu((raw[k] - min_raw + 2048u) >> 12); }
    o.put('\n');
}

// len[i] = bytes of line i; len[n] = 0 (the scan's last entry: all bytes)
__global__ void __launch_bounds__(256) k_gt_len(GtJob j, unsigned long long *__restrict__ len)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < j.n; i += (uint64_t)gridDim.x * blockDim.x) {
        GtEmit o{ nullptr, 0 };
        gt_line(j, i, o);
        len[i] = o.n;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[j.n] = 0;
}
// lines [i0, i1) to out + off[i] - off[i0]
__global__ void __launch_bounds__(256) k_gt_write(GtJob j, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ out)
{
    for (uint64_t i = i0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * blockDim.x) {
        GtEmit o{ out + (off[i] - off[i0]), 0 };
        gt_line(j, i, o);
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

struct GtText {
    GtJob job{};
    uint64_t n_sites = 0, tile = 0; bool bgzf = false;
    // buffers, sized by begin for a tile; kept from one text to the next while the sizes hold
    uint64_t buf_tile = 0, text_cap = 0, pos_sites = ~0ull;
    Dev<uint32_t> pos; Dev<uint8_t> tmp, text; Dev<unsigned long long> len;
    size_t tmp_bytes = 0;
    Dev<uint32_t> bz_slots, bz_sizes; Dev<unsigned long long> bz_offs; Dev<uint8_t> bz_out;
    char *host = nullptr; uint64_t host_cap = 0;
    // progress
    uint64_t s_next = 0; bool active = false;
    std::vector<unsigned long long> h_off; uint64_t line_at = 0; bool lines_pending = false, whole = false;      // the lines of job not yet handed out; whole: they fit one piece
    ~GtText() { if (host) hipHostFree(host); }
};

GtText *gt_text_new() { return new GtText; }
void gt_text_free(GtText *t) { delete t; }

#define GT_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string("genotype text: " #x ": ") + hipGetErrorString(e_); return SALT_E_HIP; } } while (0)

static const uint32_t GT_TILE_DEFAULT = 1u << 18, GT_TILE_MAX = 1u << 22;

int gt_text_begin(GtText *t, const unsigned long long *d_sums, const SnpWin *d_tab, uint64_t n_win, uint32_t n_sites, const uint32_t *d_ref, const uint32_t *d_text,
                  uint32_t ref_len, uint32_t text_len, const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names, int32_t n_contigs, uint32_t max_name,
                  uint32_t tile_sites, int bgzf, std::string &err)
{
    t->active = false;
    uint64_t tile = tile_sites ? tile_sites : GT_TILE_DEFAULT;
    if (tile > GT_TILE_MAX) tile = GT_TILE_MAX;
    // the longest line: name, position, the fixed fields, QUAL and two DP of 20 digits, four AD, GQ and ten PL of 20 digits with their separators
    const uint64_t max_line = (uint64_t)max_name + 64 + 18 * 21;
    const uint64_t text_cap = tile * 96 + max_line;                    // a tile whose lines need more leaves in several pieces
    if (tile != t->buf_tile || text_cap != t->text_cap) {
        t->buf_tile = 0;
        unsigned long long *l = nullptr;
        size_t b_len = 0;
        GT_HIP(rocprim::exclusive_scan(nullptr, b_len, l, l, 0ull, (size_t)tile + 1, rocprim::plus<unsigned long long>(), nullptr));
        t->tmp_bytes = b_len;
        const uint64_t n_blocks = bgzf_blocks(text_cap);
        if (t->tmp.alloc(t->tmp_bytes) != hipSuccess || t->text.alloc(text_cap + 64) != hipSuccess || t->len.alloc(tile + 1) != hipSuccess ||
            t->bz_slots.alloc(n_blocks * (BGZF_SLOT_BYTES / 4)) != hipSuccess || t->bz_sizes.alloc(n_blocks) != hipSuccess || t->bz_offs.alloc(n_blocks + 1) != hipSuccess ||
            t->bz_out.alloc(n_blocks * (BGZF_CUT_BYTES + 31)) != hipSuccess) {
            err = "genotype text: no room for the buffers of a tile of " + std::to_string(tile) + " sites: about " + std::to_string(tile * 8 + t->tmp_bytes + text_cap + n_blocks * 2 * BGZF_SLOT_BYTES) + " bytes";
            return SALT_E_NOMEM;
        }
        const uint64_t host_cap = std::max<uint64_t>(text_cap, bgzf_bound(text_cap));
        if (t->host) { hipHostFree(t->host); t->host = nullptr; }
        GT_HIP(hipHostMalloc((void **)&t->host, host_cap, hipHostMallocDefault));
        t->host_cap = host_cap; t->buf_tile = tile; t->text_cap = text_cap;
    }
    if (t->pos_sites != n_sites) {                                     // the sites' positions, once per index
        t->pos_sites = ~0ull;
        if (t->pos.alloc(n_sites) != hipSuccess) { err = "genotype text: no room for the sites' positions: " + std::to_string((uint64_t)n_sites * 4) + " bytes (4 per site)"; return SALT_E_NOMEM; }
        if (n_sites) GT_HIP(launch_snp_pos(d_tab, n_win, t->pos.p, nullptr));
        t->pos_sites = n_sites;
    }
    GtJob &j = t->job;
    j = GtJob{};
    j.sums = d_sums; j.pos = t->pos.p; j.ref = d_ref; j.text = d_text; j.ref_len = ref_len; j.text_len = text_len;
    j.c_off = d_c_off; j.c_name_off = d_c_name_off; j.c_names = d_c_names; j.n_contigs = n_contigs;
    t->n_sites = n_sites; t->tile = tile; t->bgzf = bgzf != 0;
    t->s_next = 0; t->lines_pending = false; t->line_at = 0;
    t->active = true;
    return SALT_OK;
}

// the next tile: the lengths of its lines, scanned; the offsets come to the host only when the lines have to leave in pieces
static int gt_tile(GtText *t, std::string &err)
{
    GtJob &j = t->job;
    j.s0 = t->s_next; j.n = (uint32_t)std::min<uint64_t>(t->tile, t->n_sites - t->s_next);
    t->s_next += j.n;
    t->lines_pending = false; t->line_at = 0; t->h_off.clear();
    hipLaunchKernelGGL(k_gt_len, dim3(tally_grid(j.n)), dim3(256), 0, nullptr, j, t->len.p);
    GT_HIP(hipGetLastError());
    GT_HIP(rocprim::exclusive_scan(t->tmp.p, t->tmp_bytes, t->len.p, t->len.p, 0ull, (size_t)j.n + 1, rocprim::plus<unsigned long long>(), nullptr));
    unsigned long long total = 0;
    GT_HIP(hipMemcpy(&total, t->len.p + j.n, 8, hipMemcpyDeviceToHost));
    t->whole = total <= t->text_cap;
    if (!t->whole) {
        t->h_off.resize((size_t)j.n + 1);
        GT_HIP(hipMemcpy(t->h_off.data(), t->len.p, t->h_off.size() * 8, hipMemcpyDeviceToHost));
    } else t->h_off = { 0ull, total };                                 // one piece: first and last offset
    t->lines_pending = true;
    return SALT_OK;
}

// the next piece of the measured lines into the host buffer
static int gt_piece(GtText *t, const char **data, uint64_t *n_bytes, std::string &err)
{
    GtJob &j = t->job;
    uint64_t i0 = t->line_at, i1; unsigned long long bytes;
    if (t->whole) { i1 = j.n; bytes = t->h_off[1]; }
    else {
        i1 = i0;
        while (i1 < j.n && t->h_off[(size_t)i1 + 1] - t->h_off[(size_t)i0] <= t->text_cap) ++i1;      // (a single line always fits: text_cap >= max_line)
        if (i1 == i0) { err = "genotype text: a line longer than the text buffer"; return SALT_E_HIP; }
        bytes = t->h_off[(size_t)i1] - t->h_off[(size_t)i0];
    }
    hipLaunchKernelGGL(k_gt_write, dim3(tally_grid(i1 - i0)), dim3(256), 0, nullptr, j, t->len.p, i0, i1, reinterpret_cast<char *>(t->text.p));
    GT_HIP(hipGetLastError());
    t->line_at = i1;
    if (i1 == j.n) t->lines_pending = false;
    if (!t->bgzf) {
        GT_HIP(hipMemcpy(t->host, t->text.p, bytes, hipMemcpyDeviceToHost));
        *data = t->host; *n_bytes = bytes;
        return SALT_OK;
    }
    const uint64_t n_blocks = bgzf_blocks(bytes);
    GT_HIP(launch_bgzf_deflate(t->text.p, bytes, t->bz_slots.p, t->bz_sizes.p, t->bz_offs.p, t->bz_out.p, nullptr));
    unsigned long long zbytes = 0;
    GT_HIP(hipMemcpy(&zbytes, t->bz_offs.p + n_blocks, 8, hipMemcpyDeviceToHost));
    if (zbytes > bgzf_bound(bytes) || zbytes > t->host_cap) { err = "genotype text: BGZF blocks larger than their bound"; return SALT_E_HIP; }
    GT_HIP(hipMemcpy(t->host, t->bz_out.p, zbytes, hipMemcpyDeviceToHost));
    *data = t->host; *n_bytes = zbytes;
    return SALT_OK;
}

int gt_text_next(GtText *t, const char **data, uint64_t *n_bytes, std::string &err)
{
    *data = nullptr; *n_bytes = 0;
    if (!t->active) return SALT_OK;
    if (!t->lines_pending) {
        if (t->s_next >= t->n_sites) { t->active = false; return SALT_OK; }      // complete: *n_bytes == 0
        const int rc = gt_tile(t, err);
        if (rc) { t->active = false; return rc; }
    }
    const int rc = gt_piece(t, data, n_bytes, err);
    if (rc) t->active = false;
    return rc;
}

} // namespace salt
