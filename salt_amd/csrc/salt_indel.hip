// salt_amd/csrc/salt_indel.hip -- indel candidates as VCF (salt --indels; the definition is in include/salt_gpu.h).
//
// Counting: the table is 2^log2_slots slots of (key, value), a hash table of allele keys; diff is this tally's own uint32[ref_len + 1]
// difference array; stat is uint64[4].  k_indel_add runs behind the kernels that finish a batch's result rows: a thread per record walks
// the row's ops (tally_ops); every M run marks diff (tally_diff_mark), every I or D op is classified (long, unanchored, event), and an
// event is shifted left against the 2-bit genome, 16 bases a load, packed into its key and inserted: atomicCAS on the key along a linear
// probe run of at most SALT_INDEL_PROBE slots, then one 64-bit atomicAdd on the value.  Every probe step claims, matches or moves on; no
// thread waits for another, and nothing depends on which lanes are alive.  The job carries its sign in delta: 2^64 - 1 looks the keys up
// (claiming nothing) and takes a batch's adds back.  A thread sums its counters in registers and sends each on once.
// Finishing (IndelText): the slots with a non-zero value are flagged and compacted (rocprim::select), split into keys and values and sorted by key
// (rocprim::radix_sort_pairs); diff goes by in tiles of tile_positions, scanned with the carry of the tiles in front, and the keys whose
// anchor lies in the tile -- one range of the sorted keys -- gather their depth and apply the call rule; the called alleles are compacted;
// k_indel_len / scan / k_indel_write measure and write the records with one indel_line.  Records that outgrow the text buffer leave in
// several pieces, cut at line ends; with bgzf the pieces pass k_bgzf_deflate first.  Table and diff are only read.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/functional.hpp>
#include <algorithm>
#include <string>
#include <vector>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_tally.h"

namespace salt {

// letter(x) of the definition; the word of 16 bases is kept from one call to the next (at: its index, ~0 none)
struct IndelWord { uint64_t at; uint32_t v; };
__device__ __forceinline__ uint32_t indel_letter(const uint32_t *text, uint32_t text_len, uint64_t x, IndelWord &w)
{
    if (x >= text_len) return 0u;
    if ((x >> 4) != w.at) { w.at = x >> 4; w.v = text[w.at]; }
    return (w.v >> (30u - 2u * ((uint32_t)x & 15u))) & 3u;
}

// the last contig that begins at or in front of x (n >= 1)
__device__ __forceinline__ int32_t indel_contig(const int64_t *c_off, int32_t n, uint64_t x)
{
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) { const int32_t mid = (lo + hi + 1) >> 1; if (c_off[mid] >= 0 && (uint64_t)c_off[mid] <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

__device__ __forceinline__ unsigned long long indel_key(uint64_t g, bool del, uint32_t n, uint32_t bases)
{
    return 1ull << 63 | (unsigned long long)(g & 0xFFFFFFFFull) << 31 | (del ? 1ull << 30 : 0ull) | (unsigned long long)n << 24 | bases;
}

// The insert routine: true the addend went to the key's slot, false the probe run ended without one.  claim: an empty slot may be taken.
__device__ __forceinline__ bool indel_insert(IndelSlot *tab, uint32_t log2_slots, unsigned long long key, unsigned long long add, bool claim)
{
    const uint64_t slots = 1ull << log2_slots, mask = slots - 1, home = (key * 0x9E3779B97F4A7C15ull) >> (64u - log2_slots);
    const uint32_t run = slots < SALT_INDEL_PROBE ? (uint32_t)slots : SALT_INDEL_PROBE;
    for (uint32_t p = 0; p < run; ++p) {
        IndelSlot *s = tab + ((home + p) & mask);
        const unsigned long long had = claim ? atomicCAS(&s->key, 0ull, key) : __hip_atomic_load(&s->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (had == key || (claim && had == 0ull)) { atomicAdd(&s->val, add); return true; }
        if (had == 0ull) return false;                                             // (a lookup: the key was never placed behind an empty slot)
    }
    return false;
}

// One thread per record.  Loads: the row's first 24 bytes and its CIGAR words (tally_row, tally_ops), two offsets; per event the contig
// table's offsets along a binary search, the words of the 2-bit genome the shift passes, for an insertion its own bases.  Nothing is read
// beyond the read's own L codes (s + n <= L), beyond word (text_len - 1) / 16 of the genome (indel_letter) or outside the contig table,
// nothing is added to beyond diff[ref_len] (tally_diff_mark) or outside the table's slots (the probe is masked): a row the align kernels
// got wrong cannot make this kernel fault.
__global__ void __launch_bounds__(256) k_indel_add(IndelAdd c)
{
    const bool claim = (c.delta >> 63) == 0ull;
    unsigned long long n_tab = 0, n_drop = 0, n_long = 0, n_un = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.n_rec; i += (uint64_t)gridDim.x * blockDim.x) {
        const salt_result_t *q = c.res + i;
        const TallyRow r = tally_row(q, c.pe, c.min_mapq);
        if (r.fate != TALLY_COUNTED) continue;
        const uint32_t o0 = c.offs[i], L = c.offs[i + 1] - o0;
        const uint8_t *sq = c.seqs + o0;
        tally_ops(q, r,
            [&](uint64_t g, uint32_t, uint32_t len) { tally_diff_mark(c.diff, c.ref_len, g, len, (uint32_t)c.delta); },
            [&](uint32_t what, uint32_t n, uint64_t g, uint32_t s, uint32_t prev, uint32_t next) {
                const bool del = what == 2u;
                if (n < 1u || n > (del ? SALT_INDEL_MAX_DEL : SALT_INDEL_MAX_INS)) { ++n_long; return; }
                bool ok = (prev & 3u) == 0u && (prev >> 4) >= 1u && (next & 3u) == 0u && (next >> 4) >= 1u && g >= 1u;      // (g >= 1 follows from the M op in front)
                int32_t ct = 0; uint64_t first = 0;
                if (ok) {
                    ct = indel_contig(c.c_off, c.n_contigs, g - 1);
                    first = c.c_off[ct] > 0 ? (uint64_t)c.c_off[ct] : 0ull;
                    uint64_t end = ct + 1 < c.n_contigs && c.c_off[ct + 1] >= 0 ? (uint64_t)c.c_off[ct + 1] : (uint64_t)c.ref_len;
                    if (end > c.ref_len) end = c.ref_len;                          // (a contig table that leaves the genome)
                    ok = g < end && (!del || g + n <= end);
                }
                uint32_t b = 0;                                                    // the inserted bases, b[0] highest, left-justified in 24 bits
                if (ok && !del) {
                    ok = (uint64_t)s + n <= L;
                    for (uint32_t j = 0; ok && j < n; ++j) {
                        const uint32_t x = s + j;
                        uint32_t code = r.rev ? sq[L - 1u - x] : sq[x];
                        if (code > 3u) { ok = false; break; }
                        if (r.rev) code = 3u - code;
                        b |= code << (22u - 2u * j);
                    }
                }
                if (!ok) { ++n_un; return; }
                IndelWord lo{ ~0ull, 0u }, hi{ ~0ull, 0u };
                const uint32_t keep = del ? 0u : ((1u << (2u * n)) - 1u) << (24u - 2u * n);
                for (uint32_t step = 0; step < SALT_INDEL_MAX_SHIFT && g - 1 > first; ++step) {
                    const uint32_t a = indel_letter(c.text, c.text_len, g - 1, lo);
                    if (del) { if (a != indel_letter(c.text, c.text_len, g + n - 1, hi)) break; }
                    else {
                        if (a != ((b >> (24u - 2u * n)) & 3u)) break;
                        b = (a << 22 | b >> 2) & keep;
                    }
                    --g;
                }
                const unsigned long long add = (r.rev ? 1ull << 32 : 1ull) * c.delta;
                if (indel_insert(c.tab, c.log2_slots, indel_key(g, del, n, b), add, claim)) ++n_tab; else ++n_drop;
            });
    }
    if (n_tab) atomicAdd(c.stat + SALT_INDEL_TABLED, n_tab * c.delta);
    if (n_drop) atomicAdd(c.stat + SALT_INDEL_DROPPED, n_drop * c.delta);
    if (n_long) atomicAdd(c.stat + SALT_INDEL_LONG, n_long * c.delta);
    if (n_un) atomicAdd(c.stat + SALT_INDEL_UNANCHORED, n_un * c.delta);
}

hipError_t launch_indel_add(const IndelAdd &c, hipStream_t st)
{
    if (c.n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(k_indel_add, dim3(tally_grid(c.n_rec)), dim3(256), 0, st, c);
    return hipGetLastError();
}

// pairs[2 i], pairs[2 i + 1] = key, value: the value is the addend, the sum of its halves the events; a key of 0 names no allele and is passed over
__global__ void __launch_bounds__(256) k_indel_put(const unsigned long long *__restrict__ pairs, uint64_t n, IndelSlot *tab, uint32_t log2_slots, unsigned long long *stat)
{
    unsigned long long n_tab = 0, n_drop = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = pairs[2 * i], val = pairs[2 * i + 1], ev = (val & 0xFFFFFFFFull) + (val >> 32);
        if (key == 0ull || val == 0ull) continue;
        if (indel_insert(tab, log2_slots, key, val, true)) n_tab += ev; else n_drop += ev;
    }
    if (n_tab) atomicAdd(stat + SALT_INDEL_TABLED, n_tab);
    if (n_drop) atomicAdd(stat + SALT_INDEL_DROPPED, n_drop);
}

hipError_t launch_indel_put(const unsigned long long *pairs, uint64_t n, IndelSlot *tab, uint32_t log2_slots, unsigned long long *stat, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_indel_put, dim3(tally_grid(n)), dim3(256), 0, st, pairs, n, tab, log2_slots, stat);
    return hipGetLastError();
}

// ---- finishing ----
// live[i] = slot i has a non-zero value, and their number: what is compacted is what was counted, whatever is added to the table meanwhile
__global__ void __launch_bounds__(256) k_indel_live(const IndelSlot *__restrict__ tab, uint64_t slots, uint8_t *__restrict__ live, unsigned long long *n)
{
    unsigned long long k = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x) { const bool on = tab[i].val != 0ull; live[i] = on; k += on; }
    if (k) atomicAdd(n, k);
}
__global__ void __launch_bounds__(256) k_indel_split(const IndelSlot *__restrict__ in, uint64_t n, unsigned long long *__restrict__ keys, unsigned long long *__restrict__ vals)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) { keys[i] = in[i].key; vals[i] = in[i].val; }
}

// What the tile and line kernels read (by value).  A tile is positions [t0, t0 + n_pos) of diff; depth[t0 + i] = dep[i] + carry; the keys
// whose anchor lies in it are [k0, k1).
struct IndelJob {
    const unsigned long long *keys, *vals; uint64_t n_keys;
    const uint32_t *dep; uint32_t *depth; uint8_t *flag; uint32_t t0, n_pos, carry; uint64_t k0, k1;
    const uint32_t *text; uint32_t ref_len, text_len;
    const int64_t *c_off; const uint32_t *c_name_off; const char *c_names; int32_t n_contigs;
    uint32_t min_alt, min_pct;
    const uint32_t *cand; uint64_t n_lines;                                        // line i is key cand[i]
};

__device__ __forceinline__ uint64_t indel_key_g(unsigned long long key) { return (key >> 31) & 0xFFFFFFFFull; }
__device__ __forceinline__ bool indel_well_formed(unsigned long long key, uint32_t ref_len)
{
    const uint64_t g = indel_key_g(key);
    const uint32_t n = (uint32_t)(key >> 24) & 63u, b = (uint32_t)key & 0xFFFFFFu;
    const bool del = (key >> 30) & 1ull;
    if (!(key >> 63) || g < 1u || g > ref_len || n < 1u) return false;
    return del ? b == 0u : n <= SALT_INDEL_MAX_INS && (b & ((1u << (24u - 2u * n)) - 1u)) == 0u;
}

// bound[0] = the first key whose g is at least g_min (all keys: n_keys); one thread
__global__ void k_indel_bound(const unsigned long long *__restrict__ keys, uint64_t n_keys, uint64_t g_min, unsigned long long *bound)
{
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long want = g_min > 0xFFFFFFFFull ? ~0ull : (1ull << 63 | (unsigned long long)g_min << 31);
    uint64_t lo = 0, hi = n_keys;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (keys[mid] < want) lo = mid + 1; else hi = mid; }
    if (g_min > 0xFFFFFFFFull) lo = n_keys;
    bound[0] = lo;
}

// the tile's keys: their depth and whether they are called
__global__ void __launch_bounds__(256) k_indel_depth(IndelJob j)
{
    for (uint64_t i = j.k0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < j.k1; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = j.keys[i], v = j.vals[i];
        const uint64_t a = indel_key_g(key) - 1;                                   // (the range holds keys with t0 + 1 <= g <= t0 + n_pos only; checked again)
        if (!indel_well_formed(key, j.ref_len) || a < j.t0 || a - j.t0 >= j.n_pos) { j.flag[i] = 0; continue; }
        const uint32_t depth = j.dep[a - j.t0] + j.carry;
        const unsigned long long ao = (v & 0xFFFFFFFFull) + (v >> 32);
        j.depth[i] = depth;
        j.flag[i] = ao >= j.min_alt && 100ull * ao >= (unsigned long long)j.min_pct * depth;
    }
}

// Counts the bytes of a line, or writes them: the same code measures and writes, so the two cannot disagree.
struct IndelEmit {
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

// the record of called allele i (a well-formed key: k_indel_depth flags no other)
__device__ __forceinline__ void indel_line(const IndelJob &j, uint64_t i, IndelEmit &o)
{
    const uint32_t at = j.cand[i];
    const unsigned long long key = j.keys[at], v = j.vals[at];
    const uint64_t g = indel_key_g(key), a = g - 1;
    const uint32_t n = (uint32_t)(key >> 24) & 63u, b = (uint32_t)key & 0xFFFFFFu;
    const bool del = (key >> 30) & 1ull;
    const int32_t ct = indel_contig(j.c_off, j.n_contigs, a);
    const char NT[4] = { 'A', 'C', 'G', 'T' };
    IndelWord w{ ~0ull, 0u };
    for (uint32_t x = j.c_name_off[ct]; x < j.c_name_off[ct + 1]; ++x) o.put(j.c_names[x]);
    o.put('\t'); o.putu(a - (uint64_t)j.c_off[ct] + 1u); o.put('\t'); o.put('.'); o.put('\t');
    const char anchor = NT[indel_letter(j.text, j.text_len, a, w)];
    o.put(anchor);
    if (del) for (uint32_t k = 0; k < n; ++k) o.put(NT[indel_letter(j.text, j.text_len, g + k, w)]);
    o.put('\t'); o.put(anchor);
    if (!del) for (uint32_t k = 0; k < n; ++k) o.put(NT[(b >> (22u - 2u * k)) & 3u]);
    const uint64_t fwd = v & 0xFFFFFFFFull, rev = v >> 32;
    o.puts("\t.\t.\tTYPE="); o.puts(del ? "DEL" : "INS"); o.puts(";LEN="); o.putu(n); o.puts(";DP="); o.putu(j.depth[at]);
    o.puts(";AO="); o.putu(fwd + rev); o.puts(";AOF="); o.putu(fwd); o.puts(";AOR="); o.putu(rev); o.put('\n');
}

// len[i] = bytes of line i; len[n_lines] = 0 (the scan's last entry: all bytes)
__global__ void __launch_bounds__(256) k_indel_len(IndelJob j, unsigned long long *__restrict__ len)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < j.n_lines; i += (uint64_t)gridDim.x * blockDim.x) {
        IndelEmit o{ nullptr, 0 };
        indel_line(j, i, o);
        len[i] = o.n;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[j.n_lines] = 0;
}
// lines [i0, i1) to out + off[i] - off[i0]
__global__ void __launch_bounds__(256) k_indel_write(IndelJob j, const unsigned long long *__restrict__ off, uint64_t i0, uint64_t i1, char *__restrict__ out)
{
    for (uint64_t i = i0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * blockDim.x) {
        IndelEmit o{ out + (off[i] - off[i0]), 0 };
        indel_line(j, i, o);
    }
}

namespace {
template <class T> struct Dev {                                        // a device buffer freed with its owner
    T *p = nullptr; uint64_t cap = 0;
    Dev() = default; Dev(const Dev &) = delete; Dev &operator=(const Dev &) = delete;
    ~Dev() { if (p) hipFree(p); }
    hipError_t alloc(uint64_t n) { if (p) hipFree(p); p = nullptr; cap = 0; const hipError_t e = hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)); if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); } else cap = n ? n : 1; return e; }
    hipError_t reserve(uint64_t n) { return n <= cap && p ? hipSuccess : alloc(n); }      // (the contents are not kept)
};
}

struct IndelText {
    IndelJob job{};
    // the sorted live slots
    Dev<unsigned long long> cnt, keys, vals, keys2, vals2; Dev<IndelSlot> live; Dev<uint8_t> tmp, live_flag;
    uint64_t n_keys = 0;
    // the text
    uint32_t ref_len = 0; bool bgzf = false;
    uint64_t buf_tile = 0, text_cap = 0;
    Dev<uint32_t> dep, depth, cand, cand_n; Dev<uint8_t> flag, text, tmp2; Dev<unsigned long long> len;
    Dev<uint32_t> bz_slots, bz_sizes; Dev<unsigned long long> bz_offs; Dev<uint8_t> bz_out;
    char *host = nullptr; uint64_t host_cap = 0;
    bool active = false, whole = false;
    std::vector<unsigned long long> h_off; uint64_t line_at = 0;
    ~IndelText() { if (host) hipHostFree(host); }
};

IndelText *indel_text_new() { return new IndelText; }
void indel_text_free(IndelText *t) { delete t; }

#define IC_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string("indel text: " #x ": ") + hipGetErrorString(e_); return SALT_E_HIP; } } while (0)
#define IC_ROOM(x, what) do { if ((x) != hipSuccess) { err = std::string("indel text: no room for ") + what; return SALT_E_NOMEM; } } while (0)

static const uint32_t INDEL_TILE_DEFAULT = 1u << 22, INDEL_TILE_MAX = 1u << 26;
static const uint64_t INDEL_TEXT_BYTES = 4u << 20;

int indel_sorted(IndelText *t, const IndelSlot *d_tab, uint32_t log2_slots, uint64_t *n_out, const unsigned long long **d_keys, const unsigned long long **d_vals, std::string &err)
{
    const uint64_t slots = 1ull << log2_slots;
    t->n_keys = 0; t->active = false;
    IC_ROOM(t->cnt.reserve(2), "two counters");
    IC_ROOM(t->live_flag.reserve(slots), "a byte per slot: " + std::to_string(slots) + " bytes");
    IC_HIP(hipMemset(t->cnt.p, 0, 16));
    hipLaunchKernelGGL(k_indel_live, dim3(tally_grid(slots)), dim3(256), 0, nullptr, d_tab, slots, t->live_flag.p, t->cnt.p);
    IC_HIP(hipGetLastError());
    unsigned long long n = 0;
    IC_HIP(hipMemcpy(&n, t->cnt.p, 8, hipMemcpyDeviceToHost));
    if (n > slots) { err = "indel text: more live slots than slots"; return SALT_E_HIP; }
    *n_out = n; *d_keys = nullptr; *d_vals = nullptr;
    if (n == 0) return SALT_OK;
    const std::string room = "the " + std::to_string(n) + " live slots and their sort: about " + std::to_string(n * 48) + " bytes";
    IC_ROOM(t->live.reserve(n), room); IC_ROOM(t->keys.reserve(n), room); IC_ROOM(t->vals.reserve(n), room); IC_ROOM(t->keys2.reserve(n), room); IC_ROOM(t->vals2.reserve(n), room);
    size_t b_sel = 0, b_sort = 0;
    IC_HIP(rocprim::select(nullptr, b_sel, d_tab, t->live_flag.p, t->live.p, t->cnt.p + 1, (size_t)slots, (hipStream_t) nullptr));
    IC_HIP(rocprim::radix_sort_pairs(nullptr, b_sort, t->keys.p, t->keys2.p, t->vals.p, t->vals2.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
    IC_ROOM(t->tmp.reserve(std::max(b_sel, b_sort)), "the scratch of the select and the sort");
    IC_HIP(rocprim::select(t->tmp.p, b_sel, d_tab, t->live_flag.p, t->live.p, t->cnt.p + 1, (size_t)slots, (hipStream_t) nullptr));
    unsigned long long n2 = 0;
    IC_HIP(hipMemcpy(&n2, t->cnt.p + 1, 8, hipMemcpyDeviceToHost));
    if (n2 != n) { err = "indel text: the select kept " + std::to_string(n2) + " slots of " + std::to_string(n) + " flagged"; return SALT_E_HIP; }
    hipLaunchKernelGGL(k_indel_split, dim3(tally_grid(n)), dim3(256), 0, nullptr, t->live.p, (uint64_t)n, t->keys.p, t->vals.p);
    IC_HIP(hipGetLastError());
    IC_HIP(rocprim::radix_sort_pairs(t->tmp.p, b_sort, t->keys.p, t->keys2.p, t->vals.p, t->vals2.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
    IC_HIP(hipDeviceSynchronize());
    t->n_keys = n; *d_keys = t->keys2.p; *d_vals = t->vals2.p;
    return SALT_OK;
}

int indel_text_begin(IndelText *t, const IndelSlot *d_tab, uint32_t log2_slots, const uint32_t *d_diff, const uint32_t *d_text, uint32_t ref_len, uint32_t text_len,
                     const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names, int32_t n_contigs, uint32_t max_name,
                     uint32_t min_alt, uint32_t min_pct, uint32_t tile_positions, int bgzf, std::string &err)
{
    uint64_t n_keys = 0; const unsigned long long *keys = nullptr, *vals = nullptr;
    if (const int rc = indel_sorted(t, d_tab, log2_slots, &n_keys, &keys, &vals, err)) return rc;
    t->ref_len = ref_len; t->bgzf = bgzf != 0; t->line_at = 0; t->h_off.clear();
    IndelJob &j = t->job;
    j = IndelJob{};
    if (n_keys == 0) { t->active = true; return SALT_OK; }              // (no line: the first next is complete)
    if (n_keys > 0xFFFFFFFFull) { err = "indel text: more than 2^32 - 1 live slots"; return SALT_E_INVAL; }
    uint64_t tile = tile_positions ? tile_positions : INDEL_TILE_DEFAULT;
    if (tile > INDEL_TILE_MAX) tile = INDEL_TILE_MAX;
    if (tile > ref_len) tile = ref_len;
    // name, POS of ten digits, REF of up to 64 letters, ALT of up to 13, seven tabs, three dots, the INFO field's 37 letters and five numbers of up to eleven digits, newline
    const uint64_t max_line = (uint64_t)max_name + 256, text_cap = INDEL_TEXT_BYTES + max_line;
    size_t b_scan = 0, b_sel = 0, b_len = 0;
    {
        uint32_t *u = nullptr; uint8_t *f = nullptr; unsigned long long *l = nullptr;
        IC_HIP(rocprim::inclusive_scan(nullptr, b_scan, u, u, (size_t)tile, rocprim::plus<uint32_t>(), nullptr));
        IC_HIP(rocprim::select(nullptr, b_sel, rocprim::counting_iterator<uint32_t>(0), f, u, u, (size_t)n_keys, (hipStream_t) nullptr));
        IC_HIP(rocprim::exclusive_scan(nullptr, b_len, l, l, 0ull, (size_t)n_keys + 1, rocprim::plus<unsigned long long>(), nullptr));
    }
    const size_t tmp_bytes = std::max(b_scan, std::max(b_sel, b_len));
    const uint64_t n_blocks = bgzf_blocks(text_cap);
    const std::string room = "the buffers of " + std::to_string(n_keys) + " alleles and a tile of " + std::to_string(tile) + " positions";
    IC_ROOM(t->dep.reserve(tile), room); IC_ROOM(t->depth.reserve(n_keys), room); IC_ROOM(t->flag.reserve(n_keys), room); IC_ROOM(t->cand.reserve(n_keys), room);
    IC_ROOM(t->cand_n.reserve(4), room); IC_ROOM(t->len.reserve(n_keys + 1), room); IC_ROOM(t->tmp2.reserve(tmp_bytes), room); IC_ROOM(t->text.reserve(text_cap + 64), room);
    IC_ROOM(t->bz_slots.reserve(n_blocks * (BGZF_SLOT_BYTES / 4)), room); IC_ROOM(t->bz_sizes.reserve(n_blocks), room); IC_ROOM(t->bz_offs.reserve(n_blocks + 1), room);
    IC_ROOM(t->bz_out.reserve(n_blocks * (BGZF_CUT_BYTES + 31)), room);
    const uint64_t host_cap = std::max<uint64_t>(text_cap, bgzf_bound(text_cap));
    if (host_cap != t->host_cap) {
        if (t->host) { hipHostFree(t->host); t->host = nullptr; t->host_cap = 0; }
        IC_HIP(hipHostMalloc((void **)&t->host, host_cap, hipHostMallocDefault));
        t->host_cap = host_cap;
    }
    t->text_cap = text_cap;
    j.keys = keys; j.vals = vals; j.n_keys = n_keys; j.dep = t->dep.p; j.depth = t->depth.p; j.flag = t->flag.p;
    j.text = d_text; j.ref_len = ref_len; j.text_len = text_len;
    j.c_off = d_c_off; j.c_name_off = d_c_name_off; j.c_names = d_c_names; j.n_contigs = n_contigs;
    j.min_alt = min_alt; j.min_pct = min_pct; j.cand = t->cand.p;
    IC_HIP(hipMemset(t->flag.p, 0, n_keys));                           // keys whose anchor lies in no tile (no well-formed key) are never called
    IC_HIP(hipMemset(t->depth.p, 0, n_keys * 4));
    // the tiles of diff, in genome order, with the carry of those in front; a tile's keys are those with t0 + 1 <= g <= t0 + n
    unsigned long long k0 = 0, k1 = 0; uint32_t carry = 0;
    hipLaunchKernelGGL(k_indel_bound, dim3(1), dim3(1), 0, nullptr, keys, n_keys, (uint64_t)1, t->cnt.p);
    IC_HIP(hipGetLastError());
    IC_HIP(hipMemcpy(&k0, t->cnt.p, 8, hipMemcpyDeviceToHost));
    for (uint64_t g0 = 0; g0 < ref_len && k0 < n_keys; ) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(tile, (uint64_t)ref_len - g0);
        hipLaunchKernelGGL(k_indel_bound, dim3(1), dim3(1), 0, nullptr, keys, n_keys, g0 + n + 1, t->cnt.p);
        IC_HIP(hipGetLastError());
        IC_HIP(rocprim::inclusive_scan(t->tmp2.p, b_scan, d_diff + g0, t->dep.p, (size_t)n, rocprim::plus<uint32_t>(), nullptr));
        uint32_t last = 0;
        IC_HIP(hipMemcpy(&k1, t->cnt.p, 8, hipMemcpyDeviceToHost));
        IC_HIP(hipMemcpy(&last, t->dep.p + (n - 1), 4, hipMemcpyDeviceToHost));
        if (k1 < k0 || k1 > n_keys) { err = "indel text: the sorted keys are out of order"; return SALT_E_HIP; }
        if (k1 > k0) {
            j.t0 = (uint32_t)g0; j.n_pos = n; j.carry = carry; j.k0 = k0; j.k1 = k1;
            hipLaunchKernelGGL(k_indel_depth, dim3(tally_grid(k1 - k0)), dim3(256), 0, nullptr, j);
            IC_HIP(hipGetLastError());                                 // (dep is the next tile's too: one stream)
        }
        carry += last; g0 += n; k0 = k1;
    }
    // the called alleles, their lines' lengths, scanned
    uint32_t count = 0;
    IC_HIP(rocprim::select(t->tmp2.p, b_sel, rocprim::counting_iterator<uint32_t>(0), t->flag.p, t->cand.p, t->cand_n.p, (size_t)n_keys, (hipStream_t) nullptr));
    IC_HIP(hipMemcpy(&count, t->cand_n.p, 4, hipMemcpyDeviceToHost));
    if (count > n_keys) { err = "indel text: more called alleles than alleles"; return SALT_E_HIP; }
    j.n_lines = count;
    t->active = true;
    if (count == 0) return SALT_OK;
    hipLaunchKernelGGL(k_indel_len, dim3(tally_grid(count)), dim3(256), 0, nullptr, j, t->len.p);
    IC_HIP(hipGetLastError());
    IC_HIP(rocprim::exclusive_scan(t->tmp2.p, b_len, t->len.p, t->len.p, 0ull, (size_t)count + 1, rocprim::plus<unsigned long long>(), nullptr));
    unsigned long long total = 0;
    IC_HIP(hipMemcpy(&total, t->len.p + count, 8, hipMemcpyDeviceToHost));
    t->whole = total <= t->text_cap;
    if (!t->whole) {
        t->h_off.resize((size_t)count + 1);
        IC_HIP(hipMemcpy(t->h_off.data(), t->len.p, t->h_off.size() * 8, hipMemcpyDeviceToHost));
    } else t->h_off = { 0ull, total };                                 // one piece: first and last offset
    return SALT_OK;
}

// the next piece of the measured lines into the host buffer; *n_bytes == 0: complete
int indel_text_next(IndelText *t, const char **data, uint64_t *n_bytes, std::string &err)
{
    *data = nullptr; *n_bytes = 0;
    if (!t->active) return SALT_OK;
    IndelJob &j = t->job;
    if (t->line_at >= j.n_lines) { t->active = false; return SALT_OK; }
    uint64_t i0 = t->line_at, i1; unsigned long long bytes;
    if (t->whole) { i1 = j.n_lines; bytes = t->h_off[1]; }
    else {
        i1 = i0;
        while (i1 < j.n_lines && t->h_off[(size_t)i1 + 1] - t->h_off[(size_t)i0] <= t->text_cap) ++i1;      // (a single line always fits: text_cap >= max_line)
        if (i1 == i0) { t->active = false; err = "indel text: a line longer than the text buffer"; return SALT_E_HIP; }
        bytes = t->h_off[(size_t)i1] - t->h_off[(size_t)i0];
    }
    if (bytes == 0 || bytes > t->text_cap) { t->active = false; err = "indel text: a piece of " + std::to_string(bytes) + " bytes"; return SALT_E_HIP; }
    t->active = false;                                                 // (an error below ends the text)
    hipLaunchKernelGGL(k_indel_write, dim3(tally_grid(i1 - i0)), dim3(256), 0, nullptr, j, t->len.p, i0, i1, reinterpret_cast<char *>(t->text.p));
    IC_HIP(hipGetLastError());
    t->line_at = i1;
    if (!t->bgzf) {
        IC_HIP(hipMemcpy(t->host, t->text.p, bytes, hipMemcpyDeviceToHost));
        *data = t->host; *n_bytes = bytes; t->active = true;
        return SALT_OK;
    }
    const uint64_t n_blocks = bgzf_blocks(bytes);
    IC_HIP(launch_bgzf_deflate(t->text.p, bytes, t->bz_slots.p, t->bz_sizes.p, t->bz_offs.p, t->bz_out.p, nullptr));
    unsigned long long zbytes = 0;
    IC_HIP(hipMemcpy(&zbytes, t->bz_offs.p + n_blocks, 8, hipMemcpyDeviceToHost));
    if (zbytes > bgzf_bound(bytes) || zbytes > t->host_cap) { err = "indel text: BGZF blocks larger than their bound"; return SALT_E_HIP; }
    IC_HIP(hipMemcpy(t->host, t->bz_out.p, zbytes, hipMemcpyDeviceToHost));
    *data = t->host; *n_bytes = zbytes; t->active = true;
    return SALT_OK;
}

} // namespace salt
