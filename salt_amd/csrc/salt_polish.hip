// salt_amd/csrc/salt_polish.hip -- `polish` over SAM text on the device (gfx950): record lines in, polished record lines out.
//
// The reference's post-processor (Polish_src/polish.c, samParser.c) reads, parses, scores, picks and prints a record at a time on the
// host.  Here a block of record lines goes through plain grid-stride kernels, work handed over at kernel boundaries only:
//   k_fq_count / k_fq_lines   (salt_text.hip) newline scan -> start of every line
//   k_pl_stop                 the first empty line (it ends the input, samParser.c:87-90)
//   k_pl_count                a thread per record: the strtok field rules, hits per strand as parsed, l_seq, the malformed-record status
//   k_pl_fill                 a thread per record: hits into the record's span of the global hit array (contig names looked up in the
//                             sorted table), offset sort, rm_repeat_hits, the window rule's checks and counts, the read's codes as sequenced
//   k_pl_items                a thread per record: one salt_polish_item_t per unique hit; clipped Landau-Vishkin windows into the pool
//   k_pl_swreq / k_pl_swscore items -> PeSwReq (scoring mode 2), PeSwRes -> scores (-s)
//   k_polish / k_sw*          (salt_align.hip, salt_pe.hip) every edit distance / Smith-Waterman score, then the winners' CIGARs
//   k_pl_pick                 a thread per record or pair: scores into the hits, winners, the pairing walk (it swaps hits in place) and
//                             the pair choice; one CIGAR item per winner
//   k_pl_len / k_pl_write     a thread per record: the exact length, a scan, the bytes (polish_sam_se / polish_sam_pe)
// `salt --polish` (salt_gpu_ws_set_polish) has no text to start from: k_pl_rows stands where the first five kernels stand and fills the same
// PlRec / PlHit arrays from the aligner's result rows (the fused route, at the end of this file); everything from k_pl_items on is one
// tail for both (pl_tail_len / pl_tail_write).
// The per-record rules themselves are in salt_polish_text.h, which the host compiles too.  Between the stages the host reads a few
// count words back (lines, hits, items, CIGAR items, bytes) to size the next stage's buffers; the buffers stay with the handle.
// Errors: every stage reports the smallest record index it refuses, and the call returns at the first stage that refuses one -- a
// 10-field record found by k_pl_count is reported before an unknown contig in an earlier record, which k_pl_fill would find.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "salt_device.h"
#include "salt_kernels.h"
#include "salt_polish_text.h"

namespace salt {
using namespace salt_pl;

static inline uint32_t pgrid(uint64_t n) { uint64_t b = (n + 127) / 128; if (b > (1u << 16)) b = 1u << 16; return b ? (uint32_t)b : 1u; }
#define PSTRIDE(i, n) for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, s_ = (uint64_t)gridDim.x * blockDim.x; i < (n); i += s_)

// control words of a block (64-bit each, zeroed / preset per call)
enum { C_STOP, C_ERR, C_MAXLEN, C_NCLIP, C_NCIG, C_PROPER, C_BYTES, C_N };
struct PlRec { PlFields f; uint32_t line_b, line_e, nh[2], nu[2], bad_b, bad_e, cit, proper, dead; PlWin w; };      // dead: a slot without a record (k_pl_rows)

__device__ __forceinline__ void pl_fail(unsigned long long *ctl, uint64_t rec, int code) { atomicMin(ctl + C_ERR, (unsigned long long)(rec << 8 | (uint64_t)code)); }

__global__ void __launch_bounds__(128) k_pl_stop(const uint32_t *__restrict__ line_start, uint32_t n_lines, unsigned long long *__restrict__ ctl)
{
    PSTRIDE(i, n_lines) if (line_start[i + 1] - 1 == line_start[i]) atomicMin(ctl + C_STOP, (unsigned long long)i);
}

__device__ __forceinline__ uint32_t pl_n_rec(const unsigned long long *ctl, uint32_t n_lines, int paired)
{
    uint32_t n = ctl[C_STOP] < n_lines ? (uint32_t)ctl[C_STOP] : n_lines;
    if (paired) n &= ~1u;                                        // a last record without its mate is dropped (polish.c:455-456, 652-653)
    return n;
}

__global__ void __launch_bounds__(128) k_pl_count(const uint8_t *__restrict__ raw, const uint32_t *__restrict__ line_start, uint32_t n_lines, int paired,
                                                   unsigned long long *__restrict__ ctl, PlRec *__restrict__ rec, uint32_t *__restrict__ hcount, uint32_t *__restrict__ lseq)
{
    const uint32_t n_rec = pl_n_rec(ctl, n_lines, paired);
    PSTRIDE(i, n_lines) {
        uint32_t nh[2] = { 0, 0 }, L = 0;
        if (i < n_rec) {
            PlRec r;
            r.f.name_off = r.f.name_len = r.f.chrom_off = r.f.chrom_len = r.f.seq_off = r.f.qual_off = r.f.qual_len = r.f.pos = 0; r.f.flag = 0;
            r.line_b = line_start[i]; r.line_e = line_start[i + 1] - 1;
            r.nu[0] = r.nu[1] = r.bad_b = r.bad_e = r.proper = r.dead = 0; r.cit = 0xFFFFFFFFu; r.w.strand = r.w.primary = -1; r.w.b0 = r.w.b1 = PL_UNMAPPED;
            if (!pl_parse(raw, r.line_b, r.line_e, r.f)) { pl_fail(ctl, i, PL_E_FIELDS); r.f.l_seq = 0; r.f.has_primary = 0; r.f.xa_off = r.f.xa_end = 0; }
            else if (r.f.l_seq == 0 || r.f.l_seq > PL_MAX_READ) { pl_fail(ctl, i, PL_E_LEN); r.f.l_seq = 0; r.f.has_primary = 0; r.f.xa_off = r.f.xa_end = 0; }
            else {
                PlContigs none; none.n = 0; none.off = nullptr; none.name_off = nullptr; none.names = nullptr;
                uint32_t bb = 0, be = 0;
                pl_hits(raw, r.f, none, false, (PlHit *)nullptr, (PlHit *)nullptr, nh, bb, be);
                L = r.f.l_seq;
                atomicMax(ctl + C_MAXLEN, (unsigned long long)L);
            }
            r.nh[0] = nh[0]; r.nh[1] = nh[1];
            rec[i] = r;
        }
        hcount[i] = nh[0] + nh[1]; lseq[i] = L;
    }
}

struct PlDev {                                                  // what the per-record kernels read (by value)
    const uint8_t *raw; PlRec *rec; uint32_t n_rec; PlHit *hits; const uint32_t *hbase, *offs; uint8_t *codes;
    PlContigs ct; const uint8_t *pac; unsigned long long l_pac; int use_sw, paired;
    uint32_t *nuc, *nclip; const uint32_t *ibase, *pbase; salt_polish_item_t *items; uint8_t *pool;
    const int32_t *dist; salt_polish_item_t *citems;
    const int32_t *cdist; const uint16_t *ccig; const uint8_t *cnc; const PeSwRes *cres;
    unsigned long long *ctl;
    int qual_seq;                                               // the fused route: QUAL in d.raw is as sequenced (PlOut.qual_seq)
};

__global__ void __launch_bounds__(128) k_pl_fill(PlDev d)
{
    PSTRIDE(i, d.n_rec) {
        PlRec r = d.rec[i];
        PlHit *h0 = d.hits + d.hbase[i], *h1 = h0 + r.nh[0];
        uint32_t nh[2], n_clip = 0;
        if (!pl_hits(d.raw, r.f, d.ct, true, h0, h1, nh, r.bad_b, r.bad_e)) { pl_fail(d.ctl, i, PL_E_CONTIG); r.nu[0] = r.nu[1] = 0; }
        else {
            r.nu[0] = pl_sort_unique(h0, r.nh[0]); r.nu[1] = pl_sort_unique(h1, r.nh[1]);
            const int st = pl_windows<salt_polish_item_t>((uint32_t)i, r.f.l_seq, d.l_pac, d.use_sw != 0, h0, r.nu[0], h1, r.nu[1], d.pac, nullptr, nullptr, 0, n_clip);
            if (st) { pl_fail(d.ctl, i, st); r.nu[0] = r.nu[1] = 0; n_clip = 0; }
        }
        pl_codes(d.raw, r.f, d.codes + d.offs[i]);
        d.rec[i] = r;
        d.nuc[i] = r.nu[0] + r.nu[1]; d.nclip[i] = d.use_sw ? 0u : n_clip;
        if (n_clip) atomicAdd(d.ctl + C_NCLIP, (unsigned long long)n_clip);
    }
}

__global__ void __launch_bounds__(128) k_pl_items(PlDev d)
{
    PSTRIDE(i, d.n_rec) {
        const PlRec r = d.rec[i];
        if (r.nu[0] + r.nu[1] == 0) continue;
        const PlHit *h0 = d.hits + d.hbase[i], *h1 = h0 + r.nh[0];
        uint32_t n_clip = 0;
        pl_windows<salt_polish_item_t>((uint32_t)i, r.f.l_seq, d.l_pac, d.use_sw != 0, h0, r.nu[0], h1, r.nu[1], d.pac, d.items + d.ibase[i], d.pool, d.pbase[i], n_clip);
    }
}

__global__ void __launch_bounds__(128) k_pl_swreq(const salt_polish_item_t *__restrict__ items, uint32_t n, int score_only, PeSwReq *__restrict__ req)
{
    PSTRIDE(i, n) {
        const salt_polish_item_t x = items[i];
        PeSwReq q; q.start = x.offset; q.end = x.offset + x.tlen - 1u; q.mate = x.read; q.strand = (uint8_t)(x.strand ? 1 : 0); q.aware = 2; q.pad = (uint16_t)(score_only ? 1 : 0);
        req[i] = q;
    }
}
__global__ void __launch_bounds__(128) k_pl_swscore(const PeSwRes *__restrict__ res, uint32_t n, int32_t *__restrict__ dist)
{
    PSTRIDE(i, n) dist[i] = res[i].score1;
}

// scores into the record's hits: item ibase + j is unique hit j (forward strand first)
__device__ __forceinline__ void pl_scores(const PlDev &d, uint32_t i, const PlRec &r, PlHit *h0, PlHit *h1)
{
    const int32_t *ds = d.dist + d.ibase[i];
    for (uint32_t j = 0; j < r.nu[0]; ++j) { const int32_t v = ds[j]; h0[j].score = d.use_sw ? v : (v == -1 ? PL_UNMAPPED : -v); }
    for (uint32_t j = 0; j < r.nu[1]; ++j) { const int32_t v = ds[r.nu[0] + j]; h1[j].score = d.use_sw ? v : (v == -1 ? PL_UNMAPPED : -v); }
}
// the winner's CIGAR item (gen_cigar, polish.c:190-249): a fresh window of l_seq bases, k = the winner's distance
__device__ __forceinline__ void pl_cigar_item(const PlDev &d, uint32_t i, PlRec &r, const PlHit *h0, const PlHit *h1)
{
    if (r.w.strand == -1 || r.w.primary == -1) return;
    const PlHit x = (r.w.strand ? h1 : h0)[r.w.primary];
    if (!d.use_sw && x.score == -PL_MAX_DISTANCE) return;        // "*" (polish.c:231-233)
    // a guard: pl_pick and pl_pick_pair never choose a hit (a pair sum) at or below PL_UNMAPPED, so no input reaches this today; the host path
    // has the same check in front of its CIGAR call
    if (!d.use_sw && x.score == PL_UNMAPPED) { pl_fail(d.ctl, i, PL_E_NOALN); return; }
    salt_polish_item_t it; it.read = i; it.offset = x.offset; it.pool = 0xFFFFFFFFu; it.strand = (uint8_t)r.w.strand; it.k = d.use_sw ? (uint8_t)0 : (uint8_t)(-x.score);
    uint32_t l_ref = r.f.l_seq;
    if ((uint64_t)x.offset + l_ref > d.l_pac) l_ref = (uint32_t)(d.l_pac - x.offset);
    it.tlen = (uint16_t)l_ref;
    r.cit = (uint32_t)atomicAdd(d.ctl + C_NCIG, 1ull);
    d.citems[r.cit] = it;
}
__global__ void __launch_bounds__(128) k_pl_pick(PlDev d)
{
    const uint32_t n_units = d.paired ? d.n_rec / 2 : d.n_rec;
    PSTRIDE(u, n_units) {
        if (!d.paired) {
            PlRec r = d.rec[u];
            PlHit *h0 = d.hits + d.hbase[u], *h1 = h0 + r.nh[0];
            pl_scores(d, (uint32_t)u, r, h0, h1);
            pl_pick(h0, r.nu[0], h1, r.nu[1], r.w);
            pl_cigar_item(d, (uint32_t)u, r, h0, h1);
            d.rec[u] = r;
        } else {
            const uint32_t ia = 2 * (uint32_t)u, ib = ia + 1;
            PlRec a = d.rec[ia], b = d.rec[ib];
            PlHit *a0 = d.hits + d.hbase[ia], *a1 = a0 + a.nh[0], *b0 = d.hits + d.hbase[ib], *b1 = b0 + b.nh[0];
            pl_scores(d, ia, a, a0, a1); pl_scores(d, ib, b, b0, b1);
            const bool proper = pl_pick_pair(a0, a.nu[0], a1, a.nu[1], b0, b.nu[0], b1, b.nu[1], a.w, b.w);
            a.proper = b.proper = proper ? 1u : 0u;
            if (proper) atomicAdd(d.ctl + C_PROPER, 1ull);
            pl_cigar_item(d, ia, a, a0, a1); pl_cigar_item(d, ib, b, b0, b1);
            d.rec[ia] = a; d.rec[ib] = b;
        }
    }
}

// what the printer needs of record i; false: "push cigar error" (polish.c:211-214, 238-241)
__device__ __forceinline__ bool pl_out_of(const PlDev &d, uint32_t i, PlOut &o)
{
    const PlRec &r = d.rec[i];
    o.name = d.raw + r.f.name_off; o.name_len = r.f.name_len; o.qual = d.raw + r.f.qual_off; o.qual_len = r.f.qual_len;
    o.codes = d.codes + d.offs[i]; o.l_seq = r.f.l_seq; o.flag = r.f.flag; o.qual_seq = d.qual_seq; o.w = r.w;
    o.pos = 0; o.chrom = nullptr; o.chrom_len = 0; o.star = 0; o.cigar = nullptr; o.n_cigar = 0; o.clip_front = o.clip_back = 0;
    if (r.w.strand == -1 || r.w.primary == -1) { o.w.strand = -1; return true; }
    const PlHit x = (d.hits + d.hbase[i] + (r.w.strand ? r.nh[0] : 0u))[r.w.primary];
    o.pos = x.pos; o.chrom = d.ct.names + d.ct.name_off[x.contig]; o.chrom_len = d.ct.name_off[x.contig + 1] - d.ct.name_off[x.contig];
    if (r.cit == 0xFFFFFFFFu) { o.star = 1; return true; }
    if (d.use_sw) {
        const PeSwRes &s = d.cres[r.cit];
        o.cigar = s.cigar; o.n_cigar = s.n_cigar; o.clip_front = s.read_begin; o.clip_back = (int32_t)r.f.l_seq - s.read_end - 1;
        return s.score1 == x.score;
    }
    o.cigar = d.ccig + (uint64_t)r.cit * SALT_MAX_CIGAR_OPS; o.n_cigar = d.cnc[r.cit];
    return d.cdist[r.cit] == -x.score;
}
template <class E> __device__ __forceinline__ bool pl_record(const PlDev &d, uint32_t i, E &e)
{
    PlOut me;
    bool ok = pl_out_of(d, i, me);
    if (!d.paired) { pl_print_se(e, me); return ok; }
    PlOut mate;
    ok = pl_out_of(d, i ^ 1u, mate) && ok;
    pl_print_pe(e, me, mate, (i & 1u) ? mate : me, (int)(i & 1u), d.rec[i].proper != 0);
    return ok;
}
__global__ void __launch_bounds__(128) k_pl_len(PlDev d, uint32_t *__restrict__ len)
{
    // (the loop runs whole waves: every lane takes part in the byte count's reduction)
    const uint64_t n_up = ((uint64_t)d.n_rec + 63) & ~63ull;
    PSTRIDE(i, n_up) {
        PlCount c;
        if (i < d.n_rec && !d.rec[i].dead) {
            if (!pl_record(d, (uint32_t)i, c)) pl_fail(d.ctl, i, PL_E_CIGAR);
        }
        if (i < d.n_rec) len[i] = c.n;
        unsigned long long mine = c.n;                           // the block's bytes in 64 bits beside the 32-bit offsets of the scan
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
        if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(d.ctl + C_BYTES, mine);
    }
}
__global__ void __launch_bounds__(128) k_pl_write(PlDev d, const uint32_t *__restrict__ off, char *__restrict__ out)
{
    PSTRIDE(i, d.n_rec) {
        if (d.rec[i].dead) continue;
        PlWrite w; w.o = out + off[i];
        pl_record(d, (uint32_t)i, w);
    }
}

// ---- the handle's text state -------------------------------------------------------------------------------------------------
struct DBuf { void *p = nullptr; uint64_t cap = 0; };
struct PolishText {
    DBuf raw, tile, lines, rec, hcount, lseq, nuc, nclip, outlen, hits, codes, items, pool, dist, req, res, citems, cdist, ccig, cnc, cres, creq, scratch, scan, out;
    DBuf names, name_off, c_off;                                 // the sorted contig table
    int32_t n_contigs = 0;
    unsigned long long *d_ctl = nullptr; PeCtl *d_pctl = nullptr;
    unsigned long long *h_words = nullptr;                       // page-locked: count words read back, the PeCtl staged
    char *h_out = nullptr; uint64_t h_out_cap = 0;
    hipStream_t st = nullptr;
    uint64_t stats[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    uint64_t n_mallocs = 0;
    PlDev fused;                                                 // the fused route's block between polish_rows_len and polish_rows_write
};

PolishText *polish_text_new() { return new PolishText(); }
void polish_text_free(PolishText *t)
{
    if (!t) return;
    DBuf *all[] = { &t->raw, &t->tile, &t->lines, &t->rec, &t->hcount, &t->lseq, &t->nuc, &t->nclip, &t->outlen, &t->hits, &t->codes, &t->items, &t->pool, &t->dist, &t->req,
                    &t->res, &t->citems, &t->cdist, &t->ccig, &t->cnc, &t->cres, &t->creq, &t->scratch, &t->scan, &t->out, &t->names, &t->name_off, &t->c_off };
    for (DBuf *b : all) hipFree(b->p);
    hipFree(t->d_ctl); hipFree(t->d_pctl);
    if (t->h_words) hipHostFree(t->h_words);
    if (t->h_out) hipHostFree(t->h_out);
    if (t->st) hipStreamDestroy(t->st);
    delete t;
}
const uint64_t *polish_text_stats(const PolishText *t) { return t->stats; }

// a kernel launch with its launch status checked: a failed launch is SALT_E_HIP here, not stale counts later
#define PLRUN(...) do { hipLaunchKernelGGL(__VA_ARGS__); PLCHK(hipGetLastError()); } while (0)
#define PLCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return SALT_E_HIP; } } while (0)
// grows (never shrinks) a device buffer; what it held is gone
static hipError_t grow(PolishText *t, DBuf &b, uint64_t bytes)
{
    if (bytes <= b.cap && b.p) return hipSuccess;
    hipFree(b.p); b.p = nullptr; b.cap = 0;
    const uint64_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e == hipSuccess) { b.cap = want; ++t->n_mallocs; }
    return e;
}

int polish_text_set_contigs(PolishText *t, int32_t n, const int64_t *offsets, const char *const *names, std::string &err)
{
    std::vector<int32_t> order((size_t)n);
    for (int32_t i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return strcmp(names[a], names[b]) < 0; });
    std::vector<int64_t> off; std::vector<uint32_t> noff; std::string blob;
    for (int32_t k = 0; k < n; ++k) {
        const int32_t i = order[(size_t)k];
        if (k + 1 < n && strcmp(names[i], names[order[(size_t)k + 1]]) == 0) continue;      // of equal names the last one counts, as in the host path's map
        noff.push_back((uint32_t)blob.size()); blob += names[i]; off.push_back(offsets[i]);
    }
    noff.push_back((uint32_t)blob.size());
    PLCHK(grow(t, t->names, blob.size() + 8)); PLCHK(grow(t, t->name_off, noff.size() * 4)); PLCHK(grow(t, t->c_off, off.size() * 8 + 8));
    PLCHK(hipMemcpy(t->names.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    PLCHK(hipMemcpy(t->name_off.p, noff.data(), noff.size() * 4, hipMemcpyHostToDevice));
    if (!off.empty()) PLCHK(hipMemcpy(t->c_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    t->n_contigs = (int32_t)off.size();
    return SALT_OK;
}

static std::string pl_message(int code, uint64_t recno, const char *sam, const PlRec &r)
{
    switch (code) {
    case PL_E_FIELDS: return "malformed SAM record " + std::to_string(recno) + " of the block: fewer than 11 fields";
    case PL_E_CONTIG: return "sequence " + (sam ? std::string(sam + r.bad_b, r.bad_e - r.bad_b) : std::string("?")) + " is not in the index";
    case PL_E_LEN: case PL_E_WINDOW: return "polish item: read length / window / bound outside the kernel's range";
    case PL_E_RANGE: return "[Error]: Out of reference length!";
    case PL_E_NOALN: return (sam ? std::string(sam + r.f.name_off, r.f.name_len) : "record " + std::to_string(recno) + " of the block") + ": the mate of a proper pair has no alignment within " + std::to_string(PL_MAX_DISTANCE) +
                            " edits (the reference runs its CIGAR routine with k = 100000 here)";
    case PL_E_CIGAR: return "push cigar error!";
    default: return "polish text: unknown status";
    }
}

// one failed record: its status and what the message needs of it (0: none failed).  sam: the block's text, null on the fused route
static int pl_failed(const unsigned long long *hw, const PlRec *rec, const char *sam, std::string &msg)
{
    if (hw[C_ERR] == ~0ull) return 0;
    const uint64_t recno = hw[C_ERR] >> 8; const int code = (int)(hw[C_ERR] & 0xFF);
    PlRec r; memset(&r, 0, sizeof r);
    if (hipMemcpy(&r, rec + recno, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) { msg = "polish text: a record failed and its status could not be read"; return SALT_E_HIP; }
    msg = pl_message(code, recno, sam, r);
    return SALT_E_INVAL;
}
static hipError_t pl_ctl_init(PolishText *t, hipStream_t st)
{
    unsigned long long *hw = t->h_words;
    hw[16 + C_STOP] = ~0ull; hw[16 + C_ERR] = ~0ull; hw[16 + C_MAXLEN] = 0; hw[16 + C_NCLIP] = 0; hw[16 + C_NCIG] = 0; hw[16 + C_PROPER] = 0; hw[16 + C_BYTES] = 0;
    return hipMemcpyAsync(t->d_ctl, hw + 16, C_N * 8, hipMemcpyHostToDevice, st);
}
static int pl_state(PolishText *t, std::string &err)
{
    if (!t->d_ctl) { PLCHK(hipMalloc((void **)&t->d_ctl, C_N * 8)); PLCHK(hipMalloc((void **)&t->d_pctl, sizeof(PeCtl))); PLCHK(hipHostMalloc((void **)&t->h_words, 512, hipHostMallocDefault)); }
    return SALT_OK;
}
// the per-record arrays both front ends fill: n1 = records + 1
static int pl_grow_records(PolishText *t, uint64_t n1, std::string &err)
{
    PLCHK(grow(t, t->rec, n1 * sizeof(PlRec))); PLCHK(grow(t, t->hcount, n1 * 4)); PLCHK(grow(t, t->nuc, n1 * 4)); PLCHK(grow(t, t->nclip, n1 * 4)); PLCHK(grow(t, t->outlen, n1 * 4));
    PLCHK(grow(t, t->scan, text_scan_bytes(std::max<uint64_t>(n1, 1024))));
    return SALT_OK;
}

// ---- the tail both entries share: everything behind the front end (k_pl_fill of the text route, k_pl_rows of the fused one) ----
// In: d.rec / d.hits / d.hbase / d.codes / d.offs filled, d.nuc / d.nclip the unscanned counts with entry n_rec zeroed, the control words.
// pl_tail_len: items, scores, winners, the winners' CIGARs, the record lengths and their scan (left in t->outlen); *total = all bytes.
// pl_tail_write: the records into d_out (device memory, *total bytes).  sam: the block's text for the messages, or null.
struct PlTail { const uint8_t *pac; uint64_t l_pac; void *tabs; uint32_t n_blocks, max_len; const char *sam; hipStream_t st; uint32_t n_items, n_cig; uint64_t n_clip, n_proper; };
static int pl_tail_len(PolishText *t, PlDev &d, PlTail &x, uint32_t *total, std::string &err)
{
    hipStream_t st = x.st;
    unsigned long long *hw = t->h_words;
    const uint32_t n_rec = d.n_rec; const int use_sw = d.use_sw;
    uint32_t *nuc = d.nuc, *nclip = d.nclip, *outlen = (uint32_t *)t->outlen.p;
    PLCHK(launch_text_scan(nuc, n_rec + 1, t->scan.p, t->scan.cap, st));
    PLCHK(launch_text_scan(nclip, n_rec + 1, t->scan.p, t->scan.cap, st));
    PLCHK(hipMemcpyAsync(hw, t->d_ctl, C_N * 8, hipMemcpyDeviceToHost, st));
    PLCHK(hipMemcpyAsync(hw + 8, nuc + n_rec, 4, hipMemcpyDeviceToHost, st));
    PLCHK(hipMemcpyAsync(hw + 9, nclip + n_rec, 4, hipMemcpyDeviceToHost, st));
    PLCHK(hipStreamSynchronize(st));
    if (int rc = pl_failed(hw, d.rec, x.sam, err)) return rc;
    const uint32_t n_items = *(uint32_t *)(hw + 8), n_pool = *(uint32_t *)(hw + 9);
    x.n_items = n_items; x.n_clip = hw[C_NCLIP];
    // ---- items, scores ----
    PLCHK(grow(t, t->items, ((uint64_t)n_items + 1) * sizeof(salt_polish_item_t))); PLCHK(grow(t, t->dist, ((uint64_t)n_items + 1) * 4));
    PLCHK(grow(t, t->pool, ((uint64_t)n_pool + 1) * PL_POOL_STRIDE + 8));
    PLCHK(grow(t, t->citems, ((uint64_t)n_rec + 1) * sizeof(salt_polish_item_t)));
    d.items = (salt_polish_item_t *)t->items.p; d.pool = (uint8_t *)t->pool.p; d.dist = (const int32_t *)t->dist.p; d.citems = (salt_polish_item_t *)t->citems.p;
    IndexView v; memset(&v, 0, sizeof v);
    v.ref_len = (uint32_t)x.l_pac;                               // k_sw's range check; mode 2 reads the 2-bit genome only
    SwGeom geom = sw_geom(x.max_len, x.max_len, x.n_blocks / 8u);
    if (n_items) {
        PLRUN(k_pl_items, dim3(pgrid(n_rec)), dim3(128), 0, st, d);
        if (use_sw) {
            SwGeom g1 = geom; sw_geom_limit(g1, (n_items + 7u) / 8u);
            PLCHK(grow(t, t->req, (uint64_t)n_items * sizeof(PeSwReq))); PLCHK(grow(t, t->res, (uint64_t)n_items * sizeof(PeSwRes))); PLCHK(grow(t, t->scratch, sw_scratch_bytes(g1)));
            PeCtl *hc = (PeCtl *)(hw + 32); memset(hc, 0, sizeof *hc); hc->n_req = n_items;
            PLCHK(hipMemcpyAsync(t->d_pctl, hc, sizeof *hc, hipMemcpyHostToDevice, st));
            PLRUN(k_pl_swreq, dim3(pgrid(n_items)), dim3(128), 0, st, d.items, n_items, 1, (PeSwReq *)t->req.p);
            launch_sw(v, x.pac, d.codes, d.offs, (const PeSwReq *)t->req.p, t->d_pctl, (PeSwRes *)t->res.p, (uint8_t *)t->scratch.p, g1, x.max_len, st);
            PLCHK(hipGetLastError());
            PLRUN(k_pl_swscore, dim3(pgrid(n_items)), dim3(128), 0, st, (const PeSwRes *)t->res.p, n_items, (int32_t *)t->dist.p);
        } else
            launch_polish(x.pac, d.codes, d.offs, d.items, n_items, d.pool, PL_POOL_STRIDE, 0, (int32_t *)t->dist.p, nullptr, nullptr, x.tabs, n_items < x.n_blocks ? n_items : x.n_blocks, st);
        PLCHK(hipGetLastError());
    }
    // ---- winners ----
    PLRUN(k_pl_pick, dim3(pgrid(n_rec)), dim3(128), 0, st, d);
    PLCHK(hipMemcpyAsync(hw, t->d_ctl, C_N * 8, hipMemcpyDeviceToHost, st));
    if (use_sw && n_items) PLCHK(hipMemcpyAsync(hw + 8, &t->d_pctl->overflow, 4, hipMemcpyDeviceToHost, st)); else hw[8] = 0;
    PLCHK(hipStreamSynchronize(st));
    static const char *BAND = "polish -s: an alignment needs a wider band or more CIGAR operations than this build holds";
    if (*(uint32_t *)(hw + 8)) { err = BAND; return SALT_E_INVAL; }
    if (int rc = pl_failed(hw, d.rec, x.sam, err)) return rc;
    const uint32_t n_cig = (uint32_t)hw[C_NCIG];
    x.n_cig = n_cig; x.n_proper = hw[C_PROPER];
    // ---- CIGARs of the winners ----
    if (n_cig && use_sw) {
        SwGeom g2 = geom; sw_geom_limit(g2, (n_cig + 7u) / 8u);
        PLCHK(grow(t, t->creq, (uint64_t)n_cig * sizeof(PeSwReq))); PLCHK(grow(t, t->cres, (uint64_t)n_cig * sizeof(PeSwRes))); PLCHK(grow(t, t->scratch, sw_scratch_bytes(g2)));
        PeCtl *hc = (PeCtl *)(hw + 32); memset(hc, 0, sizeof *hc); hc->n_req = n_cig;
        PLCHK(hipMemcpyAsync(t->d_pctl, hc, sizeof *hc, hipMemcpyHostToDevice, st));
        PLRUN(k_pl_swreq, dim3(pgrid(n_cig)), dim3(128), 0, st, d.citems, n_cig, 0, (PeSwReq *)t->creq.p);
        launch_sw(v, x.pac, d.codes, d.offs, (const PeSwReq *)t->creq.p, t->d_pctl, (PeSwRes *)t->cres.p, (uint8_t *)t->scratch.p, g2, x.max_len, st);
        PLCHK(hipGetLastError());
        d.cres = (const PeSwRes *)t->cres.p;
    } else if (n_cig) {
        PLCHK(grow(t, t->cdist, (uint64_t)n_cig * 4)); PLCHK(grow(t, t->ccig, (uint64_t)n_cig * SALT_MAX_CIGAR_OPS * 2)); PLCHK(grow(t, t->cnc, (uint64_t)n_cig + 8));
        PLCHK(hipMemsetAsync(t->cnc.p, 0, n_cig, st));
        launch_polish(x.pac, d.codes, d.offs, d.citems, n_cig, nullptr, PL_POOL_STRIDE, 1, (int32_t *)t->cdist.p, (uint16_t *)t->ccig.p, (uint8_t *)t->cnc.p, x.tabs,
                      n_cig < x.n_blocks ? n_cig : x.n_blocks, st);
        PLCHK(hipGetLastError());
        d.cdist = (const int32_t *)t->cdist.p; d.ccig = (const uint16_t *)t->ccig.p; d.cnc = (const uint8_t *)t->cnc.p;
    }
    // ---- records ----
    PLCHK(hipMemsetAsync(outlen + n_rec, 0, 4, st));
    PLRUN(k_pl_len, dim3(pgrid(n_rec)), dim3(128), 0, st, d, outlen);
    PLCHK(launch_text_scan(outlen, n_rec + 1, t->scan.p, t->scan.cap, st));
    PLCHK(hipMemcpyAsync(hw, t->d_ctl, C_N * 8, hipMemcpyDeviceToHost, st));
    PLCHK(hipMemcpyAsync(hw + 8, outlen + n_rec, 4, hipMemcpyDeviceToHost, st));
    if (use_sw && n_cig) PLCHK(hipMemcpyAsync(hw + 9, &t->d_pctl->overflow, 4, hipMemcpyDeviceToHost, st)); else hw[9] = 0;
    PLCHK(hipStreamSynchronize(st));
    if (*(uint32_t *)(hw + 9)) { err = BAND; return SALT_E_INVAL; }
    if (int rc = pl_failed(hw, d.rec, x.sam, err)) return rc;
    if (hw[C_BYTES] >> 32) { err = "the polished records of this block pass 4 GiB (their offsets are 32-bit): hand over smaller blocks"; return SALT_E_CAPACITY; }
    *total = *(uint32_t *)(hw + 8);
    return SALT_OK;
}
static int pl_tail_write(PolishText *t, const PlDev &d, hipStream_t st, char *d_out, std::string &err)
{
    PLRUN(k_pl_write, dim3(pgrid(d.n_rec)), dim3(128), 0, st, d, (const uint32_t *)t->outlen.p, d_out);
    return SALT_OK;
}

int polish_text_run(PolishText *t, const uint8_t *d_pac, uint64_t l_pac, void *d_tabs, uint32_t n_blocks, int paired, int use_sw, const char *sam, uint64_t n_bytes,
                    const char **out, uint64_t *out_bytes, uint32_t *n_records, int *stopped, std::string &err)
{
    *out = ""; *out_bytes = 0; *n_records = 0; *stopped = 0;
    memset(t->stats, 0, sizeof t->stats);
    if (!t->st) PLCHK(hipStreamCreateWithFlags(&t->st, hipStreamNonBlocking));
    if (int rc = pl_state(t, err)) return rc;
    if (!t->h_out) { PLCHK(hipHostMalloc((void **)&t->h_out, 4096, hipHostMallocDefault)); t->h_out_cap = 4096; }
    *out = t->h_out;
    if (n_bytes == 0) return SALT_OK;
    hipStream_t st = t->st;
    unsigned long long *hw = t->h_words;
    const uint64_t n_tiles = (n_bytes + FQ_TILE - 1) / FQ_TILE;
    // ---- lines ----
    PLCHK(grow(t, t->raw, n_bytes + 8)); PLCHK(grow(t, t->tile, (n_tiles + 1) * 4));
    PLCHK(grow(t, t->scan, text_scan_bytes(std::max<uint64_t>(n_tiles + 1, 1024))));
    PLCHK(hipMemcpyAsync(t->raw.p, sam, n_bytes, hipMemcpyHostToDevice, st));
    const uint8_t *raw = (const uint8_t *)t->raw.p;
    uint32_t *tile = (uint32_t *)t->tile.p;
    PLCHK(launch_fq_count(raw, n_bytes, tile, t->scan.p, t->scan.cap, st));
    uint32_t n_newlines = 0;
    PLCHK(hipMemcpyAsync(hw, tile + n_tiles, 4, hipMemcpyDeviceToHost, st));
    PLCHK(hipStreamSynchronize(st));
    n_newlines = *(uint32_t *)hw;
    const bool open_end = sam[n_bytes - 1] != '\n';             // a last line without its newline
    const uint32_t n_lines = n_newlines + (open_end ? 1u : 0u);
    const uint64_t n1 = (uint64_t)n_lines + 1;
    PLCHK(grow(t, t->lines, (n1 + 1) * 4)); PLCHK(grow(t, t->lseq, n1 * 4));
    if (int rc = pl_grow_records(t, n1, err)) return rc;
    uint32_t *lines = (uint32_t *)t->lines.p, *hcount = (uint32_t *)t->hcount.p, *lseq = (uint32_t *)t->lseq.p, *nuc = (uint32_t *)t->nuc.p, *nclip = (uint32_t *)t->nclip.p;
    PLCHK(launch_fq_lines(raw, n_bytes, tile, lines, st));
    if (open_end) { hw[8] = n_bytes + 1; PLCHK(hipMemcpyAsync(lines + n_lines, hw + 8, 4, hipMemcpyHostToDevice, st)); }
    PLCHK(pl_ctl_init(t, st));
    PlRec *rec = (PlRec *)t->rec.p;
    PLRUN(k_pl_stop, dim3(pgrid(n_lines)), dim3(128), 0, st, lines, n_lines, t->d_ctl);
    PLCHK(hipMemsetAsync(hcount + n_lines, 0, 4, st)); PLCHK(hipMemsetAsync(lseq + n_lines, 0, 4, st));
    PLRUN(k_pl_count, dim3(pgrid(n_lines)), dim3(128), 0, st, raw, lines, n_lines, paired, t->d_ctl, rec, hcount, lseq);
    PLCHK(launch_text_scan(hcount, (uint32_t)n1, t->scan.p, t->scan.cap, st));
    PLCHK(launch_text_scan(lseq, (uint32_t)n1, t->scan.p, t->scan.cap, st));
    PLCHK(hipMemcpyAsync(hw, t->d_ctl, C_N * 8, hipMemcpyDeviceToHost, st));
    PLCHK(hipMemcpyAsync(hw + 8, hcount + n_lines, 4, hipMemcpyDeviceToHost, st));
    PLCHK(hipMemcpyAsync(hw + 9, lseq + n_lines, 4, hipMemcpyDeviceToHost, st));
    PLCHK(hipStreamSynchronize(st));
    uint32_t n_rec = hw[C_STOP] < n_lines ? (uint32_t)hw[C_STOP] : n_lines;
    *stopped = hw[C_STOP] < n_lines ? 1 : 0;
    if (paired) n_rec &= ~1u;
    const uint32_t n_hits = *(uint32_t *)(hw + 8), n_bases = *(uint32_t *)(hw + 9), max_len = (uint32_t)hw[C_MAXLEN];
    if (int rc = pl_failed(hw, rec, sam, err)) return rc;
    if (n_rec == 0) return SALT_OK;
    // ---- hits, codes ----
    PLCHK(grow(t, t->hits, ((uint64_t)n_hits + 1) * sizeof(PlHit))); PLCHK(grow(t, t->codes, (uint64_t)n_bases + 64));
    PlDev d; memset(&d, 0, sizeof d);
    d.raw = raw; d.rec = rec; d.n_rec = n_rec; d.hits = (PlHit *)t->hits.p; d.hbase = hcount; d.offs = lseq; d.codes = (uint8_t *)t->codes.p;
    d.ct.off = (const int64_t *)t->c_off.p; d.ct.name_off = (const uint32_t *)t->name_off.p; d.ct.names = (const uint8_t *)t->names.p; d.ct.n = t->n_contigs;
    d.pac = d_pac; d.l_pac = l_pac; d.use_sw = use_sw; d.paired = paired; d.nuc = nuc; d.nclip = nclip; d.ibase = nuc; d.pbase = nclip; d.ctl = t->d_ctl;
    PLCHK(hipMemsetAsync(nuc + n_rec, 0, 4, st)); PLCHK(hipMemsetAsync(nclip + n_rec, 0, 4, st));
    PLRUN(k_pl_fill, dim3(pgrid(n_rec)), dim3(128), 0, st, d);
    PlTail x; memset(&x, 0, sizeof x);
    x.pac = d_pac; x.l_pac = l_pac; x.tabs = d_tabs; x.n_blocks = n_blocks; x.max_len = max_len; x.sam = sam; x.st = st;
    uint32_t total = 0;
    if (int rc = pl_tail_len(t, d, x, &total, err)) return rc;
    PLCHK(grow(t, t->out, (uint64_t)total + 64));
    if ((uint64_t)total + 64 > t->h_out_cap) {
        hipHostFree(t->h_out); t->h_out = nullptr; t->h_out_cap = 0; *out = "";
        const uint64_t want = (uint64_t)total + total / 4 + 64;
        PLCHK(hipHostMalloc((void **)&t->h_out, want, hipHostMallocDefault));
        t->h_out_cap = want; ++t->n_mallocs;
    }
    if (int rc = pl_tail_write(t, d, st, (char *)t->out.p, err)) return rc;
    PLCHK(hipMemcpyAsync(t->h_out, t->out.p, total, hipMemcpyDeviceToHost, st));
    PLCHK(hipStreamSynchronize(st));
    *out = t->h_out; *out_bytes = total; *n_records = n_rec;
    t->stats[0] = n_rec; t->stats[1] = n_hits; t->stats[2] = x.n_items; t->stats[3] = x.n_clip; t->stats[4] = x.n_cig; t->stats[5] = x.n_proper; t->stats[6] = total; t->stats[7] = 0;
    return SALT_OK;
}

// ---- the fused route (salt --polish): the records of a text call of the aligner, straight from its result rows -------------------------
// k_pl_rows stands where k_fq_count, k_fq_lines, k_pl_stop, k_pl_count and k_pl_fill stand on the text route (and k_sam_len / k_sam_write
// in front of them): a thread per record reads the head of its row (pl_row_hits: the first 104 bytes of the 880), sorts and checks its
// hits in the record's fixed span of 2 x PL_ROW_HITS entries, and fills the PlRec from the FqRec -- name and QUAL stay where they are in
// the FASTQ text, the codes are the aligner's own, as sequenced, and nothing is copied; PlFields.flag carries only bit 0x10 of the line's FLAG (pl_row_rev).  A skipped read and both
// mates of a pair with a skipped mate are dead: no hits, no bytes, the slot stays.
__global__ void __launch_bounds__(128) k_pl_rows(PlDev d, const salt_result_t *__restrict__ res, const FqRec *__restrict__ fq, uint32_t *__restrict__ hbase)
{
    PSTRIDE(i, d.n_rec) {
        const salt_result_t &q = res[i];
        const FqRec fr = fq[i];
        PlRec r;
        r.f.name_off = fr.name_off; r.f.name_len = fr.name_len; r.f.qual_off = fr.qual_off; r.f.qual_len = fr.len; r.f.seq_off = fr.seq_off; r.f.l_seq = fr.len;
        r.f.chrom_off = r.f.chrom_len = r.f.xa_off = r.f.xa_end = r.f.pos = 0; r.f.flag = pl_row_rev(q, d.paired != 0) ? 0x10 : 0; r.f.has_primary = q.pos != 0xFFFFFFFFu;
        r.line_b = r.line_e = r.bad_b = r.bad_e = r.proper = 0; r.cit = 0xFFFFFFFFu; r.w.strand = r.w.primary = -1; r.w.b0 = r.w.b1 = PL_UNMAPPED;
        r.nh[0] = r.nh[1] = PL_ROW_HITS;                         // the strands' spans are fixed: strand 1 starts PL_ROW_HITS entries in
        r.nu[0] = r.nu[1] = 0;
        r.dead = (q.skipped || (d.paired && res[i ^ 1u].skipped)) ? 1u : 0u;
        const uint32_t hb = (uint32_t)i * 2u * PL_ROW_HITS;
        uint32_t n_clip = 0;
        if (!r.dead) {
            PlHit *h0 = d.hits + hb, *h1 = h0 + PL_ROW_HITS;
            uint32_t nh[2];
            pl_row_hits(q, d.paired != 0, d.ct.off, d.ct.n, h0, h1, nh);
            r.nu[0] = pl_sort_unique(h0, nh[0]); r.nu[1] = pl_sort_unique(h1, nh[1]);
            int st = (r.f.l_seq == 0 || r.f.l_seq > PL_MAX_READ) ? (int)PL_E_LEN
                   : pl_windows<salt_polish_item_t>((uint32_t)i, r.f.l_seq, d.l_pac, d.use_sw != 0, h0, r.nu[0], h1, r.nu[1], d.pac, nullptr, nullptr, 0, n_clip);
            if (st) { pl_fail(d.ctl, i, st); r.nu[0] = r.nu[1] = 0; n_clip = 0; }
        }
        d.rec[i] = r; hbase[i] = hb;
        d.nuc[i] = r.nu[0] + r.nu[1]; d.nclip[i] = d.use_sw ? 0u : n_clip;
        if (n_clip) atomicAdd(d.ctl + C_NCLIP, (unsigned long long)n_clip);
    }
}

int polish_rows_len(PolishText *t, const PolishRows &in, uint64_t *total, std::string &err)
{
    *total = 0;
    if (int rc = pl_state(t, err)) return rc;
    if (in.n_rec == 0) return SALT_OK;
    if ((uint64_t)in.n_rec * 2u * PL_ROW_HITS >> 32) { err = "polish: more records in a block than its 32-bit hit offsets hold"; return SALT_E_CAPACITY; }
    hipStream_t st = in.st;
    if (int rc = pl_grow_records(t, (uint64_t)in.n_rec + 1, err)) return rc;
    PLCHK(grow(t, t->hits, (uint64_t)in.n_rec * 2u * PL_ROW_HITS * sizeof(PlHit)));
    PLCHK(pl_ctl_init(t, st));
    PlDev &d = t->fused;
    memset(&d, 0, sizeof d);
    uint32_t *nuc = (uint32_t *)t->nuc.p, *nclip = (uint32_t *)t->nclip.p;
    d.raw = in.raw; d.rec = (PlRec *)t->rec.p; d.n_rec = in.n_rec; d.hits = (PlHit *)t->hits.p; d.hbase = (const uint32_t *)t->hcount.p; d.offs = in.offs; d.codes = const_cast<uint8_t *>(in.codes);
    d.ct.off = in.c_off; d.ct.name_off = in.c_name_off; d.ct.names = reinterpret_cast<const uint8_t *>(in.c_names); d.ct.n = in.n_contigs;
    d.pac = in.pac; d.l_pac = in.l_pac; d.use_sw = in.use_sw; d.paired = in.paired; d.nuc = nuc; d.nclip = nclip; d.ibase = nuc; d.pbase = nclip; d.ctl = t->d_ctl; d.qual_seq = 1;
    PLCHK(hipMemsetAsync(nuc + in.n_rec, 0, 4, st)); PLCHK(hipMemsetAsync(nclip + in.n_rec, 0, 4, st));
    PLRUN(k_pl_rows, dim3(pgrid(in.n_rec)), dim3(128), 0, st, d, in.res, in.fq, (uint32_t *)t->hcount.p);
    PlTail x; memset(&x, 0, sizeof x);
    x.pac = in.pac; x.l_pac = in.l_pac; x.tabs = in.tabs; x.n_blocks = in.n_blocks; x.max_len = in.max_len; x.sam = nullptr; x.st = st;
    uint32_t tot = 0;
    if (int rc = pl_tail_len(t, d, x, &tot, err)) return rc;
    *total = tot;
    return SALT_OK;
}
int polish_rows_write(PolishText *t, char *d_out, hipStream_t st, std::string &err) { return pl_tail_write(t, t->fused, st, d_out, err); }

} // namespace salt
