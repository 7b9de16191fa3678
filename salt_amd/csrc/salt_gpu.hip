// salt_amd/csrc/salt_gpu.hip -- the C ABI of include/salt_gpu.h: device-index attach (re-packing
// the file-format arrays into the HBM layout of salt_device.h), per-batch workspaces, and the
// align entry points.  gfx950 only; fails loudly when no HIP device is usable.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <cstddef>
#include <cctype>
#include <map>
#include <utility>
#include <string>
#include <thread>
#include <vector>
#include <algorithm>
#include "salt_kernels.h"
#include "salt_inflate_block.h"
#include <rccl/rccl.h>

using namespace salt;

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
namespace salt { int set_last_error(int code, const std::string &msg) { return fail(code, msg); } }      // for the entry points of salt_vcf.hip

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) \
    return fail(SALT_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)
// the same in a function that frees its buffers in a lambda done(rc) on every return
#define DONECHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return done(fail(SALT_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_))); } while (0)

// A device buffer with its owner: p[0 .. cap) elements, freed with the owner.  alloc() gives it exactly n elements (what it held is freed
// first, so a failed call leaves it empty); reserve() is the grow-on-demand rule of every buffer a call may find too small: nothing when it is
// large enough, else the stream is drained (kernels queued on it may still read the old one) and it gets a quarter more than asked for.
template <class T> struct DevBuf {
    T *p = nullptr; uint64_t cap = 0;
    DevBuf() = default; DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { hipFree(p); }
    operator T *() const { return p; }
    T *operator->() const { return p; }
    void release() { hipFree(p); p = nullptr; cap = 0; }
    void take(DevBuf &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    hipError_t alloc(uint64_t n) { release(); const hipError_t e = hipMalloc((void **)&p, n * sizeof(T)); if (e == hipSuccess) cap = n; else p = nullptr; return e; }
    int reserve(uint64_t need, hipStream_t st)
    {
        if (need <= cap) return SALT_OK;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(alloc(need + need / 4));
        return SALT_OK;
    }
};
// Its sibling in page-locked host memory; adopt() takes a buffer the caller keeps owning.
template <class T> struct PinBuf {
    T *p = nullptr; uint64_t cap = 0; bool owned = true;
    PinBuf() = default; PinBuf(const PinBuf &) = delete; PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    operator T *() const { return p; }
    void release() { if (p && owned) hipHostFree(p); p = nullptr; cap = 0; owned = true; }
    void adopt(T *q, uint64_t n) { release(); p = q; cap = n; owned = false; }
    hipError_t alloc(uint64_t n) { release(); const hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault); if (e == hipSuccess) cap = n; else p = nullptr; return e; }
};

struct salt_gpu_index {
    int device = 0;
    uint8_t *image = nullptr;      // device
    uint64_t bytes = 0;
    bool owns = true;
    ImageHeader hdr;               // host copy
    IndexView view;
    uint8_t *d_pac = nullptr; uint64_t l_pac = 0;      // 2-bit genome for the PE singleton rescue (not part of the image)
    uint4 *d_rctx = nullptr;                            // context records of the R rows (attach_r_ctx; not part of the image)
    int64_t *d_c_off = nullptr; uint32_t *d_c_name_off = nullptr; char *d_c_names = nullptr; int32_t n_contigs = 0;     // contig table for the SAM kernels
    // The row tallies (in front of 4.6): each table is allocated by its first enable (not part of the image) and shared by every workspace of
    // the index while its gate is on.  snp: the site table (one record per 64 genome positions) and counts[snp_sites][4]; depth: the
    // difference array of ref_len + 1 words (the text state and its buffers come with the first salt_gpu_index_depth_text_begin);
    // errprof: E[2][512][95][4][4] and R[2][8] behind it, uint64; gt: salt_gt_site_t[snp_sites] as uint64 words, over the snp tally's site table
    // (built by whichever of the two is enabled first; the text state and its buffers come with the first salt_gpu_index_gt_text_begin).
    struct Tally { uint32_t min_mapq = 0; bool on = false; } snp, depth, errprof, gt, disc, stats, indel;
    DevBuf<SnpWin> d_snp_tab; DevBuf<uint32_t> d_snp_counts; uint64_t snp_win = 0; uint32_t snp_sites = 0;
    DevBuf<uint32_t> d_depth; DepthText *depth_text = nullptr;
    std::vector<int64_t> h_c_off; uint32_t c_name_max = 0;      // set_contigs' offsets and longest name, for the depth text
    DevBuf<unsigned long long> d_errprof;
    DevBuf<unsigned long long> d_gt; GtText *gt_text = nullptr;
    // disc: alt, uint64[ref_len] of three 21-bit fields, and the tally's own difference array of ref_len + 1 words (4.10)
    DevBuf<unsigned long long> d_disc_alt; DevBuf<uint32_t> d_disc_diff; uint32_t disc_min_baseq = 0; DiscText *disc_text = nullptr;
    // stats: SALT_STATS_CELLS cells, then CT[stats_contigs][8], uint64; stats_contigs is n_contigs as the first enable found it (4.11)
    DevBuf<unsigned long long> d_stats; int32_t stats_contigs = 0;
    // indel: 2^indel_log2 slots of (key, value), the four counters, and the tally's own difference array of ref_len + 1 words (4.12)
    DevBuf<IndelSlot> d_indel; DevBuf<unsigned long long> d_indel_stat; DevBuf<uint32_t> d_indel_diff; uint32_t indel_log2 = 0; IndelText *indel_text = nullptr;
};

// Every allocation below is a DevBuf / PinBuf: a new buffer is one field here and one reserve() or alloc() where it is sized.  Buffers that
// are filled together are sized together, by the reserve_* helpers further down.
struct salt_gpu_ws {
    salt_gpu_index *ix = nullptr;
    uint32_t max_reads = 0; uint64_t max_bases = 0;              // max_bases: what d_seqs holds (+ 64 bytes of slack)
    DevBuf<uint8_t> d_seqs; DevBuf<uint32_t> d_offs; DevBuf<salt_result_t> d_results;
    DevBuf<uint4> d_sai_c, d_sai_r;                              // reserve_seed: both hold d_sai_c.cap items
    uint32_t epoch = 1;                                 // the next call's epoch (1 .. SAI_EPOCH_MAX, salt_device.h): d_sai_r is zeroed when allocated and when the epoch restarts
    DevBuf<uint32_t> d_wq; uint32_t *d_wq_cnt = nullptr; uint32_t walk_blocks = 512; bool no_unique = false;      // k_seed's walk queues (sized with the seed arrays), k_seed_walk's grid; SALT_GPU_NO_UNIQUE
    DevBuf<uint32_t> d_pm, d_tb;                                 // k_pack's records (words; reserve_pack)
    DevBuf<uint8_t> d_heads; PinBuf<uint8_t> h_heads;        // first 128 bytes of every result row: dense device copy + pinned host staging
    DevBuf<unsigned long long> d_ctr;
    DevBuf<uint32_t> d_queue; SeCtl *d_qctl = nullptr;      // reads k_light hands to k_heavy; the batch's control words
    DevBuf<uint8_t> d_lvtab;                          // one LV traceback table per persistent k_heavy block
    DevBuf<uint8_t> d_gap; uint32_t gcap = 0; GapBufs gap{};                // deferred gapped passes
    // paired end (allocated on first use)
    DevBuf<uint8_t> d_pe_scr;                          // per persistent block: PE_LOCI_CAP loci + distances
    DevBuf<PePair> d_pairs; DevBuf<PeSwReq> d_req; DevBuf<PeSwRes> d_swres; DevBuf<PeCtl> d_pctl;      // pe_prepare: all four hold d_pairs.cap pairs
    DevBuf<uint8_t> d_sw_scr; uint32_t sw_blocks = 0;
    DevBuf<uint32_t> d_pcq;                            // k_cigar items of the gapped, not rescued mates
    // FASTQ text in / SAM text out (allocated on first use, grown on demand)
    DevBuf<uint8_t> d_raw; DevBuf<uint32_t> d_tile, d_lines;
    DevBuf<FqRec> d_rec; DevBuf<uint32_t> d_tctl, d_samoff; DevBuf<uint8_t> d_scan;      // d_tctl: parse ctl[4] | the SAM block's byte count in 64 bits | k_bam_len's error word
    DevBuf<char> d_sam; PinBuf<char> h_sam; DevBuf<char> d_rg; std::string rg;      // h_sam may be the caller's page-locked buffer (salt_gpu_ws_reserve_text)
    DevBuf<char> d_samslot; DevBuf<SamSeg> d_samseg;            // [max_reads]: the records' formatted heads and tails between k_sam_len and k_sam_write
    // salt_gpu_ws_set_sam_bgzf: the SAM block leaves as BGZF blocks (allocated on first use, grown on demand)
    bool sam_bgzf = false;
    // salt_gpu_ws_set_sam_bam: the text entry points write BAM records (k_bam_len / k_bam_write) where they wrote SAM lines
    bool sam_bam = false;
    // salt_gpu_ws_set_polish: the text entry points return the polished records of the block (salt_polish.hip) where they returned its SAM
    // lines; the polish buffers and Landau-Vishkin tables are this workspace's (allocated on first use)
    int polish = 0; PolishText *pl = nullptr; DevBuf<uint8_t> d_pl_tabs; uint32_t pl_blocks = 0;
    // salt_gpu_ws_set_trim: k_fq_trim stands behind k_fq_parse in the text entry points.  d_trim_cnt: the sixteen counters of the block being
    // parsed; they come back with the parser's control words (no wait of their own) and are added to trim_total once the parser has accepted
    // the block (a refused block is parsed again by the caller's own reader); trim_last: what the last call added (salt_gpu_ws_trim_uncount)
    bool trim = false; TrimRule trim_rule{}; DevBuf<unsigned long long> d_trim_cnt; DevBuf<uint32_t> d_trim_spans;
    uint64_t trim_total[2 * TRIM_N_COUNTS] = {}, trim_last[2 * TRIM_N_COUNTS] = {};
    // (not part of forget_last: the align stage of a text call forgets the tallies' jobs behind the parse stage that set trim_last)
    // salt_gpu_ws_set_trim_pair: the paired-end text entry point launches k_fq_trim_pair in k_fq_trim's place (step 2p of the rule); its eight
    // pair counters lie behind the sixteen in d_trim_cnt and travel with them.
    TrimPairRule trim_pair{};
    uint64_t trim_pair_total[TRIM_PAIR_N_COUNTS] = {}, trim_pair_last[TRIM_PAIR_N_COUNTS] = {};
    void trim_forget() { memset(trim_last, 0, sizeof trim_last); memset(trim_pair_last, 0, sizeof trim_pair_last); }
    DevBuf<uint32_t> d_bz_slots, d_bz_sizes; DevBuf<unsigned long long> d_bz_offs; DevBuf<uint8_t> d_bz_out;      // bgzf_bufs_alloc: d_bz_sizes.cap blocks
    PinBuf<char> h_bz;                                                       // only for a compressed block that outgrows h_sam
    // salt_gpu_ws_inflate_bgzf: a chunk's BGZF members, their offsets and status words, and the text they inflate to (allocated on first use, grown on demand)
    DevBuf<uint8_t> d_zin; DevBuf<unsigned long long> d_zoff; DevBuf<uint32_t> d_zstat;      // d_zoff: 2 x (d_zstat.cap + 1) offsets
    DevBuf<uint8_t> d_text; uint64_t text_bytes = 0;
    std::vector<unsigned long long> h_zoff; std::vector<uint32_t> h_zstat;
    uint32_t text_calls = 0;                                                 // SALT_TEXT_TRACE: stage clocks of the first text call
    uint32_t heavy_blocks = 2048, gap_blocks = 2048, cigar_blocks = 2048;
    QueueRange *d_ranges = nullptr;                                           // k_heavy's queue ranges: k_light's push counters, the heads
    // d_qctl, d_ranges and d_wq_cnt are blocks of ONE allocation, every block 256-byte aligned: one memset per call zeroes them all
    DevBuf<uint8_t> d_zero;
    int all_heavy = 0;
    hipStream_t stream = nullptr;
    bool timing = false;
    std::vector<hipEvent_t> ev;        // EV_PER_CALL per call: before k_pack, k_seed, k_light, k_heavy, k_gap, k_gapfin, k_cigar, after; paired end: after k_pair, k_sw, k_pe_final (+ its k_cigar)
    std::vector<uint8_t> ev_pe;        // the call was a paired-end one (its last three events are recorded)
    uint32_t n_timed = 0;
    // what the last align call added to each tally (n_rec 0: nothing) and on which stream, for the salt_gpu_ws_*_uncount calls; the error
    // profile's job carries its quality source
    template <class Job> struct LastJob { Job job{}; hipStream_t st = nullptr; };
    LastJob<SnpCount> snp_last; LastJob<DepthMark> depth_last; LastJob<ErrProf> ep_last; LastJob<GtAdd> gt_last; LastJob<DiscAdd> disc_last; LastJob<StatsAdd> stats_last; LastJob<IndelAdd> indel_last;
    void forget_last() { snp_last.job.n_rec = 0; depth_last.job.n_rec = 0; ep_last.job.n_rec = 0; gt_last.job.n_rec = 0; disc_last.job.n_rec = 0; stats_last.job.n_rec = 0; indel_last.job.n_rec = 0; }
    // the quality bytes of the error profile and the genotype sums: q_next is salt_gpu_ws_set_quals' pointer, waiting for the next host-buffer or resident call;
    // q_cur is the source of the call that is being queued (the text entry points set it to their raw block); d_quals holds a host call's bytes
    const uint8_t *q_next = nullptr; bool q_next_dev = false;
    struct { const uint8_t *quals = nullptr; const FqRec *rec = nullptr; uint64_t bytes = 0; } q_cur;
    DevBuf<uint8_t> d_quals;
};
static const uint32_t MAX_TIMED = 256, EV_PER_CALL = 12;

static inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

static void make_view(salt_gpu_index *ix)
{
    const ImageHeader &h = ix->hdr;
    IndexView &v = ix->view;
    uint8_t *b = ix->image;
    v.c_occ = reinterpret_cast<const COcc *>(b + h.off_c_occ);
    v.c_sa = reinterpret_cast<const uint32_t *>(b + h.off_c_sa);
    v.lkt = reinterpret_cast<const uint32_t *>(b + h.off_lkt);
    v.r_occ = reinterpret_cast<const ROcc *>(b + h.off_r_occ);
    v.r_pos = reinterpret_cast<const uint32_t *>(b + h.off_r_pos);
    v.wlkt = reinterpret_cast<const uint4 *>(b + h.off_wlkt);
    v.ref = reinterpret_cast<const uint32_t *>(b + h.off_ref);
    v.text = reinterpret_cast<const uint32_t *>(b + h.off_text);
    v.c_ctx = h.off_ctx ? reinterpret_cast<const uint4 *>(b + h.off_ctx) : nullptr; v.ctx_k = h.ctx_k;
    v.r_ctx = ix->d_rctx;
    v.c_primary = h.c_primary; memcpy(v.c_L2, h.c_L2, sizeof v.c_L2); v.c_seq_len = h.c_seq_len;
    v.r_text_len = h.r_text_len; v.r_inv_sa0 = h.r_inv_sa0; memcpy(v.r_cum, h.r_cum, sizeof v.r_cum);
    v.ref_len = h.ref_len; v.lkt_len = h.lkt_len; v.r_lkt_len = h.r_lkt_len;
}

extern "C" const char *salt_gpu_last_error(void) { return g_err.c_str(); }
extern "C" uint32_t salt_gpu_result_size(void) { return (uint32_t)sizeof(salt_result_t); }

// Context records for the R rows as well (r_ctx: 16 B per row of the R index, 20 GiB at GRCh38 scale; outside the image), when the C rows
// have theirs and the device keeps the caller's reserve free beside them for what comes after; SALT_GPU_NO_RCTX=1 leaves
// them out.  Results do not depend on them (ctx_reject is a lower bound).  The image is in place and W is chosen: the table never
// costs the W-mer table a base.  Does nothing when the table is there; without the room the index simply goes without (device of ix current).
static const uint64_t R_CTX_RESERVE_ATTACH = 40ull << 30;      // no workspace exists yet: the benchmark's four workspaces, result buffers and paired-end scratch (38.5 GiB)
static const uint64_t R_CTX_RESERVE_PAC = 32ull << 30;         // set_pac, as ever: the caller's workspaces usually exist by then
static int attach_r_ctx(salt_gpu_index *ix, const uint64_t R_CTX_RESERVE)
{
    if (!ix->view.c_ctx || ix->d_rctx || (getenv("SALT_GPU_NO_RCTX") && atoi(getenv("SALT_GPU_NO_RCTX")))) return SALT_OK;
    const uint64_t rbytes = ((uint64_t)ix->hdr.r_text_len + 1) * 16;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (uint64_t)free_b >= rbytes + R_CTX_RESERVE && hipMalloc((void **)&ix->d_rctx, rbytes) == hipSuccess) {
        launch_build_r_ctx(ix->view, ix->hdr.ctx_k, ix->d_rctx, nullptr);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { hipFree(ix->d_rctx); ix->d_rctx = nullptr; return fail(SALT_E_HIP, "building the R context records failed"); }
        ix->view.r_ctx = ix->d_rctx;
    } else { (void)hipGetLastError(); ix->d_rctx = nullptr; }
    return SALT_OK;
}

extern "C" int salt_gpu_index_attach(const salt_host_index_t *h, int device, salt_gpu_index_t **out)
{
    if (!h || !out) return fail(SALT_E_INVAL, "null argument");
    if (!h->c_bwt || !h->c_sa || !h->lkt || !h->r_bwt || !h->r_sa || !h->ref) return fail(SALT_E_INDEX, "missing index array");
    if (h->c_sa_intv == 0 || h->c_n_sa != (h->c_seq_len + h->c_sa_intv) / h->c_sa_intv) return fail(SALT_E_INDEX, "inconsistent C suffix-array sampling");
    if (h->lkt_len < 1 || h->lkt_len > 14 || h->lkt_n != (1u << (2 * h->lkt_len)) + 1) return fail(SALT_E_INDEX, "unsupported lookup-table length");
    if (h->r_n_sa != h->r_text_len - h->r_cum[4] + 1) return fail(SALT_E_INDEX, "R suffix array size does not match '#' count");
    if ((uint64_t)h->r_bwt_words * 8 < h->r_text_len) return fail(SALT_E_INDEX, "R BWT shorter than its text length");
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (n_dev <= 0) return fail(SALT_E_HIP, "no HIP device visible: the salt GPU path cannot run (there is no CPU fallback)");
    HIPCHK(hipSetDevice(device));

    salt_gpu_index *ix = new salt_gpu_index();
    ix->device = device;
    ImageHeader &hd = ix->hdr;
    memset(&hd, 0, sizeof hd);
    hd.magic = IMAGE_MAGIC;
    hd.c_primary = h->c_primary; memcpy(hd.c_L2, h->c_L2, sizeof hd.c_L2); hd.c_seq_len = h->c_seq_len; hd.c_sa_intv = h->c_sa_intv;
    hd.lkt_len = h->lkt_len; hd.lkt_n = h->lkt_n;
    hd.r_text_len = h->r_text_len; hd.r_inv_sa0 = h->r_inv_sa0; memcpy(hd.r_cum, h->r_cum, sizeof hd.r_cum);
    hd.ref_len = h->ref_len;
    // The context table (c_ctx, salt_device.h): 16 B per suffix-array row (46 GiB at GRCh38 scale), taken whenever the seed length is
    // known; SALT_GPU_NO_CTX=1 leaves it out (A/B runs, small devices).
    const uint64_t ctx_bytes = (((uint64_t)h->c_seq_len + 1) * 16 + 255) / 256 * 256;
    bool want_ctx = h->l_seed > 0 && !(getenv("SALT_GPU_NO_CTX") && atoi(getenv("SALT_GPU_NO_CTX")));
    {   // width of the device k-mer table: 32 B x 4^W (14: 8 GiB, 15: 32 GiB, 16: 128 GiB).  Every extra base saves each seed
        // one C and one R backward-search step (k_seed: -9 % per base) and makes more C intervals one row wide, which the entry then
        // resolves by itself, so the widest table that leaves room for the rest is taken: W = 16 on a 288 GB MI355X.
        uint32_t w = 14;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            if (want_ctx && (uint64_t)free_b < ctx_bytes + (24ull << 30)) want_ctx = false;          // a device this small keeps the table narrow and the windows random
            const uint64_t avail = (uint64_t)free_b - (want_ctx ? ctx_bytes : 0);
            w = avail >= (200ull << 30) ? 16 : avail >= (72ull << 30) ? 15 : 14;
        }
        if (const char *e = getenv("SALT_GPU_LKT_LEN")) w = (uint32_t)atoi(e);
        if (h->l_seed > 0 && w > (uint32_t)h->l_seed) w = (uint32_t)h->l_seed;
        if (h->l_seed <= 0) w = h->lkt_len;
        if (w < h->lkt_len) w = h->lkt_len;
        if (w > 16) w = 16;
        hd.r_lkt_len = w;
    }
    hd.n_c_blocks = (uint64_t)h->c_seq_len / 64 + 1;
    hd.n_r_blocks = (uint64_t)h->r_text_len / 128 + 1;
    const uint64_t ref_words = ((uint64_t)h->ref_len + 7) / 8;
    uint64_t off = align_up(sizeof(ImageHeader), 256);
    hd.off_c_occ = off; off = align_up(off + hd.n_c_blocks * sizeof(COcc), 256);
    hd.off_c_sa = off;  off = align_up(off + ((uint64_t)h->c_seq_len + 1) * 4, 256);
    hd.off_lkt = off;   off = align_up(off + (uint64_t)h->lkt_n * 4, 256);
    hd.off_r_occ = off; off = align_up(off + hd.n_r_blocks * sizeof(ROcc), 256);
    hd.off_r_pos = off; off = align_up(off + ((uint64_t)h->r_text_len + 1) * 4, 256);
    hd.off_ref = off;   off = align_up(off + (ref_words + 4) * 4, 256);
    hd.off_text = off;  off = align_up(off + ((uint64_t)h->c_seq_len / 16 + 4) * 4, 256);
    // last: everything before it is the COMPACT image, from which the W-mer table can be rebuilt on any device
    hd.off_wlkt = off; off = align_up(off + (1ull << (2 * hd.r_lkt_len)) * 32, 256);
    if (want_ctx) { hd.off_ctx = off; hd.ctx_k = (uint32_t)h->l_seed; off += ctx_bytes; }
    hd.bytes = off;
    ix->bytes = off;

    // ---- upload the file-format arrays and re-pack them on the device ----
    hipError_t e = hipMalloc((void **)&ix->image, ix->bytes);
    if (e != hipSuccess) { delete ix; return fail(SALT_E_NOMEM, std::string("hipMalloc(index image): ") + hipGetErrorString(e)); }
    uint32_t *d_sa_s = nullptr, *d_r_sa = nullptr, *d_raw = nullptr, *d_minor = nullptr, *d_major = nullptr, *d_err = nullptr;
#define CHK2(x) do { hipError_t e2 = (x); if (e2 != hipSuccess) { hipFree(ix->image); hipFree(d_sa_s); hipFree(d_r_sa); hipFree(d_raw); hipFree(d_minor); hipFree(d_major); hipFree(d_err); delete ix; \
    return fail(SALT_E_HIP, std::string(#x) + ": " + hipGetErrorString(e2)); } } while (0)
    CHK2(hipMemset(ix->image, 0, hd.off_wlkt));      // the W-mer table (last) is fully written by its kernel
    CHK2(hipMemcpy(ix->image, &hd, sizeof hd, hipMemcpyHostToDevice));
    CHK2(hipMalloc((void **)&d_err, 4)); CHK2(hipMemset(d_err, 0, 4));
    {   // C: 2-bit BWT with interleaved counts (bwt.h:57-64) -> 32-byte COcc blocks
        CHK2(hipMalloc((void **)&d_raw, (uint64_t)h->c_bwt_size * 4 + 4));
        CHK2(hipMemcpy(d_raw, h->c_bwt, (uint64_t)h->c_bwt_size * 4, hipMemcpyHostToDevice));
        launch_pack_c_occ(d_raw, h->c_bwt_size, h->c_seq_len, hd.n_c_blocks, reinterpret_cast<COcc *>(ix->image + hd.off_c_occ), d_err, nullptr);
        CHK2(hipGetLastError()); CHK2(hipDeviceSynchronize());
        hipFree(d_raw); d_raw = nullptr;
    }
    {   // R: 4-bit BWT + explicit Occ values (rbwt.c:40-80) -> 64-byte ROcc blocks
        CHK2(hipMalloc((void **)&d_raw, (uint64_t)h->r_bwt_words * 4 + 4));
        CHK2(hipMemcpy(d_raw, h->r_bwt, (uint64_t)h->r_bwt_words * 4, hipMemcpyHostToDevice));
        CHK2(hipMalloc((void **)&d_minor, (uint64_t)h->r_occ_words * 4 + 4)); CHK2(hipMemcpy(d_minor, h->r_occ, (uint64_t)h->r_occ_words * 4, hipMemcpyHostToDevice));
        CHK2(hipMalloc((void **)&d_major, (uint64_t)h->r_major_words * 4 + 4)); CHK2(hipMemcpy(d_major, h->r_major, (uint64_t)h->r_major_words * 4, hipMemcpyHostToDevice));
        launch_pack_r_occ(d_raw, h->r_bwt_words, d_minor, h->r_occ_words, d_major, h->r_major_words, h->r_text_len, hd.n_r_blocks,
                          reinterpret_cast<ROcc *>(ix->image + hd.off_r_occ), d_err, nullptr);
        CHK2(hipGetLastError()); CHK2(hipDeviceSynchronize());
        hipFree(d_raw); hipFree(d_minor); hipFree(d_major); d_raw = d_minor = d_major = nullptr;
    }
    {
        uint32_t perr = 0;
        CHK2(hipMemcpy(&perr, d_err, 4, hipMemcpyDeviceToHost));
        hipFree(d_err); d_err = nullptr;
        if (perr) {
            hipFree(ix->image); delete ix;
            return fail(SALT_E_INDEX, perr & 1 ? "C BWT array shorter than seq_len" : perr & 4 ? "R BWT holds a symbol outside {A,C,G,T,#}" : "R BWT / Occ arrays shorter than the text length");
        }
    }
    CHK2(hipMemcpy(ix->image + hd.off_lkt, h->lkt, (uint64_t)h->lkt_n * 4, hipMemcpyHostToDevice));
    CHK2(hipMemcpy(ix->image + hd.off_ref, h->ref, ref_words * 4, hipMemcpyHostToDevice));
    make_view(ix);
    // ---- expand the sampled suffix arrays / tabulate the R 12-mers on the device ----
    CHK2(hipMalloc((void **)&d_sa_s, (uint64_t)h->c_n_sa * 4));
    CHK2(hipMalloc((void **)&d_r_sa, (uint64_t)h->r_n_sa * 4));
    CHK2(hipMemcpy(d_sa_s, h->c_sa, (uint64_t)h->c_n_sa * 4, hipMemcpyHostToDevice));
    CHK2(hipMemcpy(d_r_sa, h->r_sa, (uint64_t)h->r_n_sa * 4, hipMemcpyHostToDevice));
    launch_build_c_sa(ix->view, d_sa_s, h->c_sa_intv, reinterpret_cast<uint32_t *>(ix->image + hd.off_c_sa), nullptr);
    launch_build_r_pos(ix->view, d_r_sa, reinterpret_cast<uint32_t *>(ix->image + hd.off_r_pos), nullptr);
    launch_build_text(ix->view, reinterpret_cast<uint32_t *>(ix->image + hd.off_text), nullptr);       // after c_sa (same stream)
    launch_build_wlkt(ix->view, hd.r_lkt_len, reinterpret_cast<uint4 *>(ix->image + hd.off_wlkt), nullptr);
    if (hd.off_ctx) launch_build_c_ctx(ix->view, hd.ctx_k, reinterpret_cast<uint4 *>(ix->image + hd.off_ctx), nullptr);      // after c_sa and text
    CHK2(hipGetLastError());
    CHK2(hipDeviceSynchronize());
    hipFree(d_sa_s); hipFree(d_r_sa);
#undef CHK2
    if (attach_r_ctx(ix, R_CTX_RESERVE_ATTACH)) g_err.clear();      // single end uses the R rows' records too; a build that fails has freed them and the index goes without: no error to report
    *out = ix;
    return SALT_OK;
}

extern "C" void salt_gpu_index_detach(salt_gpu_index_t *ix)
{
    if (!ix) return;
    if (ix->owns && ix->image) { hipSetDevice(ix->device); hipFree(ix->image); }
    if (ix->d_pac) { hipSetDevice(ix->device); hipFree(ix->d_pac); }
    if (ix->d_rctx) { hipSetDevice(ix->device); hipFree(ix->d_rctx); }
    if (ix->d_c_off) { hipSetDevice(ix->device); hipFree(ix->d_c_off); hipFree(ix->d_c_name_off); hipFree(ix->d_c_names); }
    hipSetDevice(ix->device);                                  // the tallies' DevBufs go with the index
    depth_text_free(ix->depth_text);
    gt_text_free(ix->gt_text);
    disc_text_free(ix->disc_text);
    indel_text_free(ix->indel_text);
    delete ix;
}

extern "C" int salt_gpu_index_image(const salt_gpu_index_t *ix, void **dev_ptr, uint64_t *bytes)
{
    if (!ix || !dev_ptr || !bytes) return fail(SALT_E_INVAL, "null argument");
    *dev_ptr = ix->image; *bytes = ix->bytes;
    return SALT_OK;
}

extern "C" int salt_gpu_index_attach_image(void *dev_ptr, uint64_t bytes, int device, salt_gpu_index_t **out)
{
    if (!dev_ptr || !out || bytes < sizeof(ImageHeader)) return fail(SALT_E_INVAL, "bad image");
    HIPCHK(hipSetDevice(device));
    salt_gpu_index *ix = new salt_gpu_index();
    ix->device = device; ix->image = static_cast<uint8_t *>(dev_ptr); ix->bytes = bytes; ix->owns = false;
    hipError_t e = hipMemcpy(&ix->hdr, dev_ptr, sizeof(ImageHeader), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { delete ix; return fail(SALT_E_HIP, std::string("hipMemcpy(image header): ") + hipGetErrorString(e)); }
    if (ix->hdr.magic != IMAGE_MAGIC || ix->hdr.bytes != bytes) { delete ix; return fail(SALT_E_INDEX, "not a salt device-index image"); }
    make_view(ix);
    *out = ix;
    return SALT_OK;
}

extern "C" int salt_gpu_index_image_compact(const salt_gpu_index_t *ix, void **dev_ptr, uint64_t *bytes)
{
    if (!ix || !dev_ptr || !bytes) return fail(SALT_E_INVAL, "null argument");
    *dev_ptr = ix->image; *bytes = ix->hdr.off_wlkt;
    return SALT_OK;
}

// the W-mer table and the context tables of an image whose compact part is in place (device of ix current)
static int rebuild_wlkt(salt_gpu_index *ix)
{
    launch_build_wlkt(ix->view, ix->hdr.r_lkt_len, reinterpret_cast<uint4 *>(ix->image + ix->hdr.off_wlkt), nullptr);
    if (ix->hdr.off_ctx) launch_build_c_ctx(ix->view, ix->hdr.ctx_k, reinterpret_cast<uint4 *>(ix->image + ix->hdr.off_ctx), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (attach_r_ctx(ix, R_CTX_RESERVE_ATTACH)) g_err.clear();      // as salt_gpu_index_attach
    return SALT_OK;
}

extern "C" int salt_gpu_index_attach_compact(const void *dev_ptr, uint64_t bytes, int device, salt_gpu_index_t **out)
{
    if (!dev_ptr || !out || bytes < sizeof(ImageHeader)) return fail(SALT_E_INVAL, "bad image");
    HIPCHK(hipSetDevice(device));
    ImageHeader hd;
    HIPCHK(hipMemcpy(&hd, dev_ptr, sizeof hd, hipMemcpyDeviceToHost));
    if (hd.magic != IMAGE_MAGIC || hd.off_wlkt != bytes || hd.bytes < bytes) return fail(SALT_E_INDEX, "not a compact salt device-index image");
    salt_gpu_index *ix = new salt_gpu_index();
    ix->device = device; ix->bytes = hd.bytes; ix->owns = true; ix->hdr = hd;
    hipError_t e = hipMalloc((void **)&ix->image, hd.bytes);
    if (e != hipSuccess) { delete ix; return fail(SALT_E_NOMEM, std::string("hipMalloc(index image): ") + hipGetErrorString(e)); }
    e = hipMemcpy(ix->image, dev_ptr, bytes, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { hipFree(ix->image); delete ix; return fail(SALT_E_HIP, std::string("hipMemcpy(compact image): ") + hipGetErrorString(e)); }
    make_view(ix);
    int rc = rebuild_wlkt(ix);
    if (rc) { hipFree(ix->image); delete ix; return rc; }
    *out = ix;
    return SALT_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" int salt_gpu_ws_create(salt_gpu_index_t *ix, uint32_t max_reads, uint64_t max_bases, salt_gpu_ws_t **out)
{
    if (!ix || !out || max_reads == 0) return fail(SALT_E_INVAL, "bad workspace size");
    HIPCHK(hipSetDevice(ix->device));
    salt_gpu_ws *ws = new salt_gpu_ws();
    ws->ix = ix; ws->max_reads = max_reads; ws->max_bases = max_bases;
#define CHKW(x) do { hipError_t e2 = (x); if (e2 != hipSuccess) { salt_gpu_ws_destroy(ws); \
    return fail(SALT_E_NOMEM, std::string(#x) + ": " + hipGetErrorString(e2)); } } while (0)
    CHKW(ws->d_seqs.alloc(max_bases + 64));
    CHKW(ws->d_offs.alloc((uint64_t)max_reads + 1));
    CHKW(ws->d_results.alloc(max_reads));
    CHKW(hipMemset(ws->d_results, 0, (uint64_t)max_reads * sizeof(salt_result_t)));
    CHKW(ws->d_queue.alloc(queue_words(max_reads)));         // the reads k_light queues (flat, and the segments they arrive in) + k_heavy's overflow queue
    {
        const size_t a = 256, n_ranges = (QUEUE_RANGES * sizeof(QueueRange) + a - 1) / a * a, n_ctl = (sizeof(SeCtl) + a - 1) / a * a;
        const size_t n_cnt = ((size_t)seed_wq_cnt_words() * 4 + a - 1) / a * a;
        CHKW(ws->d_zero.alloc(n_ranges + n_ctl + n_cnt));
        ws->d_ranges = reinterpret_cast<QueueRange *>(ws->d_zero.p); ws->d_qctl = reinterpret_cast<SeCtl *>(ws->d_zero + n_ranges);
        ws->d_wq_cnt = reinterpret_cast<uint32_t *>(ws->d_zero + n_ranges + n_ctl);
    }
    ws->gcap = max_reads < (1u << 20) ? max_reads : (1u << 20);         // slots for reads whose gapped pass is deferred (44 B each + their rows in the pool)
    if (const char *e3 = getenv("SALT_GPU_NO_GAP_DEFER")) if (atoi(e3)) ws->gcap = 0;
    if (const char *e3 = getenv("SALT_GPU_GAP_SLOTS")) { const int v = atoi(e3); if (v > 0 && (uint32_t)v < ws->gcap) ws->gcap = (uint32_t)v; }     // tests: the overflow pass
    if (ws->gcap) {
        size_t gbytes = 0;
        gap_bufs_layout(nullptr, ws->gcap, nullptr, &gbytes);
        CHKW(ws->d_gap.alloc(gbytes));
    }
    {
        hipDeviceProp_t prop;
        CHKW(hipGetDeviceProperties(&prop, ix->device));
        uint32_t per_cu = heavy_blocks_per_cu();                           // what LDS / VGPRs admit (16)
        // All of them: the persistent kernels are latency bound (alone: 4 -> 1.98, 5 -> 1.64, 6 -> 1.40, 8 -> 1.12, 12 -> 0.82, 16 -> 0.73 ms
        // per 10^6 GRCh38-scale reads; paired end 8 -> 2.65, 12 -> 2.01, 16 -> 1.76).  Until the waves took their reads through ONE counter the kernel stood at
        // 1.165 ms from 8 blocks per CU on (the counter's ~14 ns per pop x 75 700 reads) and eight was the default; with the ranged heads
        // (pop_ranged, salt_align.hip) it follows the waves again (profiles/r03/ab_heavy_ranged_pops.log)
        if (const char *e2 = getenv("SALT_GPU_HEAVY_PER_CU")) { int v = atoi(e2); if (v > 0 && (uint32_t)v <= heavy_blocks_per_cu()) per_cu = (uint32_t)v; }
        ws->heavy_blocks = (uint32_t)prop.multiProcessorCount * per_cu;    // persistent one-wave blocks
        // k_gap's items (64 candidates' Landau-Vishkin distances, tens of microseconds each) are independent and need no table of their own: its grid is
        // 16 per CU, not k_heavy's (13 079 items per 10^6 GRCh38-scale reads: 0.54 ms on 2 048 waves, 0.31 on 4 096, with the 9.3 KB of LDS a block
        // held then; at 6.2 KB and 98 VGPRs sixteen is what the registers admit, and 8 / 12 / 16 were taken again: profiles/r13/ab_gap_grid.log)
        uint32_t gap_per_cu = 16;
        if (const char *e2 = getenv("SALT_GPU_GAP_PER_CU")) { int v = atoi(e2); if (v > 0 && v <= 16) gap_per_cu = (uint32_t)v; }
        ws->gap_blocks = (uint32_t)prop.multiProcessorCount * gap_per_cu;
        // k_cigar behind k_gapfin: k_heavy's grid (it takes a block's traceback table from the same d_lvtab).  A block's first item is its own
        // index and costs no atomic, so with more blocks than items (2 805 per 10^6 GRCh38-scale reads) nobody touches the queue head and
        // nobody runs a second traceback: 26 us alone on 3 072 or 4 096 blocks against 84 on the 2 048 it had (profiles/r19)
        ws->cigar_blocks = ws->heavy_blocks;
        if (const char *e2 = getenv("SALT_GPU_CIGAR_BLOCKS")) { int v = atoi(e2); if (v > 0 && (uint32_t)v < ws->heavy_blocks) ws->cigar_blocks = (uint32_t)v; }      // measurements and tests: fewer blocks than items
        // k_seed_walk: 2 waves per SIMD in blocks of four waves.  Its lanes are all busy, so the grid is set by the four-stream step and not by
        // the kernel alone: 2 per CU 464 - 467 Mreads/s, 4 per CU 445 - 459, 8 per CU 450 - 458 (profiles/r07/ab_grid_and_order.log).  Measured again
        // with the walk that starts from its record (one turn less): 2 per CU 470 - 479, 3 per CU 469 - 479, 4 per CU 468 - 471; no range lies
        // above the range at 2 (profiles/r08/ab_walk_grid.log)
        ws->walk_blocks = (uint32_t)prop.multiProcessorCount * 2u;
        if (const char *e2 = getenv("SALT_GPU_WALK_PER_CU")) { int v = atoi(e2); if (v > 0 && v <= 16) ws->walk_blocks = (uint32_t)prop.multiProcessorCount * (uint32_t)v; }
        if (const char *e2 = getenv("SALT_GPU_SAI_EPOCH")) { const long long v = atoll(e2); if (v >= 1 && v <= (long long)SAI_EPOCH_MAX) ws->epoch = (uint32_t)v; }     // tests: the first call's epoch, so that a few calls cross the restart
        if (const char *e2 = getenv("SALT_GPU_NO_UNIQUE")) ws->no_unique = atoi(e2) != 0;                    // A/B and tests: every C search walks
        if (const char *e2 = getenv("SALT_GPU_WALK_BLOCKS")) { int v = atoi(e2); if (v > 0 && v <= 65536) ws->walk_blocks = (uint32_t)v; }      // tests: an absolute grid (rounded up to 64s), so that a wave's slice is long
        CHKW(ws->d_lvtab.alloc((uint64_t)ws->heavy_blocks * lv_table_bytes()));
        const char *e = getenv("SALT_GPU_ALL_HEAVY");
        ws->all_heavy = e && atoi(e) != 0;
    }
    CHKW(ws->d_ctr.alloc(SALT_CTR_N));
    CHKW(hipMemset(ws->d_ctr, 0, SALT_CTR_N * sizeof(unsigned long long)));
    CHKW(hipStreamCreate(&ws->stream));
#undef CHKW
    *out = ws;
    return SALT_OK;
}

extern "C" void salt_gpu_ws_destroy(salt_gpu_ws_t *ws)
{
    if (!ws) return;
    hipSetDevice(ws->ix->device);
    if (ws->stream) hipStreamDestroy(ws->stream);
    for (auto &e : ws->ev) if (e) hipEventDestroy(e);
    polish_text_free(ws->pl);
    delete ws;                                                // its buffers free themselves
}

static int check_opt(const salt_gpu_index *ix, const salt_aln_opt_t *o, uint32_t max_len, uint32_t *spr_out)
{
    if (o->l_seed < (int32_t)ix->hdr.r_lkt_len) return fail(SALT_E_INVAL, "l_seed shorter than the device k-mer table (set SALT_GPU_LKT_LEN or pass l_seed at attach)");
    if (o->l_overlap <= 0) return fail(SALT_E_INVAL, "l_overlap must be positive (aln.c:223 sets it to l_seed when -r is absent)");
    if (o->max_locate == 0 || o->max_locate > PE_LOCI_CAP) return fail(SALT_E_INVAL, "max_locate (-m) must be in 1..262144");
    if (o->max_hits != SALT_MAX_HITS) return fail(SALT_E_INVAL, "max_hits is fixed at 5 (aln.h:133)");
    if (max_len > SALT_MAX_READ_LEN) return fail(SALT_E_INVAL, "read longer than SALT_MAX_READ_LEN (512)");
    uint32_t spr = 1;
    if (max_len >= (uint32_t)o->l_seed) spr = (max_len - (uint32_t)o->l_seed) / (uint32_t)o->l_overlap + 1;
    if (spr > SALT_MAX_SEED_SLOTS) return fail(SALT_E_INVAL, "more seeds per strand than SALT_MAX_SEED_SLOTS (512): raise -r or shorten the reads");
    *spr_out = spr;
    return SALT_OK;
}

static int align_resident_impl(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, uint32_t n_reads, uint32_t max_read_len,
                               const void *d_seqs, const void *d_offs, void *d_results, void *hip_stream, int pe);

// A tally's launch, recorded as the workspace's last one.
template <class Job> static int tally_launch(salt_gpu_ws::LastJob<Job> &last, hipError_t (*launch)(const Job &, hipStream_t), const Job &c, hipStream_t st)
{
    HIPCHK(launch(c, st));
    last.job = c; last.st = st;
    return SALT_OK;
}
// The launches behind the kernels that finish a batch's result rows, on the batch's stream, one per tally that is on: the rows' bases at the
// SNP sites into the index's counts (k_snp_count), their M runs into its difference array (k_depth_mark), their base events into its error
// profile (k_errprof), their bases and qualities at the SNP sites into its genotype sums (k_gt_add), the bases the mixRef does not have into
// its candidate arrays (k_disc_add), the last three with the qualities of the
// call's source (ws->q_cur: the text block, salt_gpu_ws_set_quals' bytes, or
// none), what the run's summary counts of them into its tables (k_stats_add; pe_opt: the call's -a / -b window, null single end), and their
// insertions and deletions, left-shifted, into its table of allele keys (k_indel_add).
// Every entry point that leaves result rows passes here: single end at the end of align_resident_impl, paired end at the end of
// pe_resident_impl (the rows are final only behind k_pe_final).
static int rows_hooks(salt_gpu_ws_t *ws, uint32_t n_rec, const void *d_seqs, const void *d_offs, const void *d_results, const salt_pe_opt_t *pe_opt, hipStream_t st)
{
    const int pe = pe_opt ? 1 : 0;
    const salt_gpu_index *ix = ws->ix;
    const salt_result_t *res = static_cast<const salt_result_t *>(d_results);
    const uint8_t *seqs = static_cast<const uint8_t *>(d_seqs); const uint32_t *offs = static_cast<const uint32_t *>(d_offs);
    if (ix->snp.on) {
        SnpCount c{};
        c.res = res; c.seqs = seqs; c.offs = offs; c.n_rec = n_rec;
        c.tab = ix->d_snp_tab; c.n_win = ix->snp_win; c.counts = ix->d_snp_counts; c.min_mapq = ix->snp.min_mapq; c.pe = pe; c.delta = 1u;
        if (const int rc = tally_launch(ws->snp_last, launch_snp_count, c, st)) return rc;
    }
    if (ix->depth.on) {
        DepthMark c{};
        c.res = res; c.n_rec = n_rec; c.diff = ix->d_depth; c.ref_len = ix->view.ref_len; c.min_mapq = ix->depth.min_mapq; c.delta = 1u;
        if (const int rc = tally_launch(ws->depth_last, launch_depth_mark, c, st)) return rc;
    }
    if (ix->errprof.on) {
        ErrProf c{};
        c.res = res; c.seqs = seqs; c.offs = offs; c.n_rec = n_rec;
        c.quals = ws->q_cur.quals; c.rec = ws->q_cur.rec; c.q_bytes = ws->q_cur.bytes;
        c.ref = ix->view.ref; c.ref_len = ix->view.ref_len; c.cells = ix->d_errprof; c.min_mapq = ix->errprof.min_mapq; c.pe = pe; c.delta = 1ull;
        if (const int rc = tally_launch(ws->ep_last, launch_errprof, c, st)) return rc;
    }
    if (ix->gt.on) {
        GtAdd c{};
        c.res = res; c.seqs = seqs; c.offs = offs; c.n_rec = n_rec;
        c.quals = ws->q_cur.quals; c.rec = ws->q_cur.rec; c.q_bytes = ws->q_cur.bytes;
        c.tab = ix->d_snp_tab; c.n_win = ix->snp_win; c.sums = ix->d_gt; c.n_sites = ix->snp_sites; c.min_mapq = ix->gt.min_mapq; c.pe = pe; c.delta = 1ull;
        if (const int rc = tally_launch(ws->gt_last, launch_gt_add, c, st)) return rc;
    }
    if (ix->disc.on) {
        DiscAdd c{};
        c.res = res; c.seqs = seqs; c.offs = offs; c.n_rec = n_rec;
        c.quals = ws->q_cur.quals; c.rec = ws->q_cur.rec; c.q_bytes = ws->q_cur.bytes;
        c.ref = ix->view.ref; c.ref_len = ix->view.ref_len; c.alt = ix->d_disc_alt; c.diff = ix->d_disc_diff;
        c.min_mapq = ix->disc.min_mapq; c.min_baseq = ix->disc_min_baseq; c.pe = pe; c.delta = 1ull;
        if (const int rc = tally_launch(ws->disc_last, launch_disc_add, c, st)) return rc;
    }
    if (ix->stats.on) {
        if (!ix->d_c_off || ix->n_contigs != ix->stats_contigs)
            return fail(SALT_E_INVAL, "stats: the contig table was set again with " + std::to_string(ix->n_contigs) + " contigs, the tables were made for " + std::to_string(ix->stats_contigs));
        StatsAdd c{};
        c.res = res; c.seqs = seqs; c.offs = offs; c.n_rec = n_rec;
        c.c_off = ix->d_c_off; c.n_contigs = ix->n_contigs; c.ref_len = ix->view.ref_len;
        c.cells = ix->d_stats; c.ct = ix->d_stats + SALT_STATS_CELLS;
        c.min_mapq = ix->stats.min_mapq; c.min_tlen = pe ? pe_opt->min_tlen : 0u; c.max_tlen = pe ? pe_opt->max_tlen : 0u; c.pe = pe; c.delta = 1ull;
        if (const int rc = tally_launch(ws->stats_last, launch_stats_add, c, st)) return rc;
    }
    if (ix->indel.on) {
        if (!ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "indels: the contig table is gone (salt_gpu_index_set_contigs)");
        IndelAdd c{};
        c.res = res; c.seqs = seqs; c.offs = offs; c.n_rec = n_rec;
        c.text = ix->view.text; c.text_len = ix->view.c_seq_len; c.ref_len = ix->view.ref_len; c.c_off = ix->d_c_off; c.n_contigs = ix->n_contigs;
        c.diff = ix->d_indel_diff; c.tab = ix->d_indel; c.log2_slots = ix->indel_log2; c.stat = ix->d_indel_stat;
        c.min_mapq = ix->indel.min_mapq; c.pe = pe; c.delta = 1ull;
        if (const int rc = tally_launch(ws->indel_last, launch_indel_add, c, st)) return rc;
    }
    return SALT_OK;
}
// salt_gpu_ws_set_quals' bytes on their way into a call.  A host-buffer call copies host bytes up beside its bases (quals_upload; with the
// profile, the genotype sums and the candidate arrays off nothing is copied and they are dropped); every host-buffer or resident call then consumes the pointer (quals_take).
static int quals_upload(salt_gpu_ws_t *ws, uint64_t bases, hipStream_t st)
{
    if (!ws->q_next || ws->q_next_dev) return SALT_OK;
    if (!ws->ix->errprof.on && !ws->ix->gt.on && !ws->ix->disc.on) { ws->q_next = nullptr; return SALT_OK; }
    if (int rc = ws->d_quals.reserve(bases + 64, st)) { ws->q_next = nullptr; return rc; }
    const hipError_t e = hipMemcpyAsync(ws->d_quals, ws->q_next, bases, hipMemcpyHostToDevice, st);
    ws->q_next = ws->d_quals; ws->q_next_dev = true;
    if (e != hipSuccess) { ws->q_next = nullptr; return fail(SALT_E_HIP, std::string("hipMemcpyAsync(quality bytes): ") + hipGetErrorString(e)); }
    return SALT_OK;
}
static int quals_take(salt_gpu_ws_t *ws)
{
    ws->q_cur = {};
    const uint8_t *q = ws->q_next; ws->q_next = nullptr;
    if (!q) return SALT_OK;
    if (!ws->q_next_dev) return fail(SALT_E_INVAL, "salt_gpu_ws_set_quals: host quality bytes cannot serve a resident call (pass a device pointer, on_device = 1)");
    ws->q_cur.quals = q; ws->q_cur.bytes = ~0ull;
    return SALT_OK;
}

// ---- the workspace's buffer families: each is sized here and nowhere else ----
// The seed-interval arrays and k_seed's walk queues, for `items` seeds.  d_sai_r is zeroed when allocated: no row of any epoch (sai_r_row,
// salt_device.h).  settle: the zeroing is waited for, for a caller that does not know which stream the calls will use.  d_sai_c comes last:
// its capacity is the one compared, so a failed allocation is made up for by the next call.
static int reserve_seed(salt_gpu_ws_t *ws, uint64_t items, hipStream_t st, bool settle)
{
    if (items <= ws->d_sai_c.cap) return SALT_OK;
    HIPCHK(hipStreamSynchronize(st));
    ws->d_sai_c.release(); ws->d_sai_r.release(); ws->d_wq.release();
    HIPCHK(ws->d_sai_r.alloc(items));
    HIPCHK(hipMemsetAsync(ws->d_sai_r, 0, items * sizeof(uint4), st));
    if (settle) HIPCHK(hipStreamSynchronize(st));
    HIPCHK(ws->d_wq.alloc(seed_wq_words(items)));
    HIPCHK(ws->d_sai_c.alloc(items));
    return SALT_OK;
}

// k_pack's records of n_reads reads of geometry pg; sized for all the reads the workspace takes, so that only a longer read regrows them.
// d_heads / h_heads are sized by max_reads alone and stay (freeing them here left fetch_results with dangling pointers)
static int reserve_pack(salt_gpu_ws_t *ws, uint32_t n_reads, const PackGeom &pg, hipStream_t st)
{
    if ((uint64_t)n_reads * pg.pm_stride <= ws->d_pm.cap && (uint64_t)n_reads * pg.tb_stride <= ws->d_tb.cap) return SALT_OK;
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t nr = n_reads > ws->max_reads ? n_reads : ws->max_reads;
    ws->d_tb.release();
    HIPCHK(ws->d_pm.alloc(nr * pg.pm_stride));
    HIPCHK(ws->d_tb.alloc(nr * pg.tb_stride));
    return SALT_OK;
}

extern "C" int salt_gpu_align_se_resident(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, uint32_t n_reads, uint32_t max_read_len,
                                          const void *d_seqs, const void *d_offs, void *d_results, void *hip_stream)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    if (int rc = quals_take(ws)) return rc;
    return align_resident_impl(ws, o, n_reads, max_read_len, d_seqs, d_offs, d_results, hip_stream, 0);
}

static int align_resident_impl(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, uint32_t n_reads, uint32_t max_read_len,
                               const void *d_seqs, const void *d_offs, void *d_results, void *hip_stream, int pe)
{
    if (!ws || !o || !d_seqs || !d_offs || !d_results) return fail(SALT_E_INVAL, "null argument");
    ws->forget_last();
    if (n_reads == 0) return SALT_OK;
    uint32_t spr = 0;
    int rc = check_opt(ws->ix, o, max_read_len, &spr);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ws->ix->device));
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc2 = reserve_seed(ws, (uint64_t)n_reads * 2u * spr, st, false)) return rc2;      // grow rarely; not on the steady-state path
    const PackGeom pg = PackGeom::make(max_read_len);
    if (int rc2 = reserve_pack(ws, n_reads, pg, st)) return rc2;
    SeedParams sp; sp.pg = pg; sp.n_reads = n_reads; sp.spr = spr; sp.l_seed = o->l_seed; sp.l_overlap = o->l_overlap;
    sp.max_seed = o->max_seed; sp.seed_only_ref = o->seed_only_ref;
    sp.resolve_unique = !ws->no_unique;
    if (n_reads > ws->max_reads) return fail(SALT_E_CAPACITY, "more reads than the workspace holds");
    // R rows carry the call's epoch (sai_r_row, salt_device.h): nobody writes the dead ones.  Before the epoch restarts the array is zeroed
    // on the call's stream, in front of k_seed: a row stored 2^24 - 1 calls ago must not come back to life
    if (ws->epoch > SAI_EPOCH_MAX) { HIPCHK(hipMemsetAsync(ws->d_sai_r, 0, ws->d_sai_r.cap * sizeof(uint4), st)); ws->epoch = 1; }
    sp.epoch = ws->epoch++;
    AlignParams ap; ap.pg = pg; ap.n_reads = n_reads; ap.spr = spr; ap.l_seed = o->l_seed; ap.max_locate = o->max_locate; ap.max_hits = o->max_hits;
    ap.all_heavy = ws->all_heavy; ap.pe = pe; ap.dbg_stop = 0; ap.heavy_stop = 0; ap.max_amb = pe ? 5u : 200u; ap.epoch = sp.epoch;
#ifdef SALT_DIAG
    { const char *e = getenv("SALT_GPU_LIGHT_STOP"); ap.dbg_stop = e ? atoi(e) : 0; } { static const int hs = getenv("SALT_GPU_HEAVY_STOP") ? atoi(getenv("SALT_GPU_HEAVY_STOP")) : 0; ap.heavy_stop = hs; }
#endif
    // located rows beyond the LDS list (SALT_MAX_LOCATE) live in a global list per persistent block: paired end always may need it (0x40000
    // loci per strand, alnse.c:42,533), single end when -m is above the LDS list (the reference grows its vector, alnse.c:678, kvec.h)
    const bool glob_loci = pe || o->max_locate > SALT_MAX_LOCATE;
    if (glob_loci && !ws->d_pe_scr) HIPCHK(ws->d_pe_scr.alloc((uint64_t)ws->heavy_blocks * PE_LOCI_CAP * 5));
    unsigned long long *ctr = o->collect_counters ? ws->d_ctr.p : nullptr;
    const bool timed = ws->timing && ws->n_timed < MAX_TIMED;
    hipEvent_t *ev = timed ? &ws->ev[(size_t)ws->n_timed * EV_PER_CALL] : nullptr;
    HIPCHK(hipMemsetAsync(ws->d_zero, 0, ws->d_zero.cap, st));            // the batch's control words, k_heavy's queue ranges, the walk queues' counters
    if (timed) HIPCHK(hipEventRecord(ev[0], st));
    launch_pack(pg, n_reads, static_cast<const uint8_t *>(d_seqs), static_cast<const uint32_t *>(d_offs), ws->d_pm, ws->d_tb, st);
    if (timed) HIPCHK(hipEventRecord(ev[1], st));
    launch_seed(ws->ix->view, sp, ws->d_tb, ws->d_sai_c, ws->d_sai_r, reinterpret_cast<uint4 *>(ws->d_wq.p), ws->d_wq_cnt, ws->walk_blocks, ctr, st);
    if (timed) HIPCHK(hipEventRecord(ev[2], st));
    if (!ap.all_heavy)
        launch_light(ws->ix->view, ap, ws->d_pm, static_cast<const uint8_t *>(d_seqs), static_cast<const uint32_t *>(d_offs), ws->d_sai_c, ws->d_sai_r,
                     static_cast<salt_result_t *>(d_results), ws->d_queue, ws->d_qctl, ws->d_queue + 2 * (size_t)ws->max_reads, ws->d_ranges, ctr, st);
    if (timed) HIPCHK(hipEventRecord(ev[3], st));
    launch_heavy(ws->ix->view, ap, ws->d_pm, ws->d_sai_c, ws->d_sai_r,
                 static_cast<salt_result_t *>(d_results), ws->d_queue, ctr, ws->heavy_blocks, ws->gap_blocks, ws->cigar_blocks, ws->d_lvtab,
                 gap_bufs_layout(ws->d_gap, ws->gcap, ws->d_qctl, nullptr), ws->d_queue + ws->max_reads, ws->d_ranges, glob_loci ? ws->d_pe_scr.p : nullptr, timed ? ev + 4 : nullptr, st);
    if (timed) { HIPCHK(hipEventRecord(ev[7], st)); ws->ev_pe[ws->n_timed] = 0; ++ws->n_timed; }
    HIPCHK(hipGetLastError());
    if (!pe) return rows_hooks(ws, n_reads, d_seqs, d_offs, d_results, nullptr, st);
    return SALT_OK;
}

// Results to host memory without moving 880 bytes per read over PCIe: nearly every row is fully described by its first
// 128 bytes (header, hits, hit_n_cigar, the first 8 CIGAR ops); those travel as one dense copy, the few rows with longer
// or alternative-hit CIGARs are fetched whole.
static const uint32_t HEAD_BYTES = 128;
static_assert(offsetof(salt_result_t, cigar) + 8 * sizeof(uint16_t) == HEAD_BYTES, "result head");
static int fetch_results(salt_gpu_ws_t *ws, uint32_t n_reads, salt_result_t *results, hipStream_t st)
{
    if (!ws->d_heads) {
        HIPCHK(ws->h_heads.alloc((uint64_t)ws->max_reads * HEAD_BYTES));
        HIPCHK(ws->d_heads.alloc((uint64_t)ws->max_reads * HEAD_BYTES));
    }
    launch_heads(ws->d_results, n_reads, ws->d_heads, st);
    HIPCHK(hipMemcpyAsync(ws->h_heads, ws->d_heads, (uint64_t)n_reads * HEAD_BYTES, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // heads -> rows: 128 bytes into every 880-byte row (two cache lines of a strided 88 MB per 100 000 reads); big batches are
    // split over a few threads, the caller's thread among them
    std::vector<uint32_t> full;
    const uint32_t n_thr = n_reads >= 262144 ? 4u : 1u;        // a driver with 100 000-read batches (salt) runs several workers already
    std::vector<std::vector<uint32_t>> full_t(n_thr);
    auto scatter = [&](uint32_t t) {
        const uint32_t lo = (uint32_t)((uint64_t)n_reads * t / n_thr), hi = (uint32_t)((uint64_t)n_reads * (t + 1) / n_thr);
        for (uint32_t i = lo; i < hi; ++i) {
            memcpy(&results[i], ws->h_heads + (uint64_t)i * HEAD_BYTES, HEAD_BYTES);
            const salt_result_t &r = results[i];
            bool more = r.n_cigar > 8;
            for (int h = 0; h < SALT_MAX_HITS; ++h) more |= r.hit_n_cigar[h] != 0;
            if (more) full_t[t].push_back(i);
        }
    };
    {
        std::vector<std::thread> th;
        for (uint32_t t = 1; t < n_thr; ++t) th.emplace_back(scatter, t);
        scatter(0);
        for (auto &x : th) x.join();
    }
    for (auto &v : full_t) full.insert(full.end(), v.begin(), v.end());
    if (full.size() > 4096) {                                  // unusual batch: one plain copy is cheaper than thousands of small ones
        HIPCHK(hipMemcpyAsync(results, ws->d_results, (uint64_t)n_reads * sizeof(salt_result_t), hipMemcpyDeviceToHost, st));
    } else {
        for (uint32_t i : full) HIPCHK(hipMemcpyAsync(&results[i], ws->d_results + i, sizeof(salt_result_t), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return SALT_OK;
}

extern "C" int salt_gpu_align_se(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, uint32_t n_reads, const uint8_t *seqs,
                                 const uint32_t *offs, salt_result_t *results)
{
    if (!ws || !o || !seqs || !offs || !results) return fail(SALT_E_INVAL, "null argument");
    if (n_reads == 0) return SALT_OK;
    if (n_reads > ws->max_reads) return fail(SALT_E_CAPACITY, "more reads than the workspace holds");
    if (offs[0] != 0) return fail(SALT_E_INVAL, "offs[0] must be 0");
    uint64_t bases = offs[n_reads];
    if (bases > ws->max_bases) return fail(SALT_E_CAPACITY, "more bases than the workspace holds");
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n_reads; ++i) {
        if (offs[i + 1] < offs[i]) return fail(SALT_E_INVAL, "offs must be non-decreasing");
        uint32_t l = offs[i + 1] - offs[i];
        if (l == 0) return fail(SALT_E_INVAL, "empty read");
        max_len = l > max_len ? l : max_len;
    }
    HIPCHK(hipSetDevice(ws->ix->device));
    HIPCHK(hipMemcpyAsync(ws->d_seqs, seqs, bases, hipMemcpyHostToDevice, ws->stream));
    HIPCHK(hipMemcpyAsync(ws->d_offs, offs, ((uint64_t)n_reads + 1) * 4, hipMemcpyHostToDevice, ws->stream));
    if (int rc2 = quals_upload(ws, bases, ws->stream)) return rc2;
    int rc = salt_gpu_align_se_resident(ws, o, n_reads, max_len, ws->d_seqs, ws->d_offs, ws->d_results, ws->stream);
    if (rc) return rc;
    return fetch_results(ws, n_reads, results, ws->stream);
}

// ---------------------------------------------------------------------------------------------
// FASTQ text in, SAM text out
// ---------------------------------------------------------------------------------------------
extern "C" int salt_gpu_index_set_contigs(salt_gpu_index_t *ix, int32_t n, const int64_t *offsets, const char *const *names)
{
    if (!ix || n <= 0 || !offsets || !names) return fail(SALT_E_INVAL, "bad contig table");
    HIPCHK(hipSetDevice(ix->device));
    std::vector<uint32_t> noff((size_t)n + 1, 0); std::string blob;
    for (int i = 0; i < n; ++i) { if (!names[i]) return fail(SALT_E_INVAL, "contig without a name"); blob += names[i]; noff[(size_t)i + 1] = (uint32_t)blob.size(); }
    if (ix->d_c_off) { hipFree(ix->d_c_off); hipFree(ix->d_c_name_off); hipFree(ix->d_c_names); ix->d_c_off = nullptr; ix->d_c_name_off = nullptr; ix->d_c_names = nullptr; ix->n_contigs = 0; }
    HIPCHK(hipMalloc((void **)&ix->d_c_off, (size_t)n * 8));
    HIPCHK(hipMalloc((void **)&ix->d_c_name_off, ((size_t)n + 1) * 4));
    HIPCHK(hipMalloc((void **)&ix->d_c_names, blob.size() + 1));
    HIPCHK(hipMemcpy(ix->d_c_off, offsets, (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_c_name_off, noff.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ix->d_c_names, blob.data(), blob.size(), hipMemcpyHostToDevice));
    ix->n_contigs = n;
    ix->h_c_off.assign(offsets, offsets + n); ix->c_name_max = 0;
    for (int i = 0; i < n; ++i) ix->c_name_max = std::max<uint32_t>(ix->c_name_max, noff[(size_t)i + 1] - noff[(size_t)i]);
    HIPCHK(text_warm());                                     // the text kernels' code object is loaded now, not inside the first block's call
    return SALT_OK;
}

extern "C" int salt_gpu_host_alloc(uint64_t bytes, void **ptr)
{
    if (!ptr || !bytes) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    return SALT_OK;
}
extern "C" void salt_gpu_host_free(void *ptr) { if (ptr) hipHostFree(ptr); }

// The host NUMA node a device hangs off (its PCI function's numa_node in sysfs); -1 when the platform does not say.  A multi-GPU driver pins
// each device's worker threads -- and allocates their page-locked buffers from them -- on that node: the reads' and the SAM text's DMA then
// stays on the socket the GPU is attached to.
extern "C" int salt_gpu_device_numa_node(int device, int *node)
{
    if (!node) return fail(SALT_E_INVAL, "null argument");
    *node = -1;
    char bus[64] = { 0 };
    HIPCHK(hipDeviceGetPCIBusId(bus, (int)sizeof bus, device));
    for (char *c = bus; *c; ++c) *c = (char)tolower((unsigned char)*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    if (FILE *f = fopen(path.c_str(), "r")) { int v = -1; if (fscanf(f, "%d", &v) == 1) *node = v; fclose(f); }
    return SALT_OK;
}
extern "C" int salt_gpu_device_count(int *n)
{
    if (!n) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipGetDeviceCount(n));
    return SALT_OK;
}

// The raw block and what follows its capacity: the newline counters of its tiles (two blocks' counters lie 4 words apart, and the paired-end
// entry rounds both up: TILE_SLACK covers either entry, so a workspace reserved once serves both) and the scan scratch.  d_tctl is the
// parse control words | the SAM block's byte count in 64 bits | k_bam_len's error word.
static const uint64_t TILE_SLACK = 16;
static int reserve_parse(salt_gpu_ws_t *ws, uint64_t raw_bytes, hipStream_t st)
{
    if (int rc = ws->d_raw.reserve(raw_bytes + 64, st)) return rc;
    if (!ws->d_tctl) HIPCHK(ws->d_tctl.alloc(8));
    if (int rc = ws->d_tile.reserve(ws->d_raw.cap / FQ_TILE + TILE_SLACK, st)) return rc;
    const size_t need = text_scan_bytes(std::max<uint64_t>(ws->d_tile.cap, (uint64_t)ws->max_reads + 2));
    if (need > ws->d_scan.cap) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(ws->d_scan.alloc(need)); }
    return SALT_OK;
}

// The codes of the block's reads; max_bases is what the resident entry points compare with
static int reserve_seqs(salt_gpu_ws_t *ws, uint64_t bases, hipStream_t st)
{
    if (bases <= ws->max_bases) return SALT_OK;
    HIPCHK(hipStreamSynchronize(st));
    ws->max_bases = 0;
    HIPCHK(ws->d_seqs.alloc(bases + bases / 4 + 64));
    ws->max_bases = bases + bases / 4;
    return SALT_OK;
}

// What the record kernels keep per read between their length pass and their write pass: sized once, by max_reads
static int reserve_records(salt_gpu_ws_t *ws)
{
    if (!ws->d_rec) HIPCHK(ws->d_rec.alloc(ws->max_reads));
    if (!ws->d_samoff) HIPCHK(ws->d_samoff.alloc((uint64_t)ws->max_reads + 2));
    if (!ws->d_samslot) HIPCHK(ws->d_samslot.alloc((uint64_t)ws->max_reads * SAM_SLOT));
    if (!ws->d_samseg) HIPCHK(ws->d_samseg.alloc(ws->max_reads));
    return SALT_OK;
}

// The output block on the device and its page-locked twin: `want` bytes of each when they hold fewer than `need`.  The callers have read the
// block's length back (or have queued nothing yet), so nothing on the stream uses the old ones.  host, when it holds `want` bytes, is the
// caller's page-locked buffer and serves as the twin.  d_sam comes last: its capacity is the one compared.
static int reserve_sam(salt_gpu_ws_t *ws, uint64_t need, uint64_t want, void *host, uint64_t host_bytes)
{
    if (need <= ws->d_sam.cap) return SALT_OK;
    ws->d_sam.release();
    if (host && host_bytes >= want) ws->h_sam.adopt(static_cast<char *>(host), want);
    else HIPCHK(ws->h_sam.alloc(want));
    HIPCHK(ws->d_sam.alloc(want));
    return SALT_OK;
}

// Sizes every buffer a text call of up to max_block_bytes / est_reads reads of max_read_len bases will ask for, so that the first call
// on the workspace finds them (a later, larger block still regrows them).  One-time work a driver does next to attaching the index.
extern "C" int salt_gpu_ws_reserve_text(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, uint64_t max_block_bytes, uint32_t est_reads, uint32_t max_read_len,
                                        uint64_t est_sam_bytes, void *host_sam, uint64_t host_sam_bytes)
{
    if (!ws || !o || max_block_bytes == 0 || est_reads == 0) return fail(SALT_E_INVAL, "bad reserve arguments");
    if (est_reads > ws->max_reads) est_reads = ws->max_reads;
    uint32_t spr = 0;
    int rc = check_opt(ws->ix, o, max_read_len, &spr);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ws->ix->device));
    hipStream_t st = ws->stream;
    if ((rc = reserve_parse(ws, max_block_bytes, st))) return rc;
    if ((rc = ws->d_lines.reserve(4ull * est_reads + 8, st))) return rc;
    if ((rc = reserve_records(ws))) return rc;
    if ((rc = reserve_seed(ws, (uint64_t)est_reads * 2u * spr, st, true))) return rc;      // settled: whichever stream the calls use
    if ((rc = reserve_pack(ws, ws->max_reads, PackGeom::make(max_read_len), st))) return rc;
    if (host_sam && host_sam_bytes > est_sam_bytes + 64) est_sam_bytes = host_sam_bytes - 64;
    return reserve_sam(ws, est_sam_bytes + 64, est_sam_bytes + 64, host_sam, host_sam_bytes);
}

// ---- BGZF: the SAM block deflated on the device, behind k_sam_write on the same stream ----
// The deflate kernels' buffers for n_blocks blocks; sizes comes last: its capacity is the block count a caller compares
static hipError_t bgzf_bufs_alloc(DevBuf<uint32_t> &slots, DevBuf<uint32_t> &sizes, DevBuf<unsigned long long> &offs, DevBuf<uint8_t> &out, uint64_t n_blocks)
{
    hipError_t e;
    slots.release(); sizes.release(); offs.release(); out.release();
    if ((e = slots.alloc(n_blocks * (BGZF_SLOT_BYTES / 4))) != hipSuccess) return e;
    if ((e = offs.alloc(n_blocks + 1)) != hipSuccess) return e;
    if ((e = out.alloc(n_blocks * (BGZF_CUT_BYTES + 31))) != hipSuccess) return e;      // bgzf_bound of n_blocks full blocks
    return sizes.alloc(n_blocks);
}

// ws->d_sam[0 .. total) -> whole BGZF blocks in page-locked host memory (*sam, *sam_bytes); no end-of-file block
static int ws_sam_bgzf(salt_gpu_ws_t *ws, uint64_t total, hipStream_t st, const char **sam, uint64_t *sam_bytes)
{
    const uint64_t n_blocks = bgzf_blocks(total);
    if (n_blocks > ws->d_bz_sizes.cap) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(bgzf_bufs_alloc(ws->d_bz_slots, ws->d_bz_sizes, ws->d_bz_offs, ws->d_bz_out, n_blocks + n_blocks / 4 + 1));
    }
    HIPCHK(launch_bgzf_deflate(reinterpret_cast<const uint8_t *>(ws->d_sam.p), total, ws->d_bz_slots, ws->d_bz_sizes, ws->d_bz_offs, ws->d_bz_out, st));
    unsigned long long bytes = 0;
    HIPCHK(hipMemcpyAsync(&bytes, ws->d_bz_offs + n_blocks, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (bytes > bgzf_bound(total)) return fail(SALT_E_HIP, "BGZF blocks larger than their bound");
    char *dst = ws->h_sam;
    if (bytes > ws->h_sam.cap) {                             // incompressible text: up to 31 bytes per block more than the text the SAM buffers were sized for
        if (bytes > ws->h_bz.cap) HIPCHK(ws->h_bz.alloc(bytes + bytes / 4));
        dst = ws->h_bz;
    }
    HIPCHK(hipMemcpyAsync(dst, ws->d_bz_out, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *sam = dst; *sam_bytes = bytes;
    return SALT_OK;
}

extern "C" int salt_gpu_ws_set_sam_bgzf(salt_gpu_ws_t *ws, int on)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    ws->sam_bgzf = on != 0;
    return SALT_OK;
}

static const char *const POLISH_BAM_ERROR = "polished records cannot be written as BAM: salt_gpu_ws_set_polish and salt_gpu_ws_set_sam_bam exclude each other";

extern "C" int salt_gpu_ws_set_sam_bam(salt_gpu_ws_t *ws, int on)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    if (on && ws->polish) return fail(SALT_E_INVAL, POLISH_BAM_ERROR);
    ws->sam_bam = on != 0;
    return SALT_OK;
}

extern "C" int salt_gpu_ws_set_polish(salt_gpu_ws_t *ws, int mode)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    if (mode < 0 || mode > 2) return fail(SALT_E_INVAL, "polish mode: 0 off, 1 Landau-Vishkin, 2 Smith-Waterman");
    if (mode) {
        if (ws->sam_bam) return fail(SALT_E_INVAL, POLISH_BAM_ERROR);
        if (!ws->ix->d_pac) return fail(SALT_E_INVAL, "polish needs the 2-bit genome: call salt_gpu_index_set_pac first");
        if (!ws->ix->d_c_off || ws->ix->n_contigs < 1) return fail(SALT_E_INVAL, "polish needs the contig table: call salt_gpu_index_set_contigs first");
    }
    ws->polish = mode;
    return SALT_OK;
}

static constexpr uint32_t TRIM_CNT_WORDS = 2 * TRIM_N_COUNTS + TRIM_PAIR_N_COUNTS;      // d_trim_cnt: the sixteen, then the eight of the pairs

extern "C" int salt_gpu_ws_set_trim(salt_gpu_ws_t *ws, const salt_trim_opt_t *o)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    TrimRule r{};
    if (o) if (const char *what = trim_rule_make(o->adapter, o->adapter_len, o->adapter2, o->adapter2_len, o->front, o->tail, o->qual, o->min_overlap, o->error_pct, &r))
        return fail(SALT_E_INVAL, what);
    if (trim_rule_on(r) && !ws->d_trim_cnt) {
        HIPCHK(hipSetDevice(ws->ix->device));
        HIPCHK(ws->d_trim_cnt.alloc(TRIM_CNT_WORDS));
    }
    ws->trim_rule = r; ws->trim = trim_rule_on(r);
    return SALT_OK;
}

extern "C" int salt_gpu_ws_set_trim_pair(salt_gpu_ws_t *ws, const salt_trim_pair_opt_t *o)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    TrimPairRule p{};
    if (o) if (const char *what = trim_pair_rule_make(o->min_overlap, o->error_pct, &p)) return fail(SALT_E_INVAL, what);
    if (trim_pair_on(p) && !ws->d_trim_cnt) {
        HIPCHK(hipSetDevice(ws->ix->device));
        HIPCHK(ws->d_trim_cnt.alloc(TRIM_CNT_WORDS));
    }
    ws->trim_pair = p;
    return SALT_OK;
}

extern "C" int salt_gpu_ws_trim_pair_counts(salt_gpu_ws_t *ws, uint64_t out[8], int reset)
{
    if (!ws || !out) return fail(SALT_E_INVAL, "null argument");
    memcpy(out, ws->trim_pair_total, sizeof ws->trim_pair_total);
    if (reset) memset(ws->trim_pair_total, 0, sizeof ws->trim_pair_total);
    return SALT_OK;
}

extern "C" int salt_gpu_ws_trim_counts(salt_gpu_ws_t *ws, uint64_t out[16], int reset)
{
    if (!ws || !out) return fail(SALT_E_INVAL, "null argument");
    memcpy(out, ws->trim_total, sizeof ws->trim_total);          // every finished call has added its block already
    if (reset) memset(ws->trim_total, 0, sizeof ws->trim_total);
    return SALT_OK;
}

extern "C" int salt_gpu_ws_trim_uncount(salt_gpu_ws_t *ws)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    for (uint32_t k = 0; k < 2 * TRIM_N_COUNTS; ++k) ws->trim_total[k] -= ws->trim_last[k];
    memset(ws->trim_last, 0, sizeof ws->trim_last);
    for (uint32_t k = 0; k < TRIM_PAIR_N_COUNTS; ++k) ws->trim_pair_total[k] -= ws->trim_pair_last[k];
    memset(ws->trim_pair_last, 0, sizeof ws->trim_pair_last);
    return SALT_OK;
}

// k_fq_trim behind the parse kernels of a call, its counters zeroed in front of it
static int ws_trim_launch(salt_gpu_ws_t *ws, uint64_t n_raw, uint32_t n_rec, int pe, uint32_t mate, uint32_t *spans, hipStream_t st)
{
    if (!ws->d_trim_cnt) HIPCHK(ws->d_trim_cnt.alloc(TRIM_CNT_WORDS));
    HIPCHK(hipMemsetAsync(ws->d_trim_cnt, 0, 2 * TRIM_N_COUNTS * 8, st));
    HIPCHK(launch_fq_trim(ws->d_raw, n_raw, ws->d_rec, ws->d_offs, n_rec, pe, mate, ws->trim_rule, ws->d_tctl, ws->d_trim_cnt, spans, st));
    return SALT_OK;
}
// k_fq_trim_pair in its place: the pair rule is on.  n_rec = both mates of every pair.
static int ws_trim_pair_launch(salt_gpu_ws_t *ws, uint64_t n_raw, uint32_t n_rec, uint32_t *spans, hipStream_t st)
{
    if (!ws->d_trim_cnt) HIPCHK(ws->d_trim_cnt.alloc(TRIM_CNT_WORDS));
    HIPCHK(hipMemsetAsync(ws->d_trim_cnt, 0, TRIM_CNT_WORDS * 8, st));
    HIPCHK(launch_fq_trim_pair(ws->d_raw, n_raw, ws->d_rec, ws->d_offs, n_rec / 2, ws->trim_rule, ws->trim_pair, ws->d_tctl, ws->d_trim_cnt,
                               ws->d_trim_cnt + 2 * TRIM_N_COUNTS, spans, st));
    return SALT_OK;
}
// blk: the sixteen, and with pair the eight behind them
static void ws_trim_add(salt_gpu_ws_t *ws, const uint64_t *blk, bool pair = false)
{
    for (uint32_t k = 0; k < 2 * TRIM_N_COUNTS; ++k) { ws->trim_total[k] += blk[k]; ws->trim_last[k] = blk[k]; }
    if (pair) for (uint32_t k = 0; k < TRIM_PAIR_N_COUNTS; ++k) { ws->trim_pair_total[k] += blk[2 * TRIM_N_COUNTS + k]; ws->trim_pair_last[k] = blk[2 * TRIM_N_COUNTS + k]; }
}

// The polish stage of a text call, where the SAM kernels run without it: the block's records from its result rows (polish_rows_len: all but
// the bytes; *total = how many they are), then -- the caller has made room in ws->d_sam -- polish_rows_write.
static int ws_polish_len(salt_gpu_ws_t *ws, uint32_t n_rec, uint32_t max_len, int paired, hipStream_t st, uint64_t *total)
{
    salt_gpu_index *ix = ws->ix;
    if (!ix->d_pac || !ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "polish needs the 2-bit genome and the contig table (salt_gpu_index_set_pac, salt_gpu_index_set_contigs)");
    if (!ws->pl) ws->pl = polish_text_new();
    if (!ws->d_pl_tabs) {
        int cus = 0;
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix->device));
        ws->pl_blocks = (uint32_t)cus * 8u;
        HIPCHK(ws->d_pl_tabs.alloc((uint64_t)ws->pl_blocks * lv_table_bytes()));
    }
    PolishRows in;
    in.raw = ws->d_raw; in.fq = ws->d_rec; in.codes = ws->d_seqs; in.offs = ws->d_offs; in.res = ws->d_results; in.n_rec = n_rec; in.max_len = max_len;
    in.c_off = ix->d_c_off; in.c_name_off = ix->d_c_name_off; in.c_names = ix->d_c_names; in.n_contigs = ix->n_contigs;
    in.pac = ix->d_pac; in.l_pac = ix->l_pac; in.tabs = ws->d_pl_tabs; in.n_blocks = ws->pl_blocks; in.paired = paired; in.use_sw = ws->polish == 2; in.st = st;
    std::string err;
    const int rc = polish_rows_len(ws->pl, in, total, err);
    return rc ? fail(rc, err) : SALT_OK;
}
static int ws_polish_write(salt_gpu_ws_t *ws, hipStream_t st)
{
    std::string err;
    const int rc = polish_rows_write(ws->pl, ws->d_sam, st, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_bgzf_deflate(int device, const void *text, uint64_t n_bytes, void *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!out_bytes || (n_bytes && (!text || !out))) return fail(SALT_E_INVAL, "null argument");
    *out_bytes = 0;
    if (n_bytes == 0) return SALT_OK;
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (n_dev <= 0) return fail(SALT_E_HIP, "no HIP device visible: the BGZF kernels cannot run (there is no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    const uint64_t n_blocks = bgzf_blocks(n_bytes);
    DevBuf<uint32_t> slots, sizes; DevBuf<unsigned long long> offs; DevBuf<uint8_t> blocks, d_text;      // freed on every return
    HIPCHK(bgzf_bufs_alloc(slots, sizes, offs, blocks, n_blocks));
    HIPCHK(d_text.alloc(n_bytes + 64));
    HIPCHK(hipMemcpy(d_text, text, n_bytes, hipMemcpyHostToDevice));
    HIPCHK(launch_bgzf_deflate(d_text, n_bytes, slots, sizes, offs, blocks, nullptr));
    unsigned long long bytes = 0;
    HIPCHK(hipMemcpy(&bytes, offs + n_blocks, 8, hipMemcpyDeviceToHost));
    if (bytes > bgzf_bound(n_bytes)) return fail(SALT_E_HIP, "BGZF blocks larger than their bound");
    if (bytes > out_cap) return fail(SALT_E_CAPACITY, "output buffer smaller than the BGZF blocks (" + std::to_string(bytes) + " bytes; 65536 per block always suffice)");
    HIPCHK(hipMemcpy(out, blocks, bytes, hipMemcpyDeviceToHost));
    *out_bytes = bytes;
    return SALT_OK;
}

// ---- BGZF input: members inflated on the device ----
static int inflate_status(const uint32_t *status, uint64_t n_blocks)
{
    for (uint64_t b = 0; b < n_blocks; ++b)
        if (status[b]) return fail(SALT_E_DATA, "BGZF member " + std::to_string(b) + ": " + bgzf::inflate_reason(status[b]));
    return SALT_OK;
}

extern "C" int salt_gpu_bgzf_inflate(int device, const void *bgzf_, uint64_t n_bytes, void *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!out_bytes || (n_bytes && !bgzf_)) return fail(SALT_E_INVAL, "null argument");
    *out_bytes = 0;
    if (n_bytes == 0) return SALT_OK;
    // the members, by their BSIZE fields; the text offsets, by their ISIZE fields
    const uint8_t *z = static_cast<const uint8_t *>(bgzf_);
    std::vector<unsigned long long> c_off, u_off;
    uint64_t at = 0, u = 0;
    while (at < n_bytes) {
        const uint8_t *h = z + at;
        uint64_t bsize = 0;
        if (n_bytes - at >= 18 && h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && h[3] == 4) {
            const uint32_t xlen = h[10] | h[11] << 8;
            for (uint32_t p = 12; p + 4 <= 12 + xlen && at + p + 6 <= n_bytes; ) {
                const uint32_t slen = h[p + 2] | h[p + 3] << 8;
                if (h[p] == 'B' && h[p + 1] == 'C' && slen == 2) { bsize = (h[p + 4] | h[p + 5] << 8) + 1u; break; }
                p += 4 + slen;
            }
        }
        if (bsize < 26 || bsize > n_bytes - at)
            return fail(SALT_E_DATA, "BGZF member " + std::to_string(c_off.size()) + ": " + (bsize ? "its BSIZE points past the end of the data" : bgzf::inflate_reason(bgzf::INFL_E_HEADER)));
        const uint8_t *t = h + bsize - 4;
        const uint32_t isize = t[0] | t[1] << 8 | t[2] << 16 | (uint32_t)t[3] << 24;
        if (isize > bgzf::INFL_MAX) return fail(SALT_E_DATA, "BGZF member " + std::to_string(c_off.size()) + ": " + bgzf::inflate_reason(bgzf::INFL_E_SIZE));
        c_off.push_back(at); u_off.push_back(u);
        at += bsize; u += isize;
    }
    const uint64_t n_blocks = c_off.size();
    c_off.push_back(at); u_off.push_back(u);
    *out_bytes = u;
    if (u > out_cap) return fail(SALT_E_CAPACITY, "output buffer smaller than the text (" + std::to_string(u) + " bytes)");
    if (u && !out) return fail(SALT_E_INVAL, "null argument");
    if (n_blocks > 0x7FFFFFFFull) return fail(SALT_E_CAPACITY, "more than 2^31 BGZF members in one call");
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (n_dev <= 0) return fail(SALT_E_HIP, "no HIP device visible: the BGZF kernels cannot run (there is no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    DevBuf<uint8_t> d_in, d_out; DevBuf<unsigned long long> d_off; DevBuf<uint32_t> d_stat;      // freed on every return
    HIPCHK(d_in.alloc(n_bytes + 64));
    HIPCHK(d_out.alloc(u + 64));
    HIPCHK(d_off.alloc(2 * (n_blocks + 1)));
    HIPCHK(d_stat.alloc(n_blocks));
    HIPCHK(hipMemcpy(d_in, z, n_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off, c_off.data(), (n_blocks + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_off + n_blocks + 1, u_off.data(), (n_blocks + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(launch_bgzf_inflate(d_in, d_off, d_off + n_blocks + 1, (uint32_t)n_blocks, d_out, d_stat, nullptr));
    std::vector<uint32_t> status(n_blocks);
    HIPCHK(hipMemcpy(status.data(), d_stat, n_blocks * 4, hipMemcpyDeviceToHost));
    if (int rc = inflate_status(status.data(), n_blocks)) { *out_bytes = 0; return rc; }
    if (u) HIPCHK(hipMemcpy(out, d_out, u, hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_ws_inflate_bgzf(salt_gpu_ws_t *ws, const void *blocks, uint64_t n_cbytes, uint32_t n_blocks, const uint32_t *c_off, const uint32_t *u_off)
{
    if (!ws || (n_blocks && (!blocks || !c_off || !u_off))) return fail(SALT_E_INVAL, "null argument");
    ws->text_bytes = 0;
    if (n_blocks == 0) return SALT_OK;
    if (n_blocks > 0x7FFFFFFFu || c_off[0] != 0 || u_off[0] != 0 || c_off[n_blocks] > n_cbytes) return fail(SALT_E_INVAL, "bad BGZF member offsets");
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (c_off[b + 1] < c_off[b] || u_off[b + 1] < u_off[b]) return fail(SALT_E_INVAL, "bad BGZF member offsets");
    HIPCHK(hipSetDevice(ws->ix->device));
    hipStream_t st = ws->stream;
    const uint64_t n_text = u_off[n_blocks];
    if (int rc = ws->d_zin.reserve((uint64_t)c_off[n_blocks] + 64, st)) return rc;
    if (int rc = ws->d_text.reserve(n_text + 64, st)) return rc;
    if (n_blocks > ws->d_zstat.cap) {                        // d_zstat last: its capacity is the one compared
        HIPCHK(hipStreamSynchronize(st));
        const uint64_t want = (uint64_t)n_blocks + n_blocks / 4 + 1;
        ws->d_zstat.release();
        HIPCHK(ws->d_zoff.alloc(2 * (want + 1)));
        HIPCHK(ws->d_zstat.alloc(want));
    }
    ws->h_zoff.resize(2 * ((size_t)n_blocks + 1)); ws->h_zstat.resize(n_blocks);
    for (uint32_t b = 0; b <= n_blocks; ++b) { ws->h_zoff[b] = c_off[b]; ws->h_zoff[(size_t)n_blocks + 1 + b] = u_off[b]; }
    HIPCHK(hipMemcpyAsync(ws->d_zin, blocks, c_off[n_blocks], hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws->d_zoff, ws->h_zoff.data(), ws->h_zoff.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(launch_bgzf_inflate(ws->d_zin, ws->d_zoff, ws->d_zoff + n_blocks + 1, n_blocks, ws->d_text, ws->d_zstat, st));
    HIPCHK(hipMemcpyAsync(ws->h_zstat.data(), ws->d_zstat, (uint64_t)n_blocks * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = inflate_status(ws->h_zstat.data(), n_blocks)) return rc;
    ws->text_bytes = n_text;
    return SALT_OK;
}

extern "C" int salt_gpu_ws_text_peek(salt_gpu_ws_t *ws, uint64_t off, uint64_t n, void *dst)
{
    if (!ws || (n && !dst)) return fail(SALT_E_INVAL, "null argument");
    if (off > ws->text_bytes || n > ws->text_bytes - off) return fail(SALT_E_INVAL, "range outside the inflated text");
    if (n == 0) return SALT_OK;
    HIPCHK(hipSetDevice(ws->ix->device));
    HIPCHK(hipMemcpyAsync(dst, ws->d_text + off, n, hipMemcpyDeviceToHost, ws->stream));
    HIPCHK(hipStreamSynchronize(ws->stream));
    return SALT_OK;
}

// The text entry points behind their arguments: the block comes from the host (fastq) or from the workspace's inflated text (d_src, with
// a newline put behind it when add_newline); everything behind the copy-in is one body.
static int se_text_impl(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_text_opt_t *to, const char *fastq, const uint8_t *d_src, uint64_t n_bytes, int add_newline,
                        const char **sam, uint64_t *sam_bytes, uint32_t *n_reads);

extern "C" int salt_gpu_align_se_text(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_text_opt_t *to, const char *fastq, uint64_t n_bytes,
                                      const char **sam, uint64_t *sam_bytes, uint32_t *n_reads)
{
    if (!ws || !o || !to || !fastq || !sam || !sam_bytes || !n_reads) return fail(SALT_E_INVAL, "null argument");
    *sam = nullptr; *sam_bytes = 0; *n_reads = 0;
    if (n_bytes == 0) return SALT_OK;
    if (n_bytes >= 0xFFFFFFF0ull) return fail(SALT_E_CAPACITY, "FASTQ block of 4 GiB or more");
    if (fastq[n_bytes - 1] != '\n') return fail(SALT_E_INVAL, "FASTQ block must end with a newline");
    return se_text_impl(ws, o, to, fastq, nullptr, n_bytes, 0, sam, sam_bytes, n_reads);
}

extern "C" int salt_gpu_align_se_text_dev(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_text_opt_t *to, uint64_t off, uint64_t n_bytes, int add_newline,
                                          const char **sam, uint64_t *sam_bytes, uint32_t *n_reads)
{
    if (!ws || !o || !to || !sam || !sam_bytes || !n_reads) return fail(SALT_E_INVAL, "null argument");
    *sam = nullptr; *sam_bytes = 0; *n_reads = 0;
    if (off > ws->text_bytes || n_bytes > ws->text_bytes - off) return fail(SALT_E_INVAL, "range outside the inflated text");
    if (n_bytes == 0) return SALT_OK;
    if (n_bytes >= 0xFFFFFFF0ull) return fail(SALT_E_CAPACITY, "FASTQ block of 4 GiB or more");
    if (!add_newline) {
        char last = 0;
        if (int rc = salt_gpu_ws_text_peek(ws, off + n_bytes - 1, 1, &last)) return rc;
        if (last != '\n') return fail(SALT_E_INVAL, "FASTQ block must end with a newline");
    }
    return se_text_impl(ws, o, to, nullptr, ws->d_text + off, n_bytes, add_newline, sam, sam_bytes, n_reads);
}

static int pe_resident_impl(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_pe_opt_t *pe, uint32_t n_pairs, uint32_t max_len,
                            const void *d_seqs, const void *d_offs, void *d_results, hipStream_t st);

// SALT_TEXT_TRACE: the stage clocks of a workspace's first single-end text call
struct TextTrace {
    bool on = false; double tm[8]; int n = 0;
    void mark() { if (on && n < 8) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); tm[n++] = (double)ts.tv_sec + ts.tv_nsec * 1e-9; } }
};

// Behind the parse kernels: their control words back (ctl[0] what is wrong, ctl[2] where; ctl[1] = *max_len, the longest read), then the reads'
// codes.  blocks: "block" or "blocks", as the entry point takes one or two.
static int text_codes(salt_gpu_ws_t *ws, uint32_t n_rec, const char *blocks, hipStream_t st, uint32_t *max_len, bool pair = false)
{
    uint32_t ctl[4] = { 0, 0, 0, 0 }, bases = 0; uint64_t trimmed[TRIM_CNT_WORDS];
    const bool trim = ws->trim || pair;                            // pair: k_fq_trim_pair ran, its eight counters lie behind the sixteen
    HIPCHK(hipMemcpyAsync(ctl, ws->d_tctl, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&bases, ws->d_offs + n_rec, 4, hipMemcpyDeviceToHost, st));
    if (trim) HIPCHK(hipMemcpyAsync(trimmed, ws->d_trim_cnt, (pair ? TRIM_CNT_WORDS : 2 * TRIM_N_COUNTS) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ctl[0]) {
        const char *what = ctl[0] & 1 ? "a record does not start with '@'" : ctl[0] & 2 ? "the third line of a record does not start with '+'"
                         : ctl[0] & 4 ? "sequence and quality lengths differ" : "empty read";
        return fail(SALT_E_INVAL, std::string("input is not 4-line FASTQ at record ") + std::to_string(ctl[2]) + " of the " + blocks + ": " + what);
    }
    if (trim) ws_trim_add(ws, trimmed, pair);
    if (int rc = reserve_seqs(ws, bases, st)) return rc;
    HIPCHK(launch_fq_codes(ws->d_raw, ws->d_rec, ws->d_offs, n_rec, ws->d_seqs, st));
    *max_len = trim ? ctl[3] : ctl[1];                             // k_fq_trim leaves the longest trimmed read in ctl[3]
    return SALT_OK;
}

// The output stage of both text entry points, behind the align kernels queued on st: the block's n_rec records as SAM lines, BAM records or
// polished records (a length pass, room for the block, a write pass), then the block to page-locked host memory, deflated into BGZF blocks
// first when the workspace says so.  pe: the paired-end options, null for single end.  A new output mode is a branch of the two passes here.
static int text_emit(salt_gpu_ws_t *ws, const salt_text_opt_t *to, const salt_pe_opt_t *pe, uint32_t n_rec, uint32_t max_len, hipStream_t st, TextTrace &tr,
                     const char **sam, uint64_t *sam_bytes)
{
    salt_gpu_index *ix = ws->ix;
    const std::string rg = to->rg_id ? to->rg_id : "";
    if (to->rg_id && rg.empty()) return fail(SALT_E_INVAL, "empty read group id");
    if (rg != ws->rg || (!rg.empty() && !ws->d_rg)) {
        HIPCHK(hipStreamSynchronize(st));
        ws->d_rg.release();
        if (!rg.empty()) { HIPCHK(ws->d_rg.alloc(rg.size() + 1)); HIPCHK(hipMemcpy(ws->d_rg, rg.data(), rg.size(), hipMemcpyHostToDevice)); }
        ws->rg = rg;
    }
    SamDev d;
    d.raw = ws->d_raw; d.rec = ws->d_rec; d.seqs = ws->d_seqs; d.offs = ws->d_offs; d.res = ws->d_results;
    d.c_off = ix->d_c_off; d.c_name_off = ix->d_c_name_off; d.c_names = ix->d_c_names; d.n_contigs = ix->n_contigs;
    d.text = ix->view.text; d.ref = ix->view.ref; d.xa_cigar = to->print_xa_cigar; d.nm_md = to->print_nm_md;
    d.rg = ws->d_rg; d.rg_len = to->rg_id ? (int32_t)rg.size() : 0;
    d.pe = pe ? 1 : 0; d.min_tlen = pe ? pe->min_tlen : 0; d.max_tlen = pe ? pe->max_tlen : 0;
    d.slot = ws->d_samslot; d.seg = ws->d_samseg; d.tb = ws->d_tb; d.pg = PackGeom::make(max_len);
    // ---- lengths: the block's byte count, and with it every status word of the call, in one batch of copies ----
    uint32_t total = 0, n_over = 0, bam_err = 0; unsigned long long total64 = 0; int rc = SALT_OK;
    if (!ws->polish) {
        unsigned long long *d_total64 = reinterpret_cast<unsigned long long *>(ws->d_tctl + 4);
        if (ws->sam_bam) HIPCHK(launch_bam_len(d, n_rec, ws->d_samoff, d_total64, ws->d_tctl + 6, ws->d_scan, ws->d_scan.cap, st));
        else HIPCHK(launch_sam_len(d, n_rec, ws->d_samoff, d_total64, ws->d_scan, ws->d_scan.cap, st));
        HIPCHK(hipMemcpyAsync(&total, ws->d_samoff + n_rec, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&total64, d_total64, 8, hipMemcpyDeviceToHost, st));
        if (ws->sam_bam) HIPCHK(hipMemcpyAsync(&bam_err, ws->d_tctl + 6, 4, hipMemcpyDeviceToHost, st));
    }
    if (pe && ws->d_pctl) HIPCHK(hipMemcpyAsync(&n_over, &ws->d_pctl->overflow, 4, hipMemcpyDeviceToHost, st));      // (polish: read with the first count words of its own)
    if (!ws->polish) HIPCHK(hipStreamSynchronize(st));
    else {
        uint64_t pl_total = 0;
        rc = ws_polish_len(ws, n_rec, max_len, pe ? 1 : 0, st, &pl_total);
        if (rc && !n_over) return rc;
        total = (uint32_t)pl_total;
    }
    // a mate rescue that did not fit says more about the batch than what followed from it
    if (n_over) return fail(SALT_E_CAPACITY, std::to_string(n_over) + " mate rescue(s) need a Smith-Waterman band wider than this build holds (SW_BAND_W) "
                                             "or a CIGAR of more than SALT_MAX_CIGAR_OPS operations: the rows of this batch would differ from the reference's");
    if (bam_err) return fail(SALT_E_INVAL, "BAM: a read name in this block is longer than 254 bytes, the most a BAM record holds (its length byte counts the NUL)");
    if (total64 >> 32) return fail(SALT_E_CAPACITY, "the SAM text of this block passes 4 GiB (its offsets are 32-bit): hand over smaller blocks (SALT_CHUNK_MB)");
    tr.mark();
    if ((rc = reserve_sam(ws, (uint64_t)total + 64, (uint64_t)total + total / 4 + 64, nullptr, 0))) return rc;
    tr.mark();
    if (ws->polish && total == 0) { *sam = ws->h_sam; *sam_bytes = 0; return SALT_OK; }      // nothing but skipped reads: no record, no block
    // ---- write, and out ----
    if (ws->polish) { if ((rc = ws_polish_write(ws, st))) return rc; }
    else if (ws->sam_bam) HIPCHK(launch_bam_write(d, n_rec, ws->d_samoff, ws->d_sam, st));
    else HIPCHK(launch_sam_write(d, n_rec, ws->d_samoff, ws->d_sam, st));
    if (ws->sam_bgzf) { if ((rc = ws_sam_bgzf(ws, total, st, sam, sam_bytes))) return rc; }      // (sets them last)
    else {
        HIPCHK(hipMemcpyAsync(ws->h_sam, ws->d_sam, total, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        *sam = ws->h_sam; *sam_bytes = total;
    }
    tr.mark();
    return SALT_OK;
}

// The parse stage of a single-end text call: the block to the device (from the host, or n_src bytes of d_src with a newline behind them when
// n_bytes says so), its lines, records, offsets and codes.  *n_rec = 0: a block without a record, and nothing further was queued.
static int text_parse_se(salt_gpu_ws_t *ws, const char *fastq, const uint8_t *d_src, uint64_t n_src, uint64_t n_bytes, hipStream_t st, TextTrace &tr,
                         uint32_t *n_rec_out, uint32_t *max_len)
{
    *n_rec_out = 0;
    // ---- the raw block and its lines ----
    int rc = reserve_parse(ws, n_bytes, st);
    if (rc) return rc;
    const uint64_t n_tiles = (n_bytes + FQ_TILE - 1) / FQ_TILE;
    tr.mark();
    if (d_src) {
        static const char nl = '\n';
        HIPCHK(hipMemcpyAsync(ws->d_raw, d_src, n_src, hipMemcpyDeviceToDevice, st));
        if (n_bytes > n_src) HIPCHK(hipMemcpyAsync(ws->d_raw + n_src, &nl, 1, hipMemcpyHostToDevice, st));
    } else
        HIPCHK(hipMemcpyAsync(ws->d_raw, fastq, n_bytes, hipMemcpyHostToDevice, st));
    // newline count first: the line table is sized by it
    uint32_t n_nl = 0;
    HIPCHK(launch_fq_count(ws->d_raw, n_bytes, ws->d_tile, ws->d_scan, ws->d_scan.cap, st));
    HIPCHK(hipMemcpyAsync(&n_nl, ws->d_tile + n_tiles, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_nl % 4 != 0) return fail(SALT_E_INVAL, "FASTQ block does not hold whole 4-line records (" + std::to_string(n_nl) + " lines)");
    const uint32_t n_rec = n_nl / 4;
    if (n_rec > ws->max_reads) return fail(SALT_E_CAPACITY, "more reads in the block (" + std::to_string(n_rec) + ") than the workspace holds");
    if (n_rec == 0) return SALT_OK;
    tr.mark();
    if ((rc = ws->d_lines.reserve((uint64_t)n_nl + 8, st))) return rc;
    HIPCHK(launch_fq_lines(ws->d_raw, n_bytes, ws->d_tile, ws->d_lines, st));
    // ---- records, offsets, codes ----
    if ((rc = reserve_records(ws))) return rc;
    if (!ws->trim) HIPCHK(launch_fq_parse(ws->d_raw, ws->d_lines, n_rec, ws->d_rec, ws->d_offs, ws->d_tctl, ws->d_scan, ws->d_scan.cap, st));
    else {                                                       // the same, k_fq_trim between the records and the scan of their lengths
        HIPCHK(launch_fq_ctl_init(ws->d_tctl, st));
        HIPCHK(hipMemsetAsync(ws->d_offs + n_rec, 0, 4, st));
        HIPCHK(launch_fq_parse_recs(ws->d_raw, ws->d_lines, n_rec, ws->d_rec, ws->d_offs, ws->d_tctl, st));
        if ((rc = ws_trim_launch(ws, n_bytes, n_rec, 0, 0u, nullptr, st))) return rc;
        HIPCHK(launch_text_scan(ws->d_offs, n_rec + 1, ws->d_scan, ws->d_scan.cap, st));
    }
    if ((rc = text_codes(ws, n_rec, "block", st, max_len))) return rc;
    ws->q_cur.quals = ws->d_raw; ws->q_cur.rec = ws->d_rec; ws->q_cur.bytes = n_bytes;      // the error profile reads the qualities where they lie
    *n_rec_out = n_rec;
    return SALT_OK;
}

static int se_text_impl(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_text_opt_t *to, const char *fastq, const uint8_t *d_src, uint64_t n_bytes, int add_newline,
                        const char **sam, uint64_t *sam_bytes, uint32_t *n_reads)
{
    const uint64_t n_src = n_bytes;
    if (d_src && add_newline) ++n_bytes;
    ws->forget_last(); ws->trim_forget();
    salt_gpu_index *ix = ws->ix;
    if (!ix->d_c_off) return fail(SALT_E_INVAL, "SAM text needs the contig table: call salt_gpu_index_set_contigs first");
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t st = ws->stream;
    TextTrace tr; tr.on = ws->text_calls++ == 0 && getenv("SALT_TEXT_TRACE");
    tr.mark();
    uint32_t n_rec = 0, max_len = 0;
    int rc = text_parse_se(ws, fastq, d_src, n_src, n_bytes, st, tr, &n_rec, &max_len);
    if (rc) return rc;
    if (n_rec == 0) return SALT_OK;
    // ---- align ----
    tr.mark();
    if ((rc = align_resident_impl(ws, o, n_rec, max_len, ws->d_seqs, ws->d_offs, ws->d_results, st, 0))) return rc;
    tr.mark();
    // ---- SAM text ----
    if ((rc = text_emit(ws, to, nullptr, n_rec, max_len, st, tr, sam, sam_bytes))) return rc;
    if (tr.on && tr.n == 8) {
        const double *tm = tr.tm;
        fprintf(stderr, "[salt_gpu] first text call (ms): raw buffers %.1f, copy in + count %.1f, lines/parse/codes %.1f, align launch (+ its buffers) %.1f, "
                        "kernels + SAM lengths %.1f, SAM buffers %.1f, write + copy out %.1f\n", (tm[1] - tm[0]) * 1e3, (tm[2] - tm[1]) * 1e3, (tm[3] - tm[2]) * 1e3,
                (tm[4] - tm[3]) * 1e3, (tm[5] - tm[4]) * 1e3, (tm[6] - tm[5]) * 1e3, (tm[7] - tm[6]) * 1e3);
    }
    *n_reads = n_rec;
    return SALT_OK;
}

// The parse stage of a paired-end text call: both blocks to the device, their lines, the mates' records interleaved (record 2p + m = mate m
// of pair p), offsets and codes.  *n_pairs = 0: blocks without a record, and nothing further was queued.
static int text_parse_pe(salt_gpu_ws_t *ws, const char *fastq1, uint64_t n1, const char *fastq2, uint64_t n2, hipStream_t st, uint32_t *n_pairs, uint32_t *max_len)
{
    *n_pairs = 0;
    const uint64_t b2 = (n1 + 3) & ~3ull;                      // block 2 behind block 1, on a word boundary
    int rc = reserve_parse(ws, b2 + n2, st);
    if (rc) return rc;
    const uint64_t t1 = (n1 + FQ_TILE - 1) / FQ_TILE, t2 = (n2 + FQ_TILE - 1) / FQ_TILE;
    uint32_t *tile1 = ws->d_tile, *tile2 = ws->d_tile + t1 + 4;
    HIPCHK(hipMemcpyAsync(ws->d_raw, fastq1, n1, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws->d_raw + b2, fastq2, n2, hipMemcpyHostToDevice, st));
    uint32_t nl[2] = { 0, 0 };
    HIPCHK(launch_fq_count(ws->d_raw, n1, tile1, ws->d_scan, ws->d_scan.cap, st));
    HIPCHK(launch_fq_count(ws->d_raw + b2, n2, tile2, ws->d_scan, ws->d_scan.cap, st));
    HIPCHK(hipMemcpyAsync(&nl[0], tile1 + t1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nl[1], tile2 + t2, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nl[0] % 4 != 0 || nl[1] % 4 != 0) return fail(SALT_E_INVAL, "FASTQ block does not hold whole 4-line records (" + std::to_string(nl[0]) + " / " + std::to_string(nl[1]) + " lines)");
    if (nl[0] != nl[1]) return fail(SALT_E_INVAL, "the two FASTQ blocks hold different numbers of reads (" + std::to_string(nl[0] / 4) + " / " + std::to_string(nl[1] / 4) + ")");
    const uint32_t n = nl[0] / 4, n_rec = 2 * n;
    if (n_rec > ws->max_reads) return fail(SALT_E_CAPACITY, "more reads in the blocks (" + std::to_string(n_rec) + ") than the workspace holds");
    if (n == 0) return SALT_OK;
    if ((rc = ws->d_lines.reserve((uint64_t)nl[0] + nl[1] + 24, st))) return rc;
    uint32_t *lines1 = ws->d_lines, *lines2 = ws->d_lines + nl[0] + 8;
    HIPCHK(launch_fq_lines(ws->d_raw, n1, tile1, lines1, st));
    HIPCHK(launch_fq_lines(ws->d_raw + b2, n2, tile2, lines2, st));
    if ((rc = reserve_records(ws))) return rc;
    HIPCHK(launch_fq_ctl_init(ws->d_tctl, st));
    HIPCHK(hipMemsetAsync(ws->d_offs + n_rec, 0, 4, st));
    HIPCHK(launch_fq_parse_mate(ws->d_raw, 0u, lines1, n, 0u, ws->d_rec, ws->d_offs, ws->d_tctl, st));
    HIPCHK(launch_fq_parse_mate(ws->d_raw, (uint32_t)b2, lines2, n, 1u, ws->d_rec, ws->d_offs, ws->d_tctl, st));
    const bool pair = trim_pair_on(ws->trim_pair);
    if (pair) { if ((rc = ws_trim_pair_launch(ws, b2 + n2, n_rec, nullptr, st))) return rc; }
    else if (ws->trim && (rc = ws_trim_launch(ws, b2 + n2, n_rec, 1, 0u, nullptr, st))) return rc;
    HIPCHK(launch_text_scan(ws->d_offs, n_rec + 1, ws->d_scan, ws->d_scan.cap, st));
    if ((rc = text_codes(ws, n_rec, "blocks", st, max_len, pair))) return rc;
    ws->q_cur.quals = ws->d_raw; ws->q_cur.rec = ws->d_rec; ws->q_cur.bytes = b2 + n2;      // both blocks; a mate's qual_off counts from d_raw
    *n_pairs = n;
    return SALT_OK;
}

// Paired end: two blocks holding the same number of whole 4-line records (mates in file order); the SAM block holds both records of
// every pair, each followed by the reference's empty line (alnpe.c:640-648).
extern "C" int salt_gpu_align_pe_text(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_pe_opt_t *pe, const salt_text_opt_t *to,
                                      const char *fastq1, uint64_t n1, const char *fastq2, uint64_t n2,
                                      const char **sam, uint64_t *sam_bytes, uint32_t *n_pairs)
{
    if (!ws || !o || !pe || !to || !fastq1 || !fastq2 || !sam || !sam_bytes || !n_pairs) return fail(SALT_E_INVAL, "null argument");
    *sam = nullptr; *sam_bytes = 0; *n_pairs = 0; ws->forget_last(); ws->trim_forget();
    if (n1 == 0 && n2 == 0) return SALT_OK;
    if (n1 == 0 || n2 == 0) return fail(SALT_E_INVAL, "the two FASTQ blocks hold different numbers of reads");
    if (n1 + n2 >= 0xFFFFFFE0ull) return fail(SALT_E_CAPACITY, "FASTQ blocks of 4 GiB or more");
    if (fastq1[n1 - 1] != '\n' || fastq2[n2 - 1] != '\n') return fail(SALT_E_INVAL, "FASTQ block must end with a newline");
    salt_gpu_index *ix = ws->ix;
    if (!ix->d_c_off) return fail(SALT_E_INVAL, "SAM text needs the contig table: call salt_gpu_index_set_contigs first");
    if (!ix->d_pac) return fail(SALT_E_INVAL, "paired end needs the 2-bit genome: call salt_gpu_index_set_pac first");
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t st = ws->stream;
    uint32_t n = 0, max_len = 0;
    int rc = text_parse_pe(ws, fastq1, n1, fastq2, n2, st, &n, &max_len);
    if (rc) return rc;
    if (n == 0) return SALT_OK;
    const uint32_t n_rec = 2 * n;
    if ((rc = pe_resident_impl(ws, o, pe, n, max_len, ws->d_seqs, ws->d_offs, ws->d_results, st))) return rc;
    TextTrace tr;                                               // off: the stage clocks are single end's
    if ((rc = text_emit(ws, to, pe, n_rec, max_len, st, tr, sam, sam_bytes))) return rc;
    *n_pairs = n;
    return SALT_OK;
}

// The parser and k_fq_trim alone (include/salt_gpu.h): the lines and records of one block as text_parse_se makes them, every record trimmed
// as mate `mate`, the spans back.  Nothing behind the trim kernel runs: no scan, no codes.
extern "C" int salt_gpu_trim_spans(salt_gpu_ws_t *ws, const char *fastq, uint64_t n_bytes, int mate, uint32_t *beg_end)
{
    if (!ws || !fastq || !beg_end) return fail(SALT_E_INVAL, "null argument");
    if (mate != 0 && mate != 1) return fail(SALT_E_INVAL, "trim spans: mate is 0 or 1");
    ws->forget_last(); ws->trim_forget();
    if (n_bytes == 0) return SALT_OK;
    if (n_bytes >= 0xFFFFFFF0ull) return fail(SALT_E_CAPACITY, "FASTQ block of 4 GiB or more");
    if (fastq[n_bytes - 1] != '\n') return fail(SALT_E_INVAL, "FASTQ block must end with a newline");
    HIPCHK(hipSetDevice(ws->ix->device));
    hipStream_t st = ws->stream;
    int rc = reserve_parse(ws, n_bytes, st);
    if (rc) return rc;
    const uint64_t n_tiles = (n_bytes + FQ_TILE - 1) / FQ_TILE;
    HIPCHK(hipMemcpyAsync(ws->d_raw, fastq, n_bytes, hipMemcpyHostToDevice, st));
    uint32_t n_nl = 0;
    HIPCHK(launch_fq_count(ws->d_raw, n_bytes, ws->d_tile, ws->d_scan, ws->d_scan.cap, st));
    HIPCHK(hipMemcpyAsync(&n_nl, ws->d_tile + n_tiles, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_nl % 4 != 0) return fail(SALT_E_INVAL, "FASTQ block does not hold whole 4-line records (" + std::to_string(n_nl) + " lines)");
    const uint32_t n_rec = n_nl / 4;
    if (n_rec > ws->max_reads) return fail(SALT_E_CAPACITY, "more reads in the block (" + std::to_string(n_rec) + ") than the workspace holds");
    if (n_rec == 0) return SALT_OK;
    if ((rc = ws->d_lines.reserve((uint64_t)n_nl + 8, st))) return rc;
    HIPCHK(launch_fq_lines(ws->d_raw, n_bytes, ws->d_tile, ws->d_lines, st));
    if ((rc = reserve_records(ws))) return rc;
    if (!ws->d_trim_spans) HIPCHK(ws->d_trim_spans.alloc(2 * (uint64_t)ws->max_reads));
    HIPCHK(launch_fq_ctl_init(ws->d_tctl, st));
    HIPCHK(launch_fq_parse_recs(ws->d_raw, ws->d_lines, n_rec, ws->d_rec, ws->d_offs, ws->d_tctl, st));
    if ((rc = ws_trim_launch(ws, n_bytes, n_rec, 0, (uint32_t)mate, ws->d_trim_spans, st))) return rc;
    uint32_t ctl[4] = { 0, 0, 0, 0 }; uint64_t trimmed[2 * TRIM_N_COUNTS];
    HIPCHK(hipMemcpyAsync(ctl, ws->d_tctl, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(trimmed, ws->d_trim_cnt, sizeof trimmed, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(beg_end, ws->d_trim_spans, 2 * (uint64_t)n_rec * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ctl[0]) {
        const char *what = ctl[0] & 1 ? "a record does not start with '@'" : ctl[0] & 2 ? "the third line of a record does not start with '+'"
                         : ctl[0] & 4 ? "sequence and quality lengths differ" : "empty read";
        return fail(SALT_E_INVAL, std::string("input is not 4-line FASTQ at record ") + std::to_string(ctl[2]) + " of the block: " + what);
    }
    ws_trim_add(ws, trimmed);
    return SALT_OK;
}

// The pair form of salt_gpu_trim_spans: both blocks through the parser as text_parse_pe takes them, then k_fq_trim_pair alone (the pair rule
// on or off), b1, e1, b2, e2 of every pair back.  No scan, no codes.
extern "C" int salt_gpu_trim_pair_spans(salt_gpu_ws_t *ws, const char *fastq1, uint64_t n1, const char *fastq2, uint64_t n2, uint32_t *beg_end)
{
    if (!ws || !fastq1 || !fastq2 || !beg_end) return fail(SALT_E_INVAL, "null argument");
    ws->forget_last(); ws->trim_forget();
    if (n1 == 0 && n2 == 0) return SALT_OK;
    if (n1 == 0 || n2 == 0) return fail(SALT_E_INVAL, "the two FASTQ blocks hold different numbers of reads");
    if (n1 + n2 >= 0xFFFFFFE0ull) return fail(SALT_E_CAPACITY, "FASTQ blocks of 4 GiB or more");
    if (fastq1[n1 - 1] != '\n' || fastq2[n2 - 1] != '\n') return fail(SALT_E_INVAL, "FASTQ block must end with a newline");
    HIPCHK(hipSetDevice(ws->ix->device));
    hipStream_t st = ws->stream;
    const uint64_t b2 = (n1 + 3) & ~3ull;
    int rc = reserve_parse(ws, b2 + n2, st);
    if (rc) return rc;
    const uint64_t t1 = (n1 + FQ_TILE - 1) / FQ_TILE, t2 = (n2 + FQ_TILE - 1) / FQ_TILE;
    uint32_t *tile1 = ws->d_tile, *tile2 = ws->d_tile + t1 + 4;
    HIPCHK(hipMemcpyAsync(ws->d_raw, fastq1, n1, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws->d_raw + b2, fastq2, n2, hipMemcpyHostToDevice, st));
    uint32_t nl[2] = { 0, 0 };
    HIPCHK(launch_fq_count(ws->d_raw, n1, tile1, ws->d_scan, ws->d_scan.cap, st));
    HIPCHK(launch_fq_count(ws->d_raw + b2, n2, tile2, ws->d_scan, ws->d_scan.cap, st));
    HIPCHK(hipMemcpyAsync(&nl[0], tile1 + t1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nl[1], tile2 + t2, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nl[0] % 4 != 0 || nl[1] % 4 != 0) return fail(SALT_E_INVAL, "FASTQ block does not hold whole 4-line records (" + std::to_string(nl[0]) + " / " + std::to_string(nl[1]) + " lines)");
    if (nl[0] != nl[1]) return fail(SALT_E_INVAL, "the two FASTQ blocks hold different numbers of reads (" + std::to_string(nl[0] / 4) + " / " + std::to_string(nl[1] / 4) + ")");
    const uint32_t n = nl[0] / 4, n_rec = 2 * n;
    if (n_rec > ws->max_reads) return fail(SALT_E_CAPACITY, "more reads in the blocks (" + std::to_string(n_rec) + ") than the workspace holds");
    if (n == 0) return SALT_OK;
    if ((rc = ws->d_lines.reserve((uint64_t)nl[0] + nl[1] + 24, st))) return rc;
    uint32_t *lines1 = ws->d_lines, *lines2 = ws->d_lines + nl[0] + 8;
    HIPCHK(launch_fq_lines(ws->d_raw, n1, tile1, lines1, st));
    HIPCHK(launch_fq_lines(ws->d_raw + b2, n2, tile2, lines2, st));
    if ((rc = reserve_records(ws))) return rc;
    if (!ws->d_trim_spans) HIPCHK(ws->d_trim_spans.alloc(2 * (uint64_t)ws->max_reads));
    HIPCHK(launch_fq_ctl_init(ws->d_tctl, st));
    HIPCHK(launch_fq_parse_mate(ws->d_raw, 0u, lines1, n, 0u, ws->d_rec, ws->d_offs, ws->d_tctl, st));
    HIPCHK(launch_fq_parse_mate(ws->d_raw, (uint32_t)b2, lines2, n, 1u, ws->d_rec, ws->d_offs, ws->d_tctl, st));
    if ((rc = ws_trim_pair_launch(ws, b2 + n2, n_rec, ws->d_trim_spans, st))) return rc;
    uint32_t ctl[4] = { 0, 0, 0, 0 }; uint64_t trimmed[TRIM_CNT_WORDS];
    HIPCHK(hipMemcpyAsync(ctl, ws->d_tctl, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(trimmed, ws->d_trim_cnt, sizeof trimmed, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(beg_end, ws->d_trim_spans, 2 * (uint64_t)n_rec * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ctl[0]) {
        const char *what = ctl[0] & 1 ? "a record does not start with '@'" : ctl[0] & 2 ? "the third line of a record does not start with '+'"
                         : ctl[0] & 4 ? "sequence and quality lengths differ" : "empty read";
        return fail(SALT_E_INVAL, std::string("input is not 4-line FASTQ at record ") + std::to_string(ctl[2]) + " of the blocks: " + what);
    }
    ws_trim_add(ws, trimmed, true);
    return SALT_OK;
}

// One row of salt_gpu_diag_text_rows against what the record kernels index with it: empty = the row is in range.  L: the read's length.
// pe: the paired-end kernels never read `skipped` (mapped is pos alone there), so only a single-end row is excused by it.
static std::string text_row_fault(const salt_result_t &q, uint32_t L, uint32_t ref_len, bool pe)
{
    const uint32_t n_hits = (uint32_t)q.n_hits[0] + q.n_hits[1];
    if (n_hits > SALT_MAX_HITS) return "n_hits[0] + n_hits[1] = " + std::to_string(n_hits) + " is more than SALT_MAX_HITS";
    for (uint32_t s = 0, h = 0; s < 2; ++s)
        for (uint32_t k = 0; k < q.n_hits[s]; ++k, ++h) {
            if (q.hit_n_cigar[h] > SALT_MAX_CIGAR_OPS) return "hit_n_cigar[" + std::to_string(h) + "] is more than SALT_MAX_CIGAR_OPS";
            if (q.hits[s][k].pos >= ref_len) return "the pos of hit " + std::to_string(h) + " lies beyond the genome";
        }
    if ((!pe && q.skipped) || q.pos == 0xFFFFFFFFu) return "";
    if (q.n_cigar > SALT_MAX_CIGAR_OPS) return "n_cigar is more than SALT_MAX_CIGAR_OPS";
    if (q.pos >= ref_len) return "pos lies beyond the genome";
    uint64_t on_ref = 0, on_read = 0;
    for (uint32_t c = 0; c < q.n_cigar; ++c) {
        const uint32_t n = q.cigar[c] >> 4, op = q.cigar[c] & 15u;
        if (op == 0) { on_ref += n; on_read += n; } else if (op == 1) on_read += n; else if (op == 2) on_ref += n;
    }
    if ((uint64_t)q.pos + on_ref > ref_len) return "pos + the CIGAR's M and D operations end beyond the genome";
    if ((uint64_t)q.seq_start + on_read > L) return "seq_start + the CIGAR's M and I operations end beyond the read";
    if (q.seq_end >= L) return "seq_end lies beyond the read";
    return "";
}

// The text stage on rows of the caller's (include/salt_gpu.h): the parse stage and text_emit of the production entry points, and between them
// k_pack and a copy where those align.  Every row is checked on the host against the lengths the parse kernels found: no kernel sees a row
// that would take it outside the genome, the read or the row itself.
extern "C" int salt_gpu_diag_text_rows(salt_gpu_ws_t *ws, const salt_text_opt_t *to, const salt_pe_opt_t *pe, const char *fastq1, uint64_t n1,
                                       const char *fastq2, uint64_t n2, const salt_result_t *rows, uint32_t n_rows,
                                       const char **out, uint64_t *out_bytes, uint32_t *n_records)
{
    if (!ws || !to || !fastq1 || (pe && !fastq2) || (n_rows && !rows) || !out || !out_bytes || !n_records) return fail(SALT_E_INVAL, "null argument");
    *out = nullptr; *out_bytes = 0; *n_records = 0; ws->forget_last(); ws->trim_forget();
    if (ws->polish) return fail(SALT_E_INVAL, "text rows: the polish stage is not driven from rows (salt_gpu_ws_set_polish is on)");
    if (ws->trim) return fail(SALT_E_INVAL, "text rows: the rows are checked against the untrimmed reads (salt_gpu_ws_set_trim is on)");
    if (trim_pair_on(ws->trim_pair)) return fail(SALT_E_INVAL, "text rows: the rows are checked against the untrimmed reads (salt_gpu_ws_set_trim_pair is on)");
    if (n1 == 0 || (pe && n2 == 0)) return fail(SALT_E_INVAL, "text rows: an empty FASTQ block");
    if (n1 + (pe ? n2 : 0) >= 0xFFFFFFE0ull) return fail(SALT_E_CAPACITY, "FASTQ blocks of 4 GiB or more");
    if (fastq1[n1 - 1] != '\n' || (pe && fastq2[n2 - 1] != '\n')) return fail(SALT_E_INVAL, "FASTQ block must end with a newline");
    salt_gpu_index *ix = ws->ix;
    if (!ix->d_c_off) return fail(SALT_E_INVAL, "SAM text needs the contig table: call salt_gpu_index_set_contigs first");
    HIPCHK(hipSetDevice(ix->device));
    hipStream_t st = ws->stream;
    TextTrace tr;                                               // off
    uint32_t n_rec = 0, max_len = 0;
    int rc;
    if (pe) { uint32_t n = 0; rc = text_parse_pe(ws, fastq1, n1, fastq2, n2, st, &n, &max_len); n_rec = 2 * n; }
    else rc = text_parse_se(ws, fastq1, nullptr, n1, n1, st, tr, &n_rec, &max_len);
    if (rc) return rc;
    if (n_rows != n_rec) return fail(SALT_E_INVAL, "text rows: " + std::to_string(n_rows) + " rows for " + std::to_string(n_rec) + " parsed records");
    if (n_rec == 0) return SALT_OK;
    if (max_len > SALT_MAX_READ_LEN) return fail(SALT_E_INVAL, "read longer than SALT_MAX_READ_LEN (512)");
    // ---- the rows, checked against the parsed lengths before anything reads them ----
    std::vector<uint32_t> offs((size_t)n_rec + 1);
    HIPCHK(hipMemcpyAsync(offs.data(), ws->d_offs, ((uint64_t)n_rec + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n_rec; ++i) {
        const std::string what = text_row_fault(rows[i], offs[i + 1] - offs[i], ix->view.ref_len, pe != nullptr);
        if (!what.empty()) return fail(SALT_E_INVAL, "text rows: row " + std::to_string(i) + ": " + what);
    }
    // ---- where the align kernels stand: k_pack's records (the MD / NM / XV words of k_sam_len), then the rows ----
    const PackGeom pg = PackGeom::make(max_len);
    if ((rc = reserve_pack(ws, n_rec, pg, st))) return rc;
    launch_pack(pg, n_rec, ws->d_seqs, ws->d_offs, ws->d_pm, ws->d_tb, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ws->d_results, rows, (uint64_t)n_rec * sizeof(salt_result_t), hipMemcpyHostToDevice, st));
    if (pe && ws->d_pctl) HIPCHK(hipMemsetAsync(ws->d_pctl, 0, sizeof(PeCtl), st));      // no rescue ran: text_emit reads its overflow count
    HIPCHK(hipStreamSynchronize(st));                           // the rows are the caller's memory
    if ((rc = text_emit(ws, to, pe, n_rec, max_len, st, tr, out, out_bytes))) return rc;
    *n_records = n_rec;
    return SALT_OK;
}

// ---------------------------------------------------------------------------------------------
// polish (row N4)
// ---------------------------------------------------------------------------------------------
struct salt_gpu_polish { int device = 0; uint8_t *d_pac = nullptr; uint64_t l_pac = 0; void *d_tabs = nullptr; uint32_t n_blocks = 0; PolishText *text = nullptr; };

extern "C" int salt_gpu_polish_open(int device, const uint8_t *pac, uint64_t l_pac, salt_gpu_polish_t **out)
{
    if (!pac || !out || l_pac == 0) return fail(SALT_E_INVAL, "null argument");
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (n_dev <= 0) return fail(SALT_E_HIP, "no HIP device visible: polish cannot run (there is no CPU fallback)");
    HIPCHK(hipSetDevice(device));
    salt_gpu_polish *p = new salt_gpu_polish();
    p->device = device; p->l_pac = l_pac;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_pac, l_pac / 4 + 8);
    if (e == hipSuccess) e = hipMemcpy(p->d_pac, pac, l_pac / 4 + 1, hipMemcpyHostToDevice);
    p->n_blocks = (uint32_t)prop.multiProcessorCount * 8u;
    if (e == hipSuccess) e = hipMalloc(&p->d_tabs, (uint64_t)p->n_blocks * lv_table_bytes());
    if (e != hipSuccess) { hipFree(p->d_pac); hipFree(p->d_tabs); delete p; return fail(SALT_E_HIP, std::string("polish open: ") + hipGetErrorString(e)); }
    *out = p;
    return SALT_OK;
}
extern "C" void salt_gpu_polish_close(salt_gpu_polish_t *p) { if (!p) return; hipSetDevice(p->device); polish_text_free(p->text); hipFree(p->d_pac); hipFree(p->d_tabs); delete p; }

// SAM record lines in, polished record lines out: the whole of `polish` for one block on the device (salt_polish.hip)
extern "C" int salt_gpu_polish_set_contigs(salt_gpu_polish_t *p, int32_t n, const int64_t *offsets, const char *const *names)
{
    if (!p || n < 0 || (n && (!offsets || !names))) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(p->device));
    if (!p->text) p->text = polish_text_new();
    std::string err;
    const int rc = polish_text_set_contigs(p->text, n, offsets, names, err);
    return rc ? fail(rc, err) : SALT_OK;
}
extern "C" int salt_gpu_polish_text(salt_gpu_polish_t *p, const salt_polish_opt_t *opt, const char *sam, uint64_t n_bytes,
                                    const char **out, uint64_t *out_bytes, uint32_t *n_records, int *stopped)
{
    if (!p || !opt || (!sam && n_bytes) || !out || !out_bytes || !n_records || !stopped) return fail(SALT_E_INVAL, "null argument");
    if (n_bytes >> 31) return fail(SALT_E_INVAL, "polish text: a block holds less than 2^31 bytes");
    if (!p->text) return fail(SALT_E_INVAL, "polish text: no contig table (salt_gpu_polish_set_contigs)");
    HIPCHK(hipSetDevice(p->device));
    std::string err;
    const int rc = polish_text_run(p->text, p->d_pac, p->l_pac, p->d_tabs, p->n_blocks, opt->paired != 0, opt->use_sw != 0, sam, n_bytes, out, out_bytes, n_records, stopped, err);
    if (rc) { *out_bytes = 0; *n_records = 0; return fail(rc, err); }
    return SALT_OK;
}
extern "C" int salt_gpu_polish_text_stats(salt_gpu_polish_t *p, uint64_t out[8])
{
    if (!p || !out) return fail(SALT_E_INVAL, "null argument");
    for (int i = 0; i < 8; ++i) out[i] = p->text ? polish_text_stats(p->text)[i] : 0;
    return SALT_OK;
}

extern "C" int salt_gpu_polish_lv(salt_gpu_polish_t *p, const uint8_t *codes, const uint32_t *offs, uint32_t n_reads, const salt_polish_item_t *items,
                                  uint32_t n_items, const uint8_t *pool, uint32_t pool_stride, uint32_t n_pool, int want_cigar,
                                  int32_t *dist, uint16_t *cigars, uint8_t *n_cigar)
{
    if (!p || !codes || !offs || !items || !dist || (want_cigar && (!cigars || !n_cigar)) || (n_pool && !pool)) return fail(SALT_E_INVAL, "null argument");
    if (n_items == 0) return SALT_OK;
    for (uint32_t i = 0; i < n_items; ++i) {                   // shapes the kernel assumes, checked before anything is launched
        const salt_polish_item_t &x = items[i];
        if (x.read >= n_reads) return fail(SALT_E_INVAL, "polish item names a read outside the batch");
        const uint32_t L = offs[x.read + 1] - offs[x.read];
        if (L == 0 || L > SALT_MAX_READ_LEN || x.tlen > L || x.k >= 31) return fail(SALT_E_INVAL, "polish item: read length / window / bound outside the kernel's range");
        if (x.pool == 0xFFFFFFFFu) { if ((uint64_t)x.offset + x.tlen > p->l_pac) return fail(SALT_E_INVAL, "polish item: window beyond the genome"); }
        else if (x.pool >= n_pool || pool_stride < L) return fail(SALT_E_INVAL, "polish item: explicit window outside the pool");
    }
    HIPCHK(hipSetDevice(p->device));
    uint8_t *d_codes = nullptr, *d_pool = nullptr, *d_nc = nullptr; uint32_t *d_offs = nullptr; salt_polish_item_t *d_items = nullptr; int32_t *d_dist = nullptr; uint16_t *d_cig = nullptr;
    const uint64_t bases = offs[n_reads];
    auto done = [&](int rc) { hipFree(d_codes); hipFree(d_pool); hipFree(d_nc); hipFree(d_offs); hipFree(d_items); hipFree(d_dist); hipFree(d_cig); return rc; };
    DONECHK(hipMalloc((void **)&d_codes, bases + 64)); DONECHK(hipMemcpy(d_codes, codes, bases, hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_offs, ((uint64_t)n_reads + 1) * 4)); DONECHK(hipMemcpy(d_offs, offs, ((uint64_t)n_reads + 1) * 4, hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_items, (uint64_t)n_items * sizeof(salt_polish_item_t))); DONECHK(hipMemcpy(d_items, items, (uint64_t)n_items * sizeof(salt_polish_item_t), hipMemcpyHostToDevice));
    if (n_pool) { DONECHK(hipMalloc((void **)&d_pool, (uint64_t)n_pool * pool_stride + 8)); DONECHK(hipMemcpy(d_pool, pool, (uint64_t)n_pool * pool_stride, hipMemcpyHostToDevice)); }
    DONECHK(hipMalloc((void **)&d_dist, (uint64_t)n_items * 4));
    if (want_cigar) { DONECHK(hipMalloc((void **)&d_cig, (uint64_t)n_items * SALT_MAX_CIGAR_OPS * 2)); DONECHK(hipMalloc((void **)&d_nc, n_items)); DONECHK(hipMemset(d_nc, 0, n_items)); }
    const uint32_t blocks = n_items < p->n_blocks ? n_items : p->n_blocks;
    launch_polish(p->d_pac, d_codes, d_offs, d_items, n_items, d_pool, pool_stride, want_cigar, d_dist, d_cig, d_nc, p->d_tabs, blocks, nullptr);
    DONECHK(hipGetLastError());
    DONECHK(hipDeviceSynchronize());
    DONECHK(hipMemcpy(dist, d_dist, (uint64_t)n_items * 4, hipMemcpyDeviceToHost));
    if (want_cigar) { DONECHK(hipMemcpy(cigars, d_cig, (uint64_t)n_items * SALT_MAX_CIGAR_OPS * 2, hipMemcpyDeviceToHost)); DONECHK(hipMemcpy(n_cigar, d_nc, n_items, hipMemcpyDeviceToHost)); }
    return done(SALT_OK);
}

// One Smith-Waterman launch outside a workspace (polish -s, the unit entry): h_req in, their rows into h_res, *overflow = the rescues
// this build cannot finish as the reference would (PeCtl::overflow).  Frees what it allocates on every path.
static int sw_run(const IndexView &v, const uint8_t *d_pac, const uint8_t *d_codes, const uint32_t *d_offs, const std::vector<PeSwReq> &h_req,
                  SwGeom geom, uint32_t max_len, std::vector<PeSwRes> &h_res, uint32_t *overflow)
{
    const uint64_t n = h_req.size();
    PeSwReq *d_req = nullptr; PeSwRes *d_res = nullptr; uint8_t *d_scr = nullptr; PeCtl *d_ctl = nullptr;
    auto done = [&](int rc) { hipFree(d_req); hipFree(d_res); hipFree(d_scr); hipFree(d_ctl); return rc; };
    DONECHK(hipMalloc((void **)&d_req, n * sizeof(PeSwReq))); DONECHK(hipMemcpy(d_req, h_req.data(), n * sizeof(PeSwReq), hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_res, n * sizeof(PeSwRes)));
    DONECHK(hipMalloc((void **)&d_scr, sw_scratch_bytes(geom)));
    PeCtl ctl{}; ctl.n_req = (uint32_t)n;
    DONECHK(hipMalloc((void **)&d_ctl, sizeof ctl)); DONECHK(hipMemcpy(d_ctl, &ctl, sizeof ctl, hipMemcpyHostToDevice));
    launch_sw(v, d_pac, d_codes, d_offs, d_req, d_ctl, d_res, d_scr, geom, max_len, nullptr);
    DONECHK(hipGetLastError());
    DONECHK(hipDeviceSynchronize());
    DONECHK(hipMemcpy(&ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
    h_res.resize(n);
    DONECHK(hipMemcpy(h_res.data(), d_res, n * sizeof(PeSwRes), hipMemcpyDeviceToHost));
    *overflow = ctl.overflow;
    return done(SALT_OK);
}

extern "C" int salt_gpu_polish_sw(salt_gpu_polish_t *p, const uint8_t *codes, const uint32_t *offs, uint32_t n_reads, const salt_polish_item_t *items,
                                  uint32_t n_items, int want_cigar, int32_t *score, int32_t *read_span, uint16_t *cigars, uint16_t *n_cigar)
{
    if (!p || !codes || !offs || !items || !score || (want_cigar && (!read_span || !cigars || !n_cigar))) return fail(SALT_E_INVAL, "null argument");
    if (n_items == 0) return SALT_OK;
    uint32_t max_len = 1;
    std::vector<PeSwReq> h_req(n_items);
    for (uint32_t i = 0; i < n_items; ++i) {                   // shapes the kernel assumes, checked before anything is launched
        const salt_polish_item_t &x = items[i];
        if (x.read >= n_reads) return fail(SALT_E_INVAL, "polish item names a read outside the batch");
        const uint32_t L = offs[x.read + 1] - offs[x.read];
        if (L == 0 || L > SALT_MAX_READ_LEN || x.tlen == 0 || x.tlen > L) return fail(SALT_E_INVAL, "polish item: read length / window outside the kernel's range");
        if ((uint64_t)x.offset + x.tlen > p->l_pac) return fail(SALT_E_INVAL, "polish item: window beyond the genome");
        if (L > max_len) max_len = L;
        h_req[i] = PeSwReq{ x.offset, x.offset + x.tlen - 1u, x.read, (uint8_t)(x.strand ? 1 : 0), 2, (uint16_t)(want_cigar ? 0 : 1) };
    }
    HIPCHK(hipSetDevice(p->device));
    uint8_t *d_codes = nullptr; uint32_t *d_offs = nullptr;
    const uint64_t bases = offs[n_reads];
    auto done = [&](int rc) { hipFree(d_codes); hipFree(d_offs); return rc; };
    DONECHK(hipMalloc((void **)&d_codes, bases + 64)); DONECHK(hipMemcpy(d_codes, codes, bases, hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_offs, ((uint64_t)n_reads + 1) * 4)); DONECHK(hipMemcpy(d_offs, offs, ((uint64_t)n_reads + 1) * 4, hipMemcpyHostToDevice));
    SwGeom geom = sw_geom(max_len, max_len, p->n_blocks / 8u);
    sw_geom_limit(geom, (n_items + 7u) / 8u);
    IndexView v; memset(&v, 0, sizeof v);
    v.ref_len = (uint32_t)p->l_pac;                            // k_sw's range check; mode 2 reads the 2-bit genome only
    std::vector<PeSwRes> h_res; uint32_t n_over = 0;
    if (int rc = sw_run(v, p->d_pac, d_codes, d_offs, h_req, geom, max_len, h_res, &n_over)) return done(rc);
    if (n_over) return done(fail(SALT_E_INVAL, "polish -s: an alignment needs a wider band or more CIGAR operations than this build holds"));
    for (uint32_t i = 0; i < n_items; ++i) {
        const PeSwRes &r = h_res[i];
        score[i] = r.score1;
        if (want_cigar) {
            read_span[2 * (uint64_t)i] = r.read_begin; read_span[2 * (uint64_t)i + 1] = r.read_end;
            n_cigar[i] = r.n_cigar;
            memcpy(cigars + (uint64_t)i * SALT_MAX_CIGAR_OPS, r.cigar, sizeof r.cigar);
        }
    }
    return done(SALT_OK);
}

extern "C" int salt_gpu_index_replicate(salt_gpu_index_t *src, const int *devices, int n, salt_gpu_index_t **out)
{
    if (!src || !devices || !out || n < 1 || devices[0] != src->device) return fail(SALT_E_INVAL, "bad replicate arguments");
    out[0] = src;
    for (int i = 1; i < n; ++i) out[i] = nullptr;
    if (n == 1) return SALT_OK;
    std::vector<void *> buf((size_t)n, nullptr);
    std::vector<ncclComm_t> comm((size_t)n, nullptr);
    std::vector<hipStream_t> st((size_t)n, nullptr);
    bool comm_ok = false;
    // every exit passes here: what a failed step leaves behind (buffers not yet owned by an index, communicators, streams) is released
    auto cleanup = [&](bool failed) {
        for (int i = 0; i < n; ++i) {
            hipSetDevice(devices[i]);
            if (st[i]) hipStreamDestroy(st[i]);
            if (comm_ok && comm[i]) ncclCommDestroy(comm[i]);
            if (failed && i > 0) {
                if (out[i]) { salt_gpu_index_detach(out[i]); out[i] = nullptr; }       // owns buf[i]
                else if (buf[i]) hipFree(buf[i]);
            }
        }
        hipSetDevice(devices[0]);
    };
#define REPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(true); \
    return fail(SALT_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } } while (0)
    buf[0] = src->image;
    for (int i = 1; i < n; ++i) { REPCHK(hipSetDevice(devices[i])); REPCHK(hipMalloc(&buf[i], src->bytes)); }
    ncclResult_t rc = ncclCommInitAll(comm.data(), n, devices);
    if (rc != ncclSuccess) { cleanup(true); return fail(SALT_E_HIP, std::string("ncclCommInitAll: ") + ncclGetErrorString(rc)); }
    comm_ok = true;
    for (int i = 0; i < n; ++i) { REPCHK(hipSetDevice(devices[i])); REPCHK(hipStreamCreate(&st[i])); }
    ncclGroupStart();
    for (int i = 0; i < n; ++i) {
        rc = ncclBroadcast(buf[i], buf[i], src->hdr.off_wlkt, ncclUint8, 0, comm[i], st[i]);      // the compact part only
        if (rc != ncclSuccess) { ncclGroupEnd(); cleanup(true); return fail(SALT_E_HIP, std::string("ncclBroadcast: ") + ncclGetErrorString(rc)); }
    }
    rc = ncclGroupEnd();
    if (rc != ncclSuccess) { cleanup(true); return fail(SALT_E_HIP, std::string("ncclGroupEnd: ") + ncclGetErrorString(rc)); }
    for (int i = 0; i < n; ++i) { REPCHK(hipSetDevice(devices[i])); REPCHK(hipStreamSynchronize(st[i])); }
    for (int i = 1; i < n; ++i) {
        int r2 = salt_gpu_index_attach_image(buf[i], src->bytes, devices[i], &out[i]);
        if (r2) { out[i] = nullptr; const std::string m = g_err; cleanup(true); return fail(r2, m); }
        out[i]->owns = true;                                        // from here on detach releases buf[i]
        REPCHK(hipSetDevice(devices[i]));
        r2 = rebuild_wlkt(out[i]);                                  // each device tabulates its own W-mer table
        if (r2) { const std::string m = g_err; cleanup(true); return fail(r2, m); }
    }
#undef REPCHK
    cleanup(false);
    return SALT_OK;
}

extern "C" int salt_gpu_index_image_copy(const salt_gpu_index_t *ix, void *dst, uint64_t dst_bytes)
{
    if (!ix || !dst) return fail(SALT_E_INVAL, "null argument");
    const uint64_t n = dst_bytes >= ix->bytes ? ix->bytes : ix->hdr.off_wlkt;       // the full image, or its compact part
    if (dst_bytes < n) return fail(SALT_E_INVAL, "destination too small for the (compact) index image");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemcpy(dst, ix->image, n, hipMemcpyDeviceToDevice));
    return SALT_OK;
}

extern "C" int salt_gpu_ws_timing(salt_gpu_ws_t *ws, int enable)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(ws->ix->device));
    if (enable && ws->ev.empty()) {
        ws->ev.resize((size_t)MAX_TIMED * EV_PER_CALL);
        ws->ev_pe.assign(MAX_TIMED, 0);
        for (auto &e : ws->ev) HIPCHK(hipEventCreate(&e));
    }
    ws->timing = enable != 0; ws->n_timed = 0;
    return SALT_OK;
}

extern "C" int salt_gpu_ws_kernel_ms(salt_gpu_ws_t *ws, double ms[SALT_N_KERNELS], uint32_t *n_calls)
{
    if (!ws || !ms || !n_calls) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(ws->ix->device));
    for (int k = 0; k < SALT_N_KERNELS; ++k) ms[k] = 0;
    *n_calls = ws->n_timed;
    for (uint32_t i = 0; i < ws->n_timed; ++i) {
        hipEvent_t *ev = &ws->ev[(size_t)i * EV_PER_CALL];
        const int n_k = ws->ev_pe[i] ? SALT_N_KERNELS : 7;
        HIPCHK(hipEventSynchronize(ev[n_k]));
        for (int k = 0; k < n_k; ++k) {
            float a = 0;
            HIPCHK(hipEventElapsedTime(&a, ev[k], ev[k + 1]));
            ms[k] += a;
        }
    }
    ws->n_timed = 0;
    return SALT_OK;
}

// Unit access for tests: verify / LV device functions on a caller-supplied mixRef (no index needed).
extern "C" int salt_gpu_diag_lv(const uint32_t *ref_words, uint32_t ref_len, uint32_t n_cases, const uint32_t *pos,
                                const uint32_t *kdiff, const uint8_t *seqs, const uint32_t *offs, int32_t *out4,
                                uint16_t *cigars)
{
    return salt_gpu_diag_lv_tab(ref_words, ref_len, n_cases, pos, kdiff, seqs, offs, out4, cigars, 0);
}
extern "C" int salt_gpu_diag_lv_tab(const uint32_t *ref_words, uint32_t ref_len, uint32_t n_cases, const uint32_t *pos,
                                    const uint32_t *kdiff, const uint8_t *seqs, const uint32_t *offs, int32_t *out4,
                                    uint16_t *cigars, int lds_tab)
{
    if (!ref_words || !pos || !kdiff || !seqs || !offs || !out4 || !cigars) return fail(SALT_E_INVAL, "null argument");
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (n_dev <= 0) return fail(SALT_E_HIP, "no HIP device visible");
    const uint64_t nw = ((uint64_t)ref_len + 7) / 8 + 4;
    uint32_t *d_ref = nullptr, *d_pos = nullptr, *d_k = nullptr, *d_offs = nullptr; uint8_t *d_seqs = nullptr;
    int32_t *d_out = nullptr; uint16_t *d_cig = nullptr;
    const uint64_t bases = offs[n_cases];
    HIPCHK(hipMalloc((void **)&d_ref, nw * 4)); HIPCHK(hipMemset(d_ref, 0, nw * 4));
    HIPCHK(hipMemcpy(d_ref, ref_words, (nw - 4) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_pos, (uint64_t)n_cases * 4)); HIPCHK(hipMemcpy(d_pos, pos, (uint64_t)n_cases * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_k, (uint64_t)n_cases * 4)); HIPCHK(hipMemcpy(d_k, kdiff, (uint64_t)n_cases * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_offs, ((uint64_t)n_cases + 1) * 4)); HIPCHK(hipMemcpy(d_offs, offs, ((uint64_t)n_cases + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_seqs, bases + 64)); HIPCHK(hipMemcpy(d_seqs, seqs, bases, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_out, (uint64_t)n_cases * 16)); HIPCHK(hipMemset(d_out, 0xFD, (uint64_t)n_cases * 16));
    HIPCHK(hipMalloc((void **)&d_cig, (uint64_t)n_cases * SALT_MAX_CIGAR_OPS * 2)); HIPCHK(hipMemset(d_cig, 0, (uint64_t)n_cases * SALT_MAX_CIGAR_OPS * 2));
    IndexView v; memset(&v, 0, sizeof v);
    v.ref = d_ref; v.ref_len = ref_len;
    void *d_tab = nullptr;
    HIPCHK(hipMalloc(&d_tab, (uint64_t)n_cases * lv_table_bytes()));
    // the lane kernel's share: where 64 cases have one (L, k) the first one's block runs all of them, a lane each; the others go alone
    std::vector<uint32_t> lane_first(n_cases + 1, 0u), lane_n(n_cases + 1, 0u), lane_case;
    {
        std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> by_shape;
        for (uint32_t c = 0; c < n_cases; ++c) {
            if (offs[c + 1] < offs[c]) return fail(SALT_E_INVAL, "offsets must not decrease");
            if (lv_lanes_fit(offs[c + 1] - offs[c], kdiff[c])) by_shape[std::make_pair(offs[c + 1] - offs[c], kdiff[c])].push_back(c);
        }
        for (const auto &kv : by_shape) {
            const std::vector<uint32_t> &cs = kv.second;
            for (size_t i = 0; i < cs.size();) {
                const uint32_t take = cs.size() - i >= 64 ? 64u : 1u;
                lane_first[cs[i]] = (uint32_t)lane_case.size(); lane_n[cs[i]] = take;
                lane_case.insert(lane_case.end(), cs.begin() + i, cs.begin() + i + take);
                i += take;
            }
        }
        lane_case.push_back(0u);
    }
    uint32_t *d_lf = nullptr, *d_ln = nullptr, *d_lc = nullptr;
    HIPCHK(hipMalloc((void **)&d_lf, lane_first.size() * 4)); HIPCHK(hipMemcpy(d_lf, lane_first.data(), lane_first.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_ln, lane_n.size() * 4)); HIPCHK(hipMemcpy(d_ln, lane_n.data(), lane_n.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_lc, lane_case.size() * 4)); HIPCHK(hipMemcpy(d_lc, lane_case.data(), lane_case.size() * 4, hipMemcpyHostToDevice));
    launch_diag_lv(v, n_cases, d_pos, d_k, d_seqs, d_offs, d_lf, d_ln, d_lc, d_out, d_cig, d_tab, lds_tab, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out4, d_out, (uint64_t)n_cases * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cigars, d_cig, (uint64_t)n_cases * SALT_MAX_CIGAR_OPS * 2, hipMemcpyDeviceToHost));
    hipFree(d_ref); hipFree(d_pos); hipFree(d_k); hipFree(d_offs); hipFree(d_seqs); hipFree(d_out); hipFree(d_cig); hipFree(d_tab);
    hipFree(d_lf); hipFree(d_ln); hipFree(d_lc);
    return SALT_OK;
}

// Unit entry of the Smith-Waterman rescue kernel: case i aligns read codes[read_offs[i]..) against the reference symbols
// ref_syms[ref_offs[i]..) (4-bit allele masks when aware[i], bases 0..3 otherwise), the way snpaln_sw_snpaware / snpaln_sw
// call ssw_init + ssw_align (alnpe.c:260-393).  out6: score1, score2, ref_begin, ref_end, read_begin, read_end.  Every row is filled; when
// cases overflow (ctl.overflow: band beyond SW_BAND_W, more than SALT_MAX_CIGAR_OPS operations) their n_cigar is 0 and the call returns
// SALT_E_CAPACITY with their count in the message.
extern "C" int salt_gpu_diag_ssw(uint32_t n_cases, const uint8_t *aware, const uint8_t *ref_syms, const uint32_t *ref_offs,
                                 const uint8_t *codes, const uint32_t *read_offs, int32_t *out6, uint16_t *cigars, uint16_t *n_cigar)
{
    if (!aware || !ref_syms || !ref_offs || !codes || !read_offs || !out6 || !cigars || !n_cigar) return fail(SALT_E_INVAL, "null argument");
    if (n_cases == 0) return SALT_OK;
    const uint64_t n_sym = ref_offs[n_cases], n_base = read_offs[n_cases];
    std::vector<uint32_t> h_ref(n_sym / 8 + 8, 0u);
    std::vector<uint8_t> h_pac(n_sym / 4 + 8, 0);
    std::vector<PeSwReq> h_req(n_cases);
    uint32_t diag_max_len = 1;
    for (uint32_t i = 0; i < n_cases; ++i) {
        if (ref_offs[i + 1] <= ref_offs[i] || read_offs[i + 1] <= read_offs[i]) return fail(SALT_E_INVAL, "empty case");
        for (uint64_t p = ref_offs[i]; p < ref_offs[i + 1]; ++p) {
            h_ref[p >> 3] |= (uint32_t)(ref_syms[p] & 15u) << (4 * (p & 7u));
            h_pac[p >> 2] |= (uint8_t)((ref_syms[p] & 3u) << ((~p & 3u) << 1));
        }
        h_req[i] = PeSwReq{ ref_offs[i], ref_offs[i + 1] - 1, i, 0, (uint8_t)(aware[i] ? 1 : 0), 0 };
        if (read_offs[i + 1] - read_offs[i] > diag_max_len) diag_max_len = read_offs[i + 1] - read_offs[i];
    }
    if (diag_max_len > SALT_MAX_READ_LEN) return fail(SALT_E_INVAL, "read longer than SALT_MAX_READ_LEN");
    uint64_t diag_max_win = 1;
    for (uint32_t i = 0; i < n_cases; ++i) if (ref_offs[i + 1] - ref_offs[i] > diag_max_win) diag_max_win = ref_offs[i + 1] - ref_offs[i];
    uint32_t *d_ref = nullptr, *d_offs = nullptr; uint8_t *d_pac = nullptr, *d_codes = nullptr;
    auto done = [&](int rc) { hipFree(d_ref); hipFree(d_pac); hipFree(d_codes); hipFree(d_offs); return rc; };
    DONECHK(hipMalloc((void **)&d_ref, h_ref.size() * 4)); DONECHK(hipMemcpy(d_ref, h_ref.data(), h_ref.size() * 4, hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_pac, h_pac.size())); DONECHK(hipMemcpy(d_pac, h_pac.data(), h_pac.size(), hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_codes, n_base + 16)); DONECHK(hipMemcpy(d_codes, codes, n_base, hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_offs, ((uint64_t)n_cases + 1) * 4)); DONECHK(hipMemcpy(d_offs, read_offs, ((uint64_t)n_cases + 1) * 4, hipMemcpyHostToDevice));
    const uint32_t blocks = n_cases / 8 + 1 < 256 ? n_cases / 8 + 1 : 256;
    SwGeom geom = sw_geom(diag_max_len, diag_max_win, 1);
    geom.n_blocks = blocks; geom.tb_blocks = blocks;
    IndexView v; memset(&v, 0, sizeof v);
    v.ref = d_ref; v.ref_len = (uint32_t)n_sym;
    std::vector<PeSwRes> h_res; uint32_t n_over = 0;
    if (int rc = sw_run(v, d_pac, d_codes, d_offs, h_req, geom, diag_max_len, h_res, &n_over)) return done(rc);
    for (uint32_t i = 0; i < n_cases; ++i) {
        const PeSwRes &r = h_res[i];
        int32_t *o = out6 + 6 * (uint64_t)i;
        o[0] = r.score1; o[1] = r.score2; o[2] = r.ref_begin; o[3] = r.ref_end; o[4] = r.read_begin; o[5] = r.read_end;
        n_cigar[i] = r.n_cigar;
        memcpy(cigars + (uint64_t)i * SALT_MAX_CIGAR_OPS, r.cigar, sizeof r.cigar);
    }
    if (n_over) return done(fail(SALT_E_CAPACITY, std::to_string(n_over) + " case(s) need a band wider than SW_BAND_W or a CIGAR of more than "
                                 "SALT_MAX_CIGAR_OPS operations: their rows hold the scores and end points, and no CIGAR"));
    return done(SALT_OK);
}

extern "C" int salt_gpu_buffer_alloc(int device, uint64_t bytes, void **dev_ptr)
{
    if (!dev_ptr || !bytes) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipMalloc(dev_ptr, bytes));
    return SALT_OK;
}

extern "C" int salt_gpu_buffer_free(int device, void *dev_ptr)
{
    if (!dev_ptr) return SALT_OK;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipFree(dev_ptr));
    return SALT_OK;
}

__global__ void k_buffer_diff(const uint32_t *a, const uint32_t *b, uint64_t n_words, unsigned long long *n_diff)
{
    unsigned long long d = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (uint64_t)gridDim.x * blockDim.x) d += a[i] != b[i];
    if (d) atomicAdd(n_diff, d);
}

extern "C" int salt_gpu_buffer_equal(int device, const void *a, const void *b, uint64_t bytes, int *equal)
{
    if (!a || !b || !equal || (bytes & 3u)) return fail(SALT_E_INVAL, "bad buffer compare arguments (bytes must be a multiple of 4)");
    HIPCHK(hipSetDevice(device));
    unsigned long long *d = nullptr, h = 0;
    HIPCHK(hipMalloc((void **)&d, 8));
    HIPCHK(hipMemset(d, 0, 8));
    hipLaunchKernelGGL(k_buffer_diff, dim3(4096), dim3(256), 0, nullptr, static_cast<const uint32_t *>(a), static_cast<const uint32_t *>(b), bytes / 4, d);
    hipError_t e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
    hipFree(d);
    if (e != hipSuccess) return fail(SALT_E_HIP, std::string("buffer compare: ") + hipGetErrorString(e));
    *equal = h == 0;
    return SALT_OK;
}

// Unit access to the candidate rule (rule_unsorted / rule_sparse): see include/salt_gpu.h
extern "C" int salt_gpu_diag_rule(uint32_t n_cases, const uint32_t *pos, const uint8_t *val, const uint32_t *offs, const uint32_t *bound_in,
                                  uint32_t L, uint32_t ref_len, int mode, uint32_t *out)
{
    if (!pos || !val || !offs || !bound_in || !out) return fail(SALT_E_INVAL, "null argument");
    if (n_cases == 0) return SALT_OK;
    const uint64_t n = offs[n_cases];
    uint32_t *d_pos = nullptr, *d_offs = nullptr, *d_b = nullptr, *d_out = nullptr; uint8_t *d_val = nullptr;
    const uint64_t ow = (uint64_t)n_cases * diag_rule_words();
    HIPCHK(hipMalloc((void **)&d_pos, (n + 64) * 4)); HIPCHK(hipMemcpy(d_pos, pos, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_val, n + 64)); HIPCHK(hipMemcpy(d_val, val, n, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_offs, ((uint64_t)n_cases + 1) * 4)); HIPCHK(hipMemcpy(d_offs, offs, ((uint64_t)n_cases + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_b, (uint64_t)n_cases * 4)); HIPCHK(hipMemcpy(d_b, bound_in, (uint64_t)n_cases * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_out, ow * 4));
    launch_diag_rule(n_cases, d_pos, d_val, d_offs, d_b, L, ref_len, mode, d_out, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out, ow * 4, hipMemcpyDeviceToHost));
    hipFree(d_pos); hipFree(d_val); hipFree(d_offs); hipFree(d_b); hipFree(d_out);
    return SALT_OK;
}

// Unit entry of the rank primitives over an attached index (k_diag_occ): see include/salt_gpu.h
extern "C" int salt_gpu_diag_occ(const salt_gpu_index_t *ix, int mode, uint32_t n, const uint32_t *queries, uint32_t *out)
{
    if (!ix || (n && (!queries || !out))) return fail(SALT_E_INVAL, "null argument");
    if (mode != 0 && mode != 1) return fail(SALT_E_INVAL, "mode must be 0 (C) or 1 (R)");
    if (n == 0) return SALT_OK;
    const uint32_t hi = mode == 0 ? ix->hdr.c_seq_len : ix->hdr.r_text_len + 1, n_sym = mode == 0 ? 4u : 5u;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t *q = queries + 3 * (uint64_t)i;
        for (int e = 0; e < 2; ++e) if (q[e] > hi && !(mode == 0 && q[e] == 0xFFFFFFFFu)) return fail(SALT_E_INVAL, "query " + std::to_string(i) + ": index outside the primitive's range");
        if (q[2] >= n_sym) return fail(SALT_E_INVAL, "query " + std::to_string(i) + ": symbol outside the alphabet");
    }
    HIPCHK(hipSetDevice(ix->device));
    uint32_t *d_q = nullptr, *d_out = nullptr;
    auto done = [&](int rc) { hipFree(d_q); hipFree(d_out); return rc; };
    DONECHK(hipMalloc((void **)&d_q, (uint64_t)n * 12)); DONECHK(hipMemcpy(d_q, queries, (uint64_t)n * 12, hipMemcpyHostToDevice));
    DONECHK(hipMalloc((void **)&d_out, (uint64_t)n * 48));
    launch_diag_occ(ix->view, mode, n, d_q, d_out, nullptr);
    DONECHK(hipGetLastError());
    DONECHK(hipDeviceSynchronize());
    DONECHK(hipMemcpy(out, d_out, (uint64_t)n * 48, hipMemcpyDeviceToHost));
    return done(SALT_OK);
}

// Unit entry of k_pack (tests): the production launch on the caller's device buffers, no index and no workspace: see include/salt_gpu.h
extern "C" int salt_gpu_diag_pack(int device, uint32_t n_reads, uint32_t max_read_len, const void *d_seqs, const void *d_offs,
                                  void *d_pm, void *d_tb, void *hip_stream)
{
    if (!d_seqs || !d_offs || !d_pm || !d_tb) return fail(SALT_E_INVAL, "null argument");
    if (max_read_len > SALT_MAX_READ_LEN) return fail(SALT_E_INVAL, "max_read_len above " + std::to_string(SALT_MAX_READ_LEN));      // 0 reads as 1 (PackGeom::make)
    if (n_reads == 0) return SALT_OK;
    HIPCHK(hipSetDevice(device));
    launch_pack(PackGeom::make(max_read_len), n_reads, static_cast<const uint8_t *>(d_seqs), static_cast<const uint32_t *>(d_offs),
                static_cast<uint32_t *>(d_pm), static_cast<uint32_t *>(d_tb), static_cast<hipStream_t>(hip_stream));
    HIPCHK(hipGetLastError());
    return SALT_OK;
}

// Unit entry of the candidate verifiers on a caller-supplied mixRef (see k_diag_verify): fault-free check of the guards that keep a
// wrapped locate from being used as an address.
extern "C" int salt_gpu_diag_verify(const uint32_t *ref_words, uint32_t ref_len, uint32_t n_cases, const uint8_t *seqs, const uint32_t *offs,
                                    const uint32_t *cand, const uint32_t *cand_offs, int mode, uint8_t *out)
{
    if (!ref_words || !seqs || !offs || !cand || !cand_offs || !out) return fail(SALT_E_INVAL, "null argument");
    if (mode < 0 || mode > 7) return fail(SALT_E_INVAL, "mode must be 0..7");
    if (n_cases == 0) return SALT_OK;
    int n_dev = 0;
    HIPCHK(hipGetDeviceCount(&n_dev));
    if (n_dev <= 0) return fail(SALT_E_HIP, "no HIP device visible");
    for (uint32_t i = 0; i < n_cases; ++i) {
        const uint32_t L = offs[i + 1] - offs[i];
        if (L == 0 || L > SALT_MAX_READ_LEN || ((mode == 1 || mode == 3 || mode == 5 || mode == 7) && L > 120) || ((mode == 2 || mode == 4 || mode == 6) && L > 248)) return fail(SALT_E_INVAL, "read length outside the verifier's range");
        if (cand_offs[i + 1] - cand_offs[i] > 256) return fail(SALT_E_INVAL, "at most 256 candidates per case");
    }
    const uint64_t nw = ((uint64_t)ref_len + 7) / 8 + 36, bases = offs[n_cases], nc = cand_offs[n_cases];
    uint32_t *d_ref = nullptr, *d_offs = nullptr, *d_cand = nullptr, *d_coffs = nullptr; uint8_t *d_seqs = nullptr, *d_out = nullptr;
    HIPCHK(hipMalloc((void **)&d_ref, nw * 4)); HIPCHK(hipMemset(d_ref, 0, nw * 4));
    HIPCHK(hipMemcpy(d_ref, ref_words, (nw - 36) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_offs, ((uint64_t)n_cases + 1) * 4)); HIPCHK(hipMemcpy(d_offs, offs, ((uint64_t)n_cases + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_coffs, ((uint64_t)n_cases + 1) * 4)); HIPCHK(hipMemcpy(d_coffs, cand_offs, ((uint64_t)n_cases + 1) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_cand, (nc + 1) * 4)); HIPCHK(hipMemcpy(d_cand, cand, nc * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_seqs, bases + 64)); HIPCHK(hipMemcpy(d_seqs, seqs, bases, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void **)&d_out, nc + 1));
    launch_diag_verify(d_ref, ref_len, n_cases, d_seqs, d_offs, d_cand, d_coffs, mode, d_out, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, d_out, nc, hipMemcpyDeviceToHost));
    hipFree(d_ref); hipFree(d_offs); hipFree(d_coffs); hipFree(d_cand); hipFree(d_seqs); hipFree(d_out);
    return SALT_OK;
}

extern "C" int salt_gpu_ws_queue_counts(salt_gpu_ws_t *ws, uint32_t out[8])
{
    if (!ws || !out) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(ws->ix->device));
    HIPCHK(hipDeviceSynchronize());
    SeCtl c; HIPCHK(hipMemcpy(&c, ws->d_qctl, sizeof c, hipMemcpyDeviceToHost));
    memset(out, 0, 32);
    out[0] = c.light_queued; out[2] = c.gap_slots; out[5] = c.gap_items; out[6] = c.cigar_items; out[7] = c.cigar_head;
    {   // the reads k_light4 left to k_light_retry
        std::vector<QueueRange> qr(QUEUE_RANGES);
        HIPCHK(hipMemcpy(qr.data(), ws->d_ranges, qr.size() * sizeof(QueueRange), hipMemcpyDeviceToHost));
        for (const QueueRange &q : qr) out[4] += q.retry;
    }
    {   // the longest R list and the longest C list among the segments of k_seed's walk queues
        std::vector<uint32_t> wc(seed_wq_cnt_words());
        HIPCHK(hipMemcpy(wc.data(), ws->d_wq_cnt, wc.size() * 4, hipMemcpyDeviceToHost));
        const uint32_t per_list = seed_wq_cnt_words() / 2u, stride = per_list / 64u;
        for (uint32_t i = 0; i < 64u; ++i) { out[1] = std::max(out[1], wc[i * stride]); out[3] = std::max(out[3], wc[per_list + i * stride]); }
    }
    return SALT_OK;
}

extern "C" int salt_gpu_ws_heavy_reads(salt_gpu_ws_t *ws, uint32_t *ids, uint32_t cap, uint32_t *n)
{
    if (!ws || !n) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(ws->ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(n, &ws->d_qctl->light_queued, 4, hipMemcpyDeviceToHost));
    if (ids && cap) HIPCHK(hipMemcpy(ids, ws->d_queue, (uint64_t)(*n < cap ? *n : cap) * 4, hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_index_set_pac(salt_gpu_index_t *ix, const uint8_t *pac, uint64_t l_pac)
{
    if (!ix || !pac || l_pac == 0) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(ix->device));
    if (ix->d_pac) { hipFree(ix->d_pac); ix->d_pac = nullptr; }
    const uint64_t bytes = l_pac / 4 + 2;
    HIPCHK(hipMalloc((void **)&ix->d_pac, bytes + 16));
    HIPCHK(hipMemset(ix->d_pac, 0, bytes + 16));
    HIPCHK(hipMemcpy(ix->d_pac, pac, bytes, hipMemcpyHostToDevice));
    ix->l_pac = l_pac;
    return attach_r_ctx(ix, R_CTX_RESERVE_PAC);      // an index attached without the room for its R context records gets them now, if the room is there
}

// ---- the row tallies (in front of 4.6): what enabling one and taking a call's adds back share ----
// The null check, the MAPQ check under the tally's prefix, the device, `first` when the tally has no table yet, then the gate.
template <class First> static int tally_enable(salt_gpu_index_t *ix, salt_gpu_index::Tally salt_gpu_index::*gate, const char *prefix, int on, uint32_t min_mapq, First first)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (min_mapq > 255) return fail(SALT_E_INVAL, std::string(prefix) + ": min_mapq " + std::to_string(min_mapq) + " is above 255, the largest MAPQ");
    HIPCHK(hipSetDevice(ix->device));
    if (on) if (const int rc = first()) return rc;
    (ix->*gate).min_mapq = min_mapq; (ix->*gate).on = on != 0;
    return SALT_OK;
}
// n zeroed elements, or the tally's own message and an empty buffer
template <class T> static int alloc_zeroed(DevBuf<T> &b, uint64_t n, const char *prefix, const std::string &no_room)
{
    if (b.alloc(n) != hipSuccess) { (void)hipGetLastError(); return fail(SALT_E_NOMEM, std::string(prefix) + ": no room for " + no_room); }
    const hipError_t e = hipMemset(b.p, 0, n * sizeof(T));
    if (e != hipSuccess) { b.release(); return fail(SALT_E_HIP, std::string("hipMemset(") + prefix + "): " + hipGetErrorString(e)); }
    return SALT_OK;
}
// The workspace's last job once more with the job's "minus one" as delta: + (2^32 - 1) or + (2^64 - 1) = - 1 in the table's arithmetic.
// never: the message for an index whose `table` was never allocated; null: such an index has nothing to take back.
template <class Job, class Delta, class T>
static int tally_uncount(salt_gpu_ws_t *ws, salt_gpu_ws::LastJob<Job> salt_gpu_ws::*last_of, hipError_t (*launch)(const Job &, hipStream_t), Delta minus_one,
                         DevBuf<T> salt_gpu_index::*table, const char *never)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    if (never && !(ws->ix->*table).p) return fail(SALT_E_INVAL, never);
    salt_gpu_ws::LastJob<Job> &last = ws->*last_of;
    if (last.job.n_rec == 0) return SALT_OK;
    HIPCHK(hipSetDevice(ws->ix->device));
    Job c = last.job;
    c.delta = minus_one;
    last.job.n_rec = 0;
    HIPCHK(launch(c, last.st));
    HIPCHK(hipStreamSynchronize(last.st));
    return SALT_OK;
}

// ---- allele counts at the SNP sites ----
// The site table from view.ref (k_snp_bits, a scan of the windows' popcounts, k_snp_rank), for the tally named by `prefix`: the SNP counts
// and the genotype sums share it, and whichever is enabled first builds it.  Already built: SALT_OK.
static int snp_table_build(salt_gpu_index_t *ix, const char *prefix)
{
    if (ix->d_snp_tab) return SALT_OK;
    const std::string pre = std::string(prefix) + ": ";
    const uint32_t ref_len = ix->view.ref_len;
    if (ref_len == 0) return fail(SALT_E_INVAL, pre + "the index has an empty genome");
    const uint64_t n_win = ((uint64_t)ref_len + 63) / 64;
    DevBuf<uint32_t> cnt; DevBuf<uint8_t> tmp; DevBuf<SnpWin> tab;
    const size_t tmp_bytes = snp_scan_bytes(n_win);
    if (tab.alloc(n_win) != hipSuccess || cnt.alloc(n_win + 1) != hipSuccess || tmp.alloc(tmp_bytes ? tmp_bytes : 1) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SALT_E_NOMEM, pre + "no room for the site table: " + std::to_string(n_win * sizeof(SnpWin)) + " bytes (16 per 64 genome positions) and " +
                                  std::to_string((n_win + 1) * 4 + tmp_bytes) + " bytes of scratch while it is built");
    }
    HIPCHK(launch_snp_table(ix->view.ref, ref_len, n_win, tab, cnt, tmp, tmp_bytes, nullptr));
    uint32_t n_sites = 0;
    HIPCHK(hipMemcpy(&n_sites, cnt + n_win, 4, hipMemcpyDeviceToHost));
    ix->d_snp_tab.take(tab);                                                   // the index owns it from here
    ix->snp_win = n_win; ix->snp_sites = n_sites;
    return SALT_OK;
}

// The first enable builds the site table if the genotype sums have not, and the zeroed counts.
extern "C" int salt_gpu_index_snp_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq)
{
    return tally_enable(ix, &salt_gpu_index::snp, "snp counts", on, min_mapq, [&]() -> int {
        if (ix->d_snp_counts) return SALT_OK;
        if (const int rc = snp_table_build(ix, "snp counts")) return rc;
        const uint64_t rows = (uint64_t)ix->snp_sites + 1;                          // (one spare row: an index without sites still has a table)
        return alloc_zeroed(ix->d_snp_counts, rows * 4, "snp counts", "the counts: " + std::to_string(rows * 16) + " bytes (16 per site, " + std::to_string(ix->snp_sites) + " sites)");
    });
}

extern "C" int salt_gpu_index_snp_sites(salt_gpu_index_t *ix, uint32_t *n_sites, uint32_t *pos, uint64_t cap)
{
    if (!ix || !n_sites) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_snp_tab) return fail(SALT_E_INVAL, "snp counts: counting was never enabled on this index (salt_gpu_index_snp_enable)");      // (the genotype sums' enable builds the table too)
    *n_sites = ix->snp_sites;
    if (!pos || ix->snp_sites == 0) return SALT_OK;
    if (cap < ix->snp_sites) return fail(SALT_E_INVAL, "snp counts: room for " + std::to_string(cap) + " positions, the index has " + std::to_string(ix->snp_sites) + " sites");
    HIPCHK(hipSetDevice(ix->device));
    DevBuf<uint32_t> d_pos;
    if (d_pos.alloc(ix->snp_sites) != hipSuccess) { (void)hipGetLastError(); return fail(SALT_E_NOMEM, "snp counts: no room for " + std::to_string((uint64_t)ix->snp_sites * 4) + " bytes of site positions"); }
    HIPCHK(launch_snp_pos(ix->d_snp_tab, ix->snp_win, d_pos, nullptr));
    HIPCHK(hipMemcpy(pos, d_pos, (uint64_t)ix->snp_sites * 4, hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_index_snp_counts(salt_gpu_index_t *ix, uint32_t *counts, uint64_t cap_words, int reset)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_snp_counts) return fail(SALT_E_INVAL, "snp counts: counting was never enabled on this index (salt_gpu_index_snp_enable)");
    const uint64_t words = (uint64_t)ix->snp_sites * 4;
    if (counts && cap_words < words) return fail(SALT_E_INVAL, "snp counts: room for " + std::to_string(cap_words) + " words, the table has " + std::to_string(words) + " (4 per site)");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (counts && words) HIPCHK(hipMemcpy(counts, ix->d_snp_counts, words * 4, hipMemcpyDeviceToHost));
    if (reset && words) HIPCHK(hipMemset(ix->d_snp_counts, 0, words * 4));
    return SALT_OK;
}

extern "C" int salt_gpu_ws_snp_uncount(salt_gpu_ws_t *ws)
{
    return tally_uncount(ws, &salt_gpu_ws::snp_last, launch_snp_count, 0xFFFFFFFFu, &salt_gpu_index::d_snp_counts, nullptr);
}

// ---- coverage ----
static const char *const DEPTH_NEVER = "depth: depth was never enabled on this index (salt_gpu_index_depth_enable)";

extern "C" int salt_gpu_index_depth_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq)
{
    return tally_enable(ix, &salt_gpu_index::depth, "depth", on, min_mapq, [&]() -> int {
        if (ix->d_depth) return SALT_OK;
        if (ix->view.ref_len == 0) return fail(SALT_E_INVAL, "depth: the index has an empty genome");
        const uint64_t words = (uint64_t)ix->view.ref_len + 1;
        return alloc_zeroed(ix->d_depth, words, "depth", "the difference array: " + std::to_string(words * 4) + " bytes (4 per genome position)");
    });
}

extern "C" int salt_gpu_index_depth_reset(salt_gpu_index_t *ix)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_depth) return fail(SALT_E_INVAL, DEPTH_NEVER);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(ix->d_depth, 0, ((uint64_t)ix->view.ref_len + 1) * 4));
    return SALT_OK;
}

// first + n words inside the array, or the message that names the range
static int depth_range(const salt_gpu_index *ix, const char *what, uint64_t first, uint64_t n)
{
    const uint64_t words = (uint64_t)ix->view.ref_len + 1;
    if (first > words || n > words - first)
        return fail(SALT_E_INVAL, std::string("depth ") + what + ": words [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") leave the array's [0, " +
                                  std::to_string(ix->view.ref_len) + "]");
    return SALT_OK;
}

extern "C" int salt_gpu_index_depth_fetch(salt_gpu_index_t *ix, uint64_t first, uint64_t n, uint32_t *out)
{
    if (!ix || (!out && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_depth) return fail(SALT_E_INVAL, DEPTH_NEVER);
    if (const int rc = depth_range(ix, "fetch", first, n)) return rc;
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (n) HIPCHK(hipMemcpy(out, ix->d_depth + first, n * 4, hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_index_depth_add(salt_gpu_index_t *ix, uint64_t first, uint64_t n, const uint32_t *in)
{
    if (!ix || (!in && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_depth) return fail(SALT_E_INVAL, DEPTH_NEVER);
    if (const int rc = depth_range(ix, "add", first, n)) return rc;
    if (n == 0) return SALT_OK;
    HIPCHK(hipSetDevice(ix->device));
    DevBuf<uint32_t> d_in;
    if (d_in.alloc(n) != hipSuccess) { (void)hipGetLastError(); return fail(SALT_E_NOMEM, "depth add: no room for " + std::to_string(n * 4) + " bytes of words to add"); }
    HIPCHK(hipMemcpy(d_in, in, n * 4, hipMemcpyHostToDevice));
    HIPCHK(launch_depth_add(ix->d_depth + first, d_in, n, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return SALT_OK;
}

extern "C" int salt_gpu_index_depth_text_begin(salt_gpu_index_t *ix, const salt_depth_text_opt_t *opt)
{
    if (!ix || !opt) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_depth) return fail(SALT_E_INVAL, DEPTH_NEVER);
    if (!ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "depth text needs the contig table: call salt_gpu_index_set_contigs first");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (!ix->depth_text) ix->depth_text = depth_text_new();
    std::string err;
    const int rc = depth_text_begin(ix->depth_text, ix->d_depth, ix->view.ref_len, ix->d_c_off, ix->d_c_name_off, ix->d_c_names, ix->h_c_off, ix->c_name_max,
                                    opt->window, opt->tile_positions, opt->bgzf, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_index_depth_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes)
{
    if (!ix || !data || !n_bytes) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_depth) return fail(SALT_E_INVAL, DEPTH_NEVER);
    if (!ix->depth_text) return fail(SALT_E_INVAL, "depth text: no text was begun (salt_gpu_index_depth_text_begin)");
    HIPCHK(hipSetDevice(ix->device));
    std::string err;
    const int rc = depth_text_next(ix->depth_text, data, n_bytes, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_ws_depth_uncount(salt_gpu_ws_t *ws)
{
    return tally_uncount(ws, &salt_gpu_ws::depth_last, launch_depth_mark, 0xFFFFFFFFu, &salt_gpu_index::d_depth, DEPTH_NEVER);
}

// ---- the error profile ----
static const char *const ERRPROF_NEVER = "error profile: the profile was never enabled on this index (salt_gpu_index_errprof_enable)";
static const uint64_t ERRPROF_ALL = (uint64_t)SALT_ERRPROF_CELLS + 16;      // E, then R

extern "C" int salt_gpu_index_errprof_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq)
{
    return tally_enable(ix, &salt_gpu_index::errprof, "error profile", on, min_mapq, [&]() -> int {
        if (ix->d_errprof) return SALT_OK;
        return alloc_zeroed(ix->d_errprof, ERRPROF_ALL, "error profile", "the tables: " + std::to_string(ERRPROF_ALL * 8) + " bytes (8 per cell of E[2][512][95][4][4] and R[2][8])");
    });
}

extern "C" int salt_gpu_index_errprof_fetch(salt_gpu_index_t *ix, uint64_t *cells, uint64_t cap_cells, uint64_t rec[16], int reset)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_errprof) return fail(SALT_E_INVAL, ERRPROF_NEVER);
    if (cells && cap_cells < SALT_ERRPROF_CELLS)
        return fail(SALT_E_INVAL, "error profile: room for " + std::to_string(cap_cells) + " cells, the table has " + std::to_string((uint64_t)SALT_ERRPROF_CELLS) + " (2 x 512 x 95 x 4 x 4)");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (cells) HIPCHK(hipMemcpy(cells, ix->d_errprof, (uint64_t)SALT_ERRPROF_CELLS * 8, hipMemcpyDeviceToHost));
    if (rec) HIPCHK(hipMemcpy(rec, ix->d_errprof + SALT_ERRPROF_CELLS, 16 * 8, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(ix->d_errprof, 0, ERRPROF_ALL * 8));
    return SALT_OK;
}

extern "C" int salt_gpu_ws_errprof_uncount(salt_gpu_ws_t *ws)
{
    return tally_uncount(ws, &salt_gpu_ws::ep_last, launch_errprof, ~0ull, &salt_gpu_index::d_errprof, ERRPROF_NEVER);
}

// ---- genotypes at the SNP sites ----
static const char *const GT_NEVER = "genotype: the genotype sums were never enabled on this index (salt_gpu_index_gt_enable)";
static const uint64_t GT_WORDS = sizeof(salt_gt_site_t) / 8;               // 16 words a site

// The first enable builds the site table if the SNP counts have not, and the zeroed sums.
extern "C" int salt_gpu_index_gt_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq)
{
    return tally_enable(ix, &salt_gpu_index::gt, "genotype", on, min_mapq, [&]() -> int {
        if (ix->d_gt) return SALT_OK;
        if (const int rc = snp_table_build(ix, "genotype")) return rc;
        const uint64_t rows = (uint64_t)ix->snp_sites + 1;                          // (one spare row: an index without sites still has a table)
        return alloc_zeroed(ix->d_gt, rows * GT_WORDS, "genotype", "the sums: " + std::to_string(rows * sizeof(salt_gt_site_t)) + " bytes (128 per site, " + std::to_string(ix->snp_sites) + " sites)");
    });
}

extern "C" int salt_gpu_index_gt_reset(salt_gpu_index_t *ix)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_gt) return fail(SALT_E_INVAL, GT_NEVER);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(ix->d_gt, 0, ((uint64_t)ix->snp_sites + 1) * sizeof(salt_gt_site_t)));
    return SALT_OK;
}

// first + n sites inside the table, or the message that names the range
static int gt_range(const salt_gpu_index *ix, const char *what, uint64_t first, uint64_t n)
{
    const uint64_t sites = ix->snp_sites;
    if (first > sites || n > sites - first)
        return fail(SALT_E_INVAL, std::string("genotype ") + what + ": sites [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") leave the table's [0, " +
                                  std::to_string(sites) + ")");
    return SALT_OK;
}

extern "C" int salt_gpu_index_gt_fetch(salt_gpu_index_t *ix, uint64_t first_site, uint64_t n, salt_gt_site_t *out)
{
    if (!ix || (!out && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_gt) return fail(SALT_E_INVAL, GT_NEVER);
    if (const int rc = gt_range(ix, "fetch", first_site, n)) return rc;
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (n) HIPCHK(hipMemcpy(out, ix->d_gt + first_site * GT_WORDS, n * sizeof(salt_gt_site_t), hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_index_gt_add(salt_gpu_index_t *ix, uint64_t first_site, uint64_t n, const salt_gt_site_t *in)
{
    if (!ix || (!in && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_gt) return fail(SALT_E_INVAL, GT_NEVER);
    if (const int rc = gt_range(ix, "add", first_site, n)) return rc;
    if (n == 0) return SALT_OK;
    HIPCHK(hipSetDevice(ix->device));
    DevBuf<unsigned long long> d_in;
    if (d_in.alloc(n * GT_WORDS) != hipSuccess) { (void)hipGetLastError(); return fail(SALT_E_NOMEM, "genotype add: no room for " + std::to_string(n * sizeof(salt_gt_site_t)) + " bytes of sums to add"); }
    HIPCHK(hipMemcpy(d_in, in, n * sizeof(salt_gt_site_t), hipMemcpyHostToDevice));
    HIPCHK(launch_gt_sum(ix->d_gt + first_site * GT_WORDS, d_in, n * GT_WORDS, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return SALT_OK;
}

extern "C" int salt_gpu_index_gt_text_begin(salt_gpu_index_t *ix, const salt_gt_text_opt_t *opt)
{
    if (!ix || !opt) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_gt) return fail(SALT_E_INVAL, GT_NEVER);
    if (!ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "genotype text needs the contig table: call salt_gpu_index_set_contigs first");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (!ix->gt_text) ix->gt_text = gt_text_new();
    std::string err;
    const int rc = gt_text_begin(ix->gt_text, ix->d_gt, ix->d_snp_tab, ix->snp_win, ix->snp_sites, ix->view.ref, ix->view.text, ix->view.ref_len, ix->view.c_seq_len,
                                 ix->d_c_off, ix->d_c_name_off, ix->d_c_names, ix->n_contigs, ix->c_name_max, opt->tile_sites, opt->bgzf, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_index_gt_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes)
{
    if (!ix || !data || !n_bytes) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_gt) return fail(SALT_E_INVAL, GT_NEVER);
    if (!ix->gt_text) return fail(SALT_E_INVAL, "genotype text: no text was begun (salt_gpu_index_gt_text_begin)");
    HIPCHK(hipSetDevice(ix->device));
    std::string err;
    const int rc = gt_text_next(ix->gt_text, data, n_bytes, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_ws_gt_uncount(salt_gpu_ws_t *ws)
{
    return tally_uncount(ws, &salt_gpu_ws::gt_last, launch_gt_add, ~0ull, &salt_gpu_index::d_gt, GT_NEVER);
}

// ---- SNP candidates off the index's sites ----
static const char *const DISC_NEVER = "discover: the candidate arrays were never enabled on this index (salt_gpu_index_disc_enable)";

// The first enable allocates and zeroes both arrays: 8 + 4 bytes a genome position.
extern "C" int salt_gpu_index_disc_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq, uint32_t min_baseq)
{
    if (min_baseq > 93) return fail(SALT_E_INVAL, "discover: min_baseq " + std::to_string(min_baseq) + " is above 93, the largest base quality");
    const int rc = tally_enable(ix, &salt_gpu_index::disc, "discover", on, min_mapq, [&]() -> int {
        if (ix->d_disc_alt) return SALT_OK;
        const uint64_t n = ix->view.ref_len;
        if (n == 0) return fail(SALT_E_INVAL, "discover: the index has an empty genome");
        const std::string size = std::to_string(n * 8 + (n + 1) * 4) + " bytes (8 + 4 per genome position)";
        DevBuf<unsigned long long> alt; DevBuf<uint32_t> diff;
        if (const int rc = alloc_zeroed(alt, n, "discover", "the candidate arrays: " + size)) return rc;
        if (const int rc = alloc_zeroed(diff, n + 1, "discover", "the candidate arrays: " + size)) return rc;
        ix->d_disc_alt.take(alt); ix->d_disc_diff.take(diff);                      // the index owns them from here
        return SALT_OK;
    });
    if (rc == SALT_OK) ix->disc_min_baseq = min_baseq;
    return rc;
}

extern "C" int salt_gpu_index_disc_reset(salt_gpu_index_t *ix)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_disc_alt) return fail(SALT_E_INVAL, DISC_NEVER);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(ix->d_disc_alt, 0, (uint64_t)ix->view.ref_len * 8));
    HIPCHK(hipMemset(ix->d_disc_diff, 0, ((uint64_t)ix->view.ref_len + 1) * 4));
    return SALT_OK;
}

// first + n words inside the array `which` names, or the message that names the range
static int disc_range(const salt_gpu_index *ix, const char *what, int which, uint64_t first, uint64_t n)
{
    if (which != SALT_DISC_ALT && which != SALT_DISC_DIFF) return fail(SALT_E_INVAL, std::string("discover ") + what + ": array " + std::to_string(which) + " is neither SALT_DISC_ALT (0) nor SALT_DISC_DIFF (1)");
    const uint64_t words = (uint64_t)ix->view.ref_len + (which == SALT_DISC_DIFF ? 1 : 0);
    if (first > words || n > words - first)
        return fail(SALT_E_INVAL, std::string("discover ") + what + ": words [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") leave " +
                                  (which == SALT_DISC_DIFF ? "diff's" : "alt's") + " [0, " + std::to_string(words) + ")");
    return SALT_OK;
}

extern "C" int salt_gpu_index_disc_fetch(salt_gpu_index_t *ix, int which, uint64_t first, uint64_t n, void *out)
{
    if (!ix || (!out && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_disc_alt) return fail(SALT_E_INVAL, DISC_NEVER);
    if (const int rc = disc_range(ix, "fetch", which, first, n)) return rc;
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (n && which == SALT_DISC_ALT) HIPCHK(hipMemcpy(out, ix->d_disc_alt + first, n * 8, hipMemcpyDeviceToHost));
    if (n && which == SALT_DISC_DIFF) HIPCHK(hipMemcpy(out, ix->d_disc_diff + first, n * 4, hipMemcpyDeviceToHost));
    return SALT_OK;
}

// The adds are the 64-bit and 32-bit word sums of the genotype sums and of the coverage: one kernel a width.
extern "C" int salt_gpu_index_disc_add(salt_gpu_index_t *ix, int which, uint64_t first, uint64_t n, const void *in)
{
    if (!ix || (!in && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_disc_alt) return fail(SALT_E_INVAL, DISC_NEVER);
    if (const int rc = disc_range(ix, "add", which, first, n)) return rc;
    if (n == 0) return SALT_OK;
    HIPCHK(hipSetDevice(ix->device));
    const uint64_t bytes = n * (which == SALT_DISC_ALT ? 8 : 4);
    DevBuf<uint8_t> d_in;
    if (d_in.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); return fail(SALT_E_NOMEM, "discover add: no room for " + std::to_string(bytes) + " bytes of words to add"); }
    HIPCHK(hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice));
    if (which == SALT_DISC_ALT) HIPCHK(launch_gt_sum(ix->d_disc_alt + first, reinterpret_cast<const unsigned long long *>(d_in.p), n, nullptr));
    else HIPCHK(launch_depth_add(ix->d_disc_diff + first, reinterpret_cast<const uint32_t *>(d_in.p), n, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return SALT_OK;
}

extern "C" int salt_gpu_index_disc_text_begin(salt_gpu_index_t *ix, const salt_disc_text_opt_t *opt)
{
    if (!ix || !opt) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_disc_alt) return fail(SALT_E_INVAL, DISC_NEVER);
    if (opt->min_alt < 1 || opt->min_alt > SALT_DISC_FIELD_MAX) return fail(SALT_E_INVAL, "discover text: min_alt " + std::to_string(opt->min_alt) + " is outside 1 .. 2097151");
    if (opt->min_pct > 100) return fail(SALT_E_INVAL, "discover text: min_pct " + std::to_string(opt->min_pct) + " is above 100");
    if (!ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "discover text needs the contig table: call salt_gpu_index_set_contigs first");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (!ix->disc_text) ix->disc_text = disc_text_new();
    std::string err;
    const int rc = disc_text_begin(ix->disc_text, ix->d_disc_alt, ix->d_disc_diff, ix->view.ref, ix->view.text, ix->view.ref_len, ix->view.c_seq_len,
                                   ix->d_c_off, ix->d_c_name_off, ix->d_c_names, ix->n_contigs, ix->c_name_max, opt->min_alt, opt->min_pct, opt->all_sites,
                                   opt->tile_positions, opt->bgzf, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_index_disc_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes)
{
    if (!ix || !data || !n_bytes) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_disc_alt) return fail(SALT_E_INVAL, DISC_NEVER);
    if (!ix->disc_text) return fail(SALT_E_INVAL, "discover text: no text was begun (salt_gpu_index_disc_text_begin)");
    HIPCHK(hipSetDevice(ix->device));
    std::string err;
    const int rc = disc_text_next(ix->disc_text, data, n_bytes, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_index_disc_text_seen(salt_gpu_index_t *ix, uint8_t *seen, uint64_t cap)
{
    if (!ix || !seen) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_disc_alt) return fail(SALT_E_INVAL, DISC_NEVER);
    if (!ix->disc_text) return fail(SALT_E_INVAL, "discover text: no text was begun (salt_gpu_index_disc_text_begin)");
    HIPCHK(hipSetDevice(ix->device));
    std::string err;
    const int rc = disc_text_seen(ix->disc_text, seen, cap, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_ws_disc_uncount(salt_gpu_ws_t *ws)
{
    return tally_uncount(ws, &salt_gpu_ws::disc_last, launch_disc_add, ~0ull, &salt_gpu_index::d_disc_alt, DISC_NEVER);
}

// ---- the run's summary ----
static const char *const STATS_NEVER = "stats: the tables were never enabled on this index (salt_gpu_index_stats_enable)";

extern "C" int salt_gpu_index_stats_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq)
{
    return tally_enable(ix, &salt_gpu_index::stats, "stats", on, min_mapq, [&]() -> int {
        if (!ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "stats needs the contig table for its per-contig counts: call salt_gpu_index_set_contigs first");
        if (ix->d_stats) {
            if (ix->n_contigs == ix->stats_contigs) return SALT_OK;
            return fail(SALT_E_INVAL, "stats: the contig table was set again with " + std::to_string(ix->n_contigs) + " contigs, the tables were made for " + std::to_string(ix->stats_contigs));
        }
        const uint64_t n = (uint64_t)SALT_STATS_CELLS + (uint64_t)ix->n_contigs * 8;
        if (const int rc = alloc_zeroed(ix->d_stats, n, "stats", "the tables: " + std::to_string(n * 8) + " bytes (8 per cell: " + std::to_string((uint64_t)SALT_STATS_CELLS) +
                                        " fixed cells and 8 for each of " + std::to_string(ix->n_contigs) + " contigs)")) return rc;
        ix->stats_contigs = ix->n_contigs;
        return SALT_OK;
    });
}

extern "C" int salt_gpu_index_stats_fetch(salt_gpu_index_t *ix, uint64_t *cells, uint64_t cap_cells, uint64_t *ct, uint64_t cap_ct, int reset)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_stats) return fail(SALT_E_INVAL, STATS_NEVER);
    const uint64_t n_ct = (uint64_t)ix->stats_contigs * 8;
    if (cells && cap_cells < SALT_STATS_CELLS)
        return fail(SALT_E_INVAL, "stats: room for " + std::to_string(cap_cells) + " cells, the fixed tables have " + std::to_string((uint64_t)SALT_STATS_CELLS));
    if (ct && cap_ct < n_ct)
        return fail(SALT_E_INVAL, "stats: room for " + std::to_string(cap_ct) + " cells of CT, the table has " + std::to_string(n_ct) + " (8 for each of " + std::to_string(ix->stats_contigs) + " contigs)");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (cells) HIPCHK(hipMemcpy(cells, ix->d_stats, (uint64_t)SALT_STATS_CELLS * 8, hipMemcpyDeviceToHost));
    if (ct) HIPCHK(hipMemcpy(ct, ix->d_stats + SALT_STATS_CELLS, n_ct * 8, hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(ix->d_stats, 0, ((uint64_t)SALT_STATS_CELLS + n_ct) * 8));
    return SALT_OK;
}

extern "C" int salt_gpu_ws_stats_uncount(salt_gpu_ws_t *ws)
{
    if (ws && ws->stats_last.job.n_rec) {                      // the contig table may have been set again since (with as many contigs): the job reads the one that stands
        if (!ws->ix->d_c_off || ws->ix->n_contigs != ws->stats_last.job.n_contigs) return fail(SALT_E_INVAL, "stats: the contig table changed since the call that is to be taken back");
        ws->stats_last.job.c_off = ws->ix->d_c_off;
    }
    return tally_uncount(ws, &salt_gpu_ws::stats_last, launch_stats_add, ~0ull, &salt_gpu_index::d_stats, STATS_NEVER);
}

// ---- indel candidates ----
static const char *const INDEL_NEVER = "indels: the table was never enabled on this index (salt_gpu_index_indel_enable)";

// The first enable allocates and zeroes the table (16 bytes a slot), the counters and the difference array (4 bytes a genome position).
extern "C" int salt_gpu_index_indel_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq, uint32_t log2_slots)
{
    if (log2_slots && (log2_slots < SALT_INDEL_LOG2_MIN || log2_slots > SALT_INDEL_LOG2_MAX))
        return fail(SALT_E_INVAL, "indels: log2_slots " + std::to_string(log2_slots) + " is outside 6 .. 28 (0: the default, 24)");
    return tally_enable(ix, &salt_gpu_index::indel, "indels", on, min_mapq, [&]() -> int {
        if (!ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "indels need the contig table (an allele stays inside its contig): call salt_gpu_index_set_contigs first");
        if (ix->d_indel) {
            if (log2_slots == 0 || log2_slots == ix->indel_log2) return SALT_OK;
            return fail(SALT_E_INVAL, "indels: the table has 2^" + std::to_string(ix->indel_log2) + " slots since the first enable, not 2^" + std::to_string(log2_slots));
        }
        const uint32_t lg = log2_slots ? log2_slots : SALT_INDEL_LOG2_DEFAULT;
        const uint64_t slots = 1ull << lg, n = ix->view.ref_len;
        if (n == 0) return fail(SALT_E_INVAL, "indels: the index has an empty genome");
        const std::string size = std::to_string(slots * 16 + 32 + (n + 1) * 4) + " bytes (16 for each of 2^" + std::to_string(lg) + " slots, 4 per genome position)";
        DevBuf<IndelSlot> tab; DevBuf<unsigned long long> stat; DevBuf<uint32_t> diff;
        if (const int rc = alloc_zeroed(tab, slots, "indels", "the table and the difference array: " + size)) return rc;
        if (const int rc = alloc_zeroed(stat, 4, "indels", "the table and the difference array: " + size)) return rc;
        if (const int rc = alloc_zeroed(diff, n + 1, "indels", "the table and the difference array: " + size)) return rc;
        ix->d_indel.take(tab); ix->d_indel_stat.take(stat); ix->d_indel_diff.take(diff); ix->indel_log2 = lg;      // the index owns them from here
        return SALT_OK;
    });
}

extern "C" int salt_gpu_index_indel_reset(salt_gpu_index_t *ix)
{
    if (!ix) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemset(ix->d_indel, 0, (16ull << ix->indel_log2)));
    HIPCHK(hipMemset(ix->d_indel_stat, 0, 32));
    HIPCHK(hipMemset(ix->d_indel_diff, 0, ((uint64_t)ix->view.ref_len + 1) * 4));
    return SALT_OK;
}

extern "C" int salt_gpu_index_indel_stats(salt_gpu_index_t *ix, uint64_t out[4])
{
    if (!ix || !out) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, ix->d_indel_stat, 32, hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_index_indel_fetch(salt_gpu_index_t *ix, uint64_t cap, uint64_t *entries, uint64_t *n)
{
    if (!ix || !n || (!entries && cap)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (!ix->indel_text) ix->indel_text = indel_text_new();
    std::string err; uint64_t live = 0; const unsigned long long *keys = nullptr, *vals = nullptr;
    if (const int rc = indel_sorted(ix->indel_text, ix->d_indel, ix->indel_log2, &live, &keys, &vals, err)) return fail(rc, err);
    *n = live;
    const uint64_t take = std::min(cap, live);
    if (take == 0) return SALT_OK;
    std::vector<uint64_t> k((size_t)take), v((size_t)take);
    HIPCHK(hipMemcpy(k.data(), keys, take * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(v.data(), vals, take * 8, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < take; ++i) { entries[2 * i] = k[(size_t)i]; entries[2 * i + 1] = v[(size_t)i]; }
    return SALT_OK;
}

extern "C" int salt_gpu_index_indel_add(salt_gpu_index_t *ix, const uint64_t *entries, uint64_t n)
{
    if (!ix || (!entries && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    if (n == 0) return SALT_OK;
    HIPCHK(hipSetDevice(ix->device));
    DevBuf<unsigned long long> d_in;
    if (d_in.alloc(n * 2) != hipSuccess) { (void)hipGetLastError(); return fail(SALT_E_NOMEM, "indels add: no room for " + std::to_string(n * 16) + " bytes of pairs to add"); }
    HIPCHK(hipMemcpy(d_in, entries, n * 16, hipMemcpyHostToDevice));
    HIPCHK(launch_indel_put(d_in, n, ix->d_indel, ix->indel_log2, ix->d_indel_stat, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return SALT_OK;
}

// first + n words inside diff's [0, ref_len], or the message that names the range
static int indel_diff_range(const salt_gpu_index *ix, const char *what, uint64_t first, uint64_t n)
{
    const uint64_t words = (uint64_t)ix->view.ref_len + 1;
    if (first > words || n > words - first)
        return fail(SALT_E_INVAL, std::string("indels ") + what + ": words [" + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(n) + ") leave diff's [0, " + std::to_string(words) + ")");
    return SALT_OK;
}

extern "C" int salt_gpu_index_indel_fetch_diff(salt_gpu_index_t *ix, uint64_t first, uint64_t n, uint32_t *out)
{
    if (!ix || (!out && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    if (const int rc = indel_diff_range(ix, "fetch", first, n)) return rc;
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (n) HIPCHK(hipMemcpy(out, ix->d_indel_diff + first, n * 4, hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_index_indel_add_diff(salt_gpu_index_t *ix, uint64_t first, uint64_t n, const uint32_t *in)
{
    if (!ix || (!in && n)) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    if (const int rc = indel_diff_range(ix, "add", first, n)) return rc;
    if (n == 0) return SALT_OK;
    HIPCHK(hipSetDevice(ix->device));
    DevBuf<uint32_t> d_in;
    if (d_in.alloc(n) != hipSuccess) { (void)hipGetLastError(); return fail(SALT_E_NOMEM, "indels add: no room for " + std::to_string(n * 4) + " bytes of words to add"); }
    HIPCHK(hipMemcpy(d_in, in, n * 4, hipMemcpyHostToDevice));
    HIPCHK(launch_depth_add(ix->d_indel_diff + first, d_in, n, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return SALT_OK;
}

extern "C" int salt_gpu_index_indel_text_begin(salt_gpu_index_t *ix, const salt_indel_text_opt_t *opt)
{
    if (!ix || !opt) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    if (opt->min_alt < 1) return fail(SALT_E_INVAL, "indel text: min_alt 0 is outside 1 .. 4294967295");
    if (opt->min_pct > 100) return fail(SALT_E_INVAL, "indel text: min_pct " + std::to_string(opt->min_pct) + " is above 100");
    if (!ix->d_c_off || ix->n_contigs < 1) return fail(SALT_E_INVAL, "indel text needs the contig table: call salt_gpu_index_set_contigs first");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipDeviceSynchronize());
    if (!ix->indel_text) ix->indel_text = indel_text_new();
    std::string err;
    const int rc = indel_text_begin(ix->indel_text, ix->d_indel, ix->indel_log2, ix->d_indel_diff, ix->view.text, ix->view.ref_len, ix->view.c_seq_len,
                                    ix->d_c_off, ix->d_c_name_off, ix->d_c_names, ix->n_contigs, ix->c_name_max, opt->min_alt, opt->min_pct, opt->tile_positions, opt->bgzf, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_index_indel_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes)
{
    if (!ix || !data || !n_bytes) return fail(SALT_E_INVAL, "null argument");
    if (!ix->d_indel) return fail(SALT_E_INVAL, INDEL_NEVER);
    if (!ix->indel_text) return fail(SALT_E_INVAL, "indel text: no text was begun (salt_gpu_index_indel_text_begin)");
    HIPCHK(hipSetDevice(ix->device));
    std::string err;
    const int rc = indel_text_next(ix->indel_text, data, n_bytes, err);
    return rc ? fail(rc, err) : SALT_OK;
}

extern "C" int salt_gpu_ws_indel_uncount(salt_gpu_ws_t *ws)
{
    if (ws && ws->indel_last.job.n_rec) {                      // the contig table may have been set again since: the job reads the one that stands
        if (!ws->ix->d_c_off || ws->ix->n_contigs < 1) return fail(SALT_E_INVAL, "indels: the contig table is gone since the call that is to be taken back");
        ws->indel_last.job.c_off = ws->ix->d_c_off; ws->indel_last.job.n_contigs = ws->ix->n_contigs;
    }
    return tally_uncount(ws, &salt_gpu_ws::indel_last, launch_indel_add, ~0ull, &salt_gpu_index::d_indel, INDEL_NEVER);
}

extern "C" int salt_gpu_ws_set_quals(salt_gpu_ws_t *ws, const uint8_t *quals, int on_device)
{
    if (!ws) return fail(SALT_E_INVAL, "null argument");
    ws->q_next = quals; ws->q_next_dev = quals && on_device != 0;
    return SALT_OK;
}

extern "C" int salt_gpu_index_r_ctx(const salt_gpu_index_t *ix, void **dev_ptr, uint64_t *bytes)
{
    if (!ix || !dev_ptr || !bytes) return fail(SALT_E_INVAL, "null argument");
    *dev_ptr = ix->d_rctx; *bytes = ix->d_rctx ? ((uint64_t)ix->hdr.r_text_len + 1) * 16 : 0;
    return SALT_OK;
}

extern "C" int salt_gpu_ws_epoch(const salt_gpu_ws_t *ws, uint32_t *next_epoch)
{
    if (!ws || !next_epoch) return fail(SALT_E_INVAL, "null argument");
    *next_epoch = ws->epoch > SAI_EPOCH_MAX ? 1u : ws->epoch;      // past the last one: the next call zeroes the R rows and restarts
    return SALT_OK;
}

extern "C" int salt_gpu_ws_pe_overflow(salt_gpu_ws_t *ws, uint32_t *n)
{
    if (!ws || !n) return fail(SALT_E_INVAL, "null argument");
    *n = 0;
    if (!ws->d_pctl) return SALT_OK;
    HIPCHK(hipSetDevice(ws->ix->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(n, &ws->d_pctl->overflow, 4, hipMemcpyDeviceToHost));
    return SALT_OK;
}

extern "C" int salt_gpu_ws_pe_counts(salt_gpu_ws_t *ws, uint32_t out[8])
{
    if (!ws || !out) return fail(SALT_E_INVAL, "null argument");
    memset(out, 0, 32);
    if (!ws->d_pctl) return SALT_OK;
    HIPCHK(hipSetDevice(ws->ix->device));
    HIPCHK(hipDeviceSynchronize());
    PeCtl c; HIPCHK(hipMemcpy(&c, ws->d_pctl, sizeof c, hipMemcpyDeviceToHost));
    out[0] = c.n_req; out[2] = c.n_cigar; out[3] = c.cigar_head; out[4] = c.overflow; out[5] = c.diag_cols; out[6] = c.diag_clk;
    return SALT_OK;
}

static int pe_prepare(salt_gpu_ws_t *ws, uint32_t n_pairs, hipStream_t st)
{
    if (n_pairs > ws->d_pairs.cap) {
        HIPCHK(hipStreamSynchronize(st));
        ws->d_pairs.release(); ws->d_req.release(); ws->d_swres.release(); ws->d_pcq.release();
        HIPCHK(ws->d_pcq.alloc((uint64_t)n_pairs * 2));
        HIPCHK(ws->d_req.alloc((uint64_t)n_pairs * 2));
        HIPCHK(ws->d_swres.alloc((uint64_t)n_pairs * 2));
        HIPCHK(ws->d_pairs.alloc(n_pairs));                   // last: its capacity is the one compared, a failed allocation above leaves it empty
    }
    if (!ws->d_pctl) {
        HIPCHK(ws->d_pctl.alloc(1));
        hipDeviceProp_t prop;
        HIPCHK(hipGetDeviceProperties(&prop, ws->ix->device));
        ws->sw_blocks = (uint32_t)prop.multiProcessorCount;             // CUs: k_sw runs up to SW_MAX_BLOCKS_PER_CU blocks on each
    }
    return SALT_OK;
}

// everything of alnpe_core1 on device-resident buffers; only enqueues on st
static int pe_resident_impl(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_pe_opt_t *pe, uint32_t n_pairs, uint32_t max_len,
                            const void *d_seqs, const void *d_offs, void *d_results, hipStream_t st)
{
    int rc = pe_prepare(ws, n_pairs, st);
    if (rc) return rc;
    const uint32_t ti = ws->n_timed;
    rc = align_resident_impl(ws, o, 2 * n_pairs, max_len, d_seqs, d_offs, d_results, st, 1);
    if (rc) return rc;
    hipEvent_t *ev = ws->n_timed == ti + 1 ? &ws->ev[(size_t)ti * EV_PER_CALL] : nullptr;      // the call above was timed: three more events
    HIPCHK(hipMemsetAsync(ws->d_pctl, 0, sizeof(PeCtl), st));
    launch_pair(n_pairs, pe->min_tlen, pe->max_tlen, (uint32_t)ws->ix->l_pac, static_cast<const uint32_t *>(d_offs), static_cast<salt_result_t *>(d_results),
                ws->d_pairs, ws->d_req, ws->d_pctl, st);
    if (ev) HIPCHK(hipEventRecord(ev[8], st));
    // rescue windows are as long as the insert-size window plus a mate (alnpe.c:213-252, 395-480), whatever -a / -b say
    const uint64_t l_pac = (uint64_t)ws->ix->l_pac;
    uint64_t max_win = (uint64_t)pe->max_tlen + max_len + 2;
    if (max_win > l_pac + 1) max_win = l_pac + 1;
    SwGeom geom = sw_geom(max_len, max_win, ws->sw_blocks);
    // one group (8 lanes) per rescue in flight; rescues are a few per cent of the mates, so a small batch does not need the full grid
    sw_geom_limit(geom, n_pairs / 96u < 256u ? 256u : n_pairs / 96u);
    const uint64_t need = sw_scratch_bytes(geom);
    if (need > ws->d_sw_scr.cap) {
        HIPCHK(hipStreamSynchronize(st));
        const hipError_t e = ws->d_sw_scr.alloc(need);
        if (e != hipSuccess) return fail(SALT_E_NOMEM, std::string("hipMalloc(rescue scratch): ") + hipGetErrorString(e));
    }
    launch_sw(ws->ix->view, ws->ix->d_pac, static_cast<const uint8_t *>(d_seqs), static_cast<const uint32_t *>(d_offs), ws->d_req, ws->d_pctl, ws->d_swres,
              ws->d_sw_scr, geom, max_len, st);
    if (ev) HIPCHK(hipEventRecord(ev[9], st));
    launch_pe_final(ws->ix->view, PackGeom::make(max_len), n_pairs, ws->d_pm, static_cast<salt_result_t *>(d_results), ws->d_pairs, ws->d_swres, ws->d_lvtab,
                    ws->d_pcq, ws->d_pctl, ws->heavy_blocks, st);
    if (ev) { HIPCHK(hipEventRecord(ev[10], st)); ws->ev_pe[ti] = 1; }
#ifdef SALT_DIAG
    if (getenv("SALT_GPU_TB_CLOCKS")) {
        PeCtl c; HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipMemcpy(&c, ws->d_pctl, sizeof c, hipMemcpyDeviceToHost)); const uint32_t *t = c.tb_clk;
        if (t[3]) fprintf(stderr, "[k_swtb] %u tracebacks: operands %.1f us, band passes %.1f us, walk + write %.1f us each (s_memtime, 10 ns ticks)\n", t[3],
                          t[0] / 100.0 / t[3], t[1] / 100.0 / t[3], t[2] / 100.0 / t[3]);
    }
#endif
    HIPCHK(hipGetLastError());
    return rows_hooks(ws, 2 * n_pairs, d_seqs, d_offs, d_results, pe, st);
}

extern "C" int salt_gpu_align_pe_resident(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_pe_opt_t *pe, uint32_t n_pairs,
                                          uint32_t max_read_len, const void *d_seqs, const void *d_offs, void *d_results, void *hip_stream)
{
    if (!ws || !o || !pe || !d_seqs || !d_offs || !d_results) return fail(SALT_E_INVAL, "null argument");
    if (n_pairs == 0) return SALT_OK;
    if (2ull * n_pairs > ws->max_reads) return fail(SALT_E_CAPACITY, "more mates than the workspace holds");
    if (!ws->ix->d_pac) return fail(SALT_E_INVAL, "paired end needs the 2-bit genome: call salt_gpu_index_set_pac first");
    HIPCHK(hipSetDevice(ws->ix->device));
    if (int rc = quals_take(ws)) return rc;
    return pe_resident_impl(ws, o, pe, n_pairs, max_read_len, d_seqs, d_offs, d_results, static_cast<hipStream_t>(hip_stream));
}

extern "C" int salt_gpu_align_pe(salt_gpu_ws_t *ws, const salt_aln_opt_t *o, const salt_pe_opt_t *pe, uint32_t n_pairs,
                                 const uint8_t *seqs, const uint32_t *offs, salt_result_t *results)
{
    if (!ws || !o || !pe || !seqs || !offs || !results) return fail(SALT_E_INVAL, "null argument");
    if (n_pairs == 0) return SALT_OK;
    const uint32_t n_reads = 2 * n_pairs;
    if (n_reads > ws->max_reads) return fail(SALT_E_CAPACITY, "more mates than the workspace holds");
    if (!ws->ix->d_pac) return fail(SALT_E_INVAL, "paired end needs the 2-bit genome: call salt_gpu_index_set_pac first");
    if (offs[0] != 0) return fail(SALT_E_INVAL, "offs[0] must be 0");
    const uint64_t bases = offs[n_reads];
    if (bases > ws->max_bases) return fail(SALT_E_CAPACITY, "more bases than the workspace holds");
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n_reads; ++i) {
        if (offs[i + 1] <= offs[i]) return fail(SALT_E_INVAL, "empty read or decreasing offsets");
        const uint32_t l = offs[i + 1] - offs[i];
        max_len = l > max_len ? l : max_len;
    }
    HIPCHK(hipSetDevice(ws->ix->device));
    hipStream_t st = ws->stream;
    HIPCHK(hipMemcpyAsync(ws->d_seqs, seqs, bases, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ws->d_offs, offs, ((uint64_t)n_reads + 1) * 4, hipMemcpyHostToDevice, st));
    int rc = quals_upload(ws, bases, st);
    if (!rc) rc = quals_take(ws);
    if (rc) return rc;
    rc = pe_resident_impl(ws, o, pe, n_pairs, max_len, ws->d_seqs, ws->d_offs, ws->d_results, st);
    if (rc) return rc;
    rc = fetch_results(ws, n_reads, results, st);
    if (rc) return rc;
    uint32_t n_over = 0;
    rc = salt_gpu_ws_pe_overflow(ws, &n_over);
    if (rc) return rc;
    if (n_over) return fail(SALT_E_CAPACITY, std::to_string(n_over) + " mate rescue(s) need a Smith-Waterman band wider than this build holds (SW_BAND_W) "
                                             "or a CIGAR of more than SALT_MAX_CIGAR_OPS operations: the rows of this batch would differ from the reference's");
    return SALT_OK;
}

extern "C" int salt_gpu_ws_counters(salt_gpu_ws_t *ws, uint64_t out[SALT_CTR_N])
{
    if (!ws || !out) return fail(SALT_E_INVAL, "null argument");
    HIPCHK(hipSetDevice(ws->ix->device));
    HIPCHK(hipDeviceSynchronize());
    unsigned long long tmp[SALT_CTR_N];
    HIPCHK(hipMemcpy(tmp, ws->d_ctr, sizeof tmp, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(ws->d_ctr, 0, sizeof tmp));
    for (int i = 0; i < SALT_CTR_N; ++i) out[i] = tmp[i];
    return SALT_OK;
}
