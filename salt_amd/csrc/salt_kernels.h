// salt_amd/csrc/salt_kernels.h -- host-visible declarations of the kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>
#include <vector>
#include "../../include/salt_gpu.h"
#include "salt_device.h"
#include "salt_trim_rule.h"

// Diagnostics that CHANGE results (phase timing by leaving kernels early) exist only in -DSALT_DIAG builds (`make DIAG=1`): the release
// library has neither the environment switches nor the code paths behind them (tests/test_release_build.py greps for the names).
#ifdef SALT_DIAG
#define SALT_DIAG_VAL(x) (x)
#else
#define SALT_DIAG_VAL(x) 0
#endif

namespace salt {

// Per-batch packed copies of the reads (k_pack), fixed stride per read so that no kernel waits for offs[]:
//   pm record (pm_stride words): one-hot nibble words (nt2bit, editdistance.c:40), 8 bases per word, base i in bits
//       4*(i%8)..+3 (the mixRef layout): words [0, nw8) forward strand, [nw8, 2*nw8) reverse complement, [2*nw8] = L
//   tb record (tb_stride words): 2-bit codes, 16 bases per word, base i in bits 30-2*(i%16) (first base highest, so a
//       k-mer is a funnel shift): [0, nw16) forward, [nw16, 2*nw16) reverse complement; then 'is N' bits, 32 bases
//       per word, base i in bit 31-(i%32): [2*nw16, +nw32) forward, [.., +nw32) reverse; then L
struct PackGeom {
    uint32_t nw8, nw16, nw32, pm_stride, tb_stride;
    __host__ __device__ static PackGeom make(uint32_t max_len)
    {
        if (max_len < 1) max_len = 1;
        PackGeom g; g.nw8 = (max_len + 7) / 8; g.nw16 = (max_len + 15) / 16; g.nw32 = (max_len + 31) / 32;
        g.pm_stride = (2 * g.nw8 + 1 + 3) & ~3u; g.tb_stride = (2 * g.nw16 + 2 * g.nw32 + 1 + 3) & ~3u;
        return g;
    }
};

struct SeedParams {
    uint32_t n_reads, spr;          // spr: seed slots per (read, strand) = ceil((Lmax-k+1)/overlap)
    int32_t  l_seed, l_overlap;
    uint32_t max_seed;
    int32_t  seed_only_ref;
    int32_t  resolve_unique;        // finish one-row C intervals against the genome text (k_seed)
    uint32_t epoch;                 // the call's epoch (1 .. 2^24 - 1): k_seed_walk stores it in the live R rows (sai_r_pack, salt_device.h)
    PackGeom pg;
};

struct AlignParams {
    uint32_t n_reads, spr;
    int32_t  l_seed;
    uint32_t max_locate;
    int32_t  max_hits;
    PackGeom pg;
    int32_t  dbg_stop;              // debug/A-B: k_light leaves after phase dbg_stop (1..4); results are then garbage
    int32_t  heavy_stop;            // diagnostics: k_heavy leaves a read after its locate (1), verify (2) or rule (3) passes; results are then garbage
    int32_t  all_heavy;             // debug/A-B: skip k_light, k_heavy walks reads 0..n_reads-1
    int32_t  pe;                    // 1: mates of a paired-end batch -- alnse_overlap semantics (alnse.c:985-1044, 501-629):
                                    //    per-interval locate cap, gapped bound stays 3, > 5 N skips the mate
    uint32_t max_amb;               // reads with more N than this are left untouched (200 SE / 5 PE)
    uint32_t epoch;                 // the call's epoch: an R row of another call is dead (sai_r_row, salt_device.h)
};
static const uint32_t PE_LOCI_CAP = 0x40000;    // loci per strand a PE mate may enumerate = MAX_LOC_POS (alnse.c:42,533); global scratch

void launch_pack(const PackGeom &pg, uint32_t n_reads, const uint8_t *seqs, const uint32_t *offs, uint32_t *pm, uint32_t *tb, hipStream_t st);
// k_seed (W-mer gather, in-register resolves, walks queued) + k_seed_walk (the queued walks, one per lane).  wq: seed_wq_words(items) words
// (a walk record is 32 bytes: the seed, its interval and its five tb words), wq_cnt: seed_wq_cnt_words() words, which the caller has
// zeroed on the stream; walk_blocks: 256-lane blocks of the walk kernel (CUs x 2: two waves per SIMD)
void launch_seed(const IndexView &ix, const SeedParams &sp, const uint32_t *tb, uint4 *sai_c, uint4 *sai_r, uint4 *wq, uint32_t *wq_cnt,
                 uint32_t walk_blocks, unsigned long long *ctr, hipStream_t st);
size_t seed_wq_words(uint64_t items);
uint32_t seed_wq_cnt_words();
// The queues of the Smith-Waterman kernels and k_cigar.  All pulls of a launch on one counter are served one after the other (~14 ns each),
// also when every puller asks for its first item at once, or finds the queue empty.  So the FIRST item of a puller is its own index (no
// atomic), the counter hands out what lies behind those, and a puller looks at the counter (a plain load) before it adds to it.
// n_first: items the static first round covers (pullers x step).  Returns the item index, >= n_items when there is none.
__device__ __forceinline__ uint32_t sw_pull(uint32_t *head, const uint32_t step, const uint32_t n_first, const uint32_t n_items)
{
    if (n_first >= n_items || n_first + __hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n_items) return 0xFFFFFFFFu;
    return n_first + atomicAdd(head, step);
}
// Control words of a single-end batch, a 128-byte line each: atomics on one line are served one after the other (~14 ns each) however
// many waves issue them, and k_heavy's gapped reads push through three of these words.  Zeroed per batch.
struct SeCtl {
    alignas(128) uint32_t light_queued;     // reads k_light queued for k_heavy (k_queue_pack)
    alignas(128) uint32_t gap_slots;        // gapped reads given a k_gap slot
    alignas(128) uint32_t gap_items;        // k_gap items
    alignas(128) uint32_t cigar_items;      // k_cigar items
    alignas(128) uint32_t cigar_head;       // k_cigar's queue head
    alignas(128) uint32_t pool_used;        // located rows in the gapped passes' pool
    alignas(128) uint32_t ovq_count;        // reads in k_heavy's overflow queue
    alignas(128) uint32_t ovq_head;         // its head
};
static_assert(sizeof(SeCtl) == 8 * 128 && alignof(SeCtl) == 128, "one control word per 128-byte line");
// One range of k_heavy's queue, 256 bytes: the counter k_light's reads of that range are pushed through, and the heads k_heavy, k_gap and
// k_gapfin pull the range's items from (pop_ranged), a 128-byte line apart from the counter; behind the heads the counter of the reads
// k_light4 leaves to k_light_retry (nobody pulls while they push).  QUEUE_RANGES of them, zeroed per batch.
static const uint32_t QUEUE_RANGES = 64;
struct QueueRange {
    enum { HEAVY, GAP, GAPFIN };            // heads[]: k_heavy's, k_gap's, k_gapfin's
    uint32_t push, pad0[31], heads[3], retry, pad1[28];
};
static_assert(sizeof(QueueRange) == 256 && offsetof(QueueRange, push) == 0 && offsetof(QueueRange, heads) == 128, "k_light's counter, then the heads");
void launch_light(const IndexView &ix, const AlignParams &ap, const uint32_t *pm, const uint8_t *seqs, const uint32_t *offs, const uint4 *sai_c,
                  const uint4 *sai_r, salt_result_t *results, uint32_t *queue, SeCtl *ctl, uint32_t *qseg, QueueRange *ranges, unsigned long long *ctr, hipStream_t st);
size_t queue_words(uint32_t max_reads);                      // d_queue: the flat queue, k_heavy's overflow queue, k_light's segments, k_light4's retry segments
// Deferred gapped passes (k_heavy -> k_gap -> k_gapfin -> k_cigar), `cap` slots; gctl = the workspace's control words
struct GapBufs {
    uint32_t *gq;        // [cap] read index of the slot (0xFFFFFFFF: not used after all)
    uint32_t *gn;        // [cap][2] located rows per strand
    uint32_t *goff;      // [cap][2] where they start in the pool
    uint32_t *gloci;     // [pool] located positions, unsorted, duplicates included
    uint8_t  *ge;        // [pool] their Landau-Vishkin distances (255 = none within the bound)
    uint32_t *gitems;    // k_gap items: (slot << 11) | (strand << 10) | chunk of 32 candidates
    uint32_t *cq;        // k_cigar items: (read << 3) | which (0 = the alignment, 1 + i = alternative hit i)
    SeCtl *gctl;
    uint32_t cap, pool, items_cap;
    uint32_t *ovq;       // reads k_heavy's small shape could not finish (launch_heavy)
    QueueRange *ranges;  // k_heavy's queue ranges and their heads (launch_heavy)
};
GapBufs gap_bufs_layout(uint8_t *base, uint32_t cap, SeCtl *gctl, size_t *bytes);   // base = nullptr: size only
void launch_heavy(const IndexView &ix, const AlignParams &ap, const uint32_t *pm, const uint4 *sai_c,
                  const uint4 *sai_r, salt_result_t *results, const uint32_t *queue, unsigned long long *ctr,
                  uint32_t n_blocks, uint32_t gap_blocks, uint32_t cigar_blocks, void *lvtab, const GapBufs &g, uint32_t *ovq, QueueRange *ranges, uint8_t *pe_scr, hipEvent_t *ev3, hipStream_t st);
size_t lv_table_bytes();                // per-block LV traceback table (global memory)

// ---- paired end (salt_pe.hip) ----
static const uint32_t SW_MAX_SEG = 64;              // stripes: reads up to 512 bases
static const uint32_t SW_BAND_W = 1100;             // ints per banded-SW row buffer (band width <= 548)
// Scratch of one Smith-Waterman launch, sized per call from the batch (sw_geom): k_sw's 8-lane groups keep the per-column maxima of the
// longest rescue window the insert-size options allow (2 B per column); k_swtb's groups three band rows and one direction byte per cell for
// alignments whose band outgrows its LDS (bands up to SW_BAND_W cells).
struct SwGeom {
    uint32_t maxcol_bytes, n_blocks;           // k_sw
    uint32_t tb_group_bytes, tb_blocks;        // k_swtb
};
SwGeom sw_geom(uint32_t max_len, uint64_t max_window, uint32_t cus);
void sw_geom_limit(SwGeom &g, uint32_t blocks);            // small batches: no more blocks than that (and their scratch)
uint64_t sw_scratch_bytes(const SwGeom &g);
struct PeSwReq { uint32_t start, end, mate; uint8_t strand, aware; uint16_t pad; };          // mate: index of the rescued mate (2p or 2p+1);
                                                                                            // aware: 0 plain, 1 SNP-aware, 2 polish matrix; pad bit 0: score only, bit 1: mate rescue (no CIGAR for spans under 20 bases)
struct PeSwRes { int32_t score1, score2, ref_begin, ref_end, read_begin, read_end; uint32_t start, strand; uint16_t n_cigar, ok; uint16_t cigar[SALT_MAX_CIGAR_OPS]; };
struct PePair { uint32_t req0; uint8_t n_req; uint8_t rescued[2]; uint8_t pad; };             // requests req0 .. req0+n_req-1, in the order tried
// Control words of a paired-end batch, zeroed per batch.  The four Smith-Waterman queue heads share one line.
struct PeCtl {
    uint32_t n_req, unused1;          // Smith-Waterman requests (k_pair)
    uint32_t n_cigar, cigar_head;     // k_cigar items of the mates k_pe_final leaves gapped, and their queue head
    uint32_t overflow;                // rescues this build cannot finish as the reference would (launch_sw)
    uint32_t diag_cols, diag_clk, unused7;      // diagnostics build: k_swf's phase clock or the column counts; k_swr's phase clock
    uint32_t tb_clk[4];               // diagnostics build: k_swtb's phase clocks (operands, band passes, walk + write) and tracebacks
    uint32_t sw_heads[4];             // the queue heads of k_swf, k_swf1, k_swr, k_swtb
    uint32_t swf1_pending;            // the requests k_swf leaves to k_swf1
};
static_assert(offsetof(PeCtl, n_cigar) == 8 && offsetof(PeCtl, overflow) == 16 && offsetof(PeCtl, diag_cols) == 20 && offsetof(PeCtl, tb_clk) == 32 &&
              offsetof(PeCtl, sw_heads) == 48 && offsetof(PeCtl, swf1_pending) == 64 && sizeof(PeCtl) == 68, "paired-end control words");
void launch_pair(uint32_t n_pairs, uint32_t min_tlen, uint32_t max_tlen, uint32_t l_pac, const uint32_t *offs, salt_result_t *res,
                 PePair *pairs, PeSwReq *req, PeCtl *ctl, hipStream_t st);
// k_swf (+ k_swf1: forward pass: scores, end point), k_swr (reverse pass: begin point), k_swtb (banded traceback -> CIGAR) on ctl->n_req
// requests.  ctl->overflow: rescues this build cannot finish as the reference would (window beyond the scratch, band beyond SW_BAND_W, more
// than SALT_MAX_CIGAR_OPS operations); the caller turns it into an error instead of returning rows that differ from the reference's
void launch_sw(const IndexView &ix, const uint8_t *pac, const uint8_t *seqs, const uint32_t *offs, const PeSwReq *req, PeCtl *ctl,
               PeSwRes *res, uint8_t *scratch, SwGeom g, uint32_t max_len, hipStream_t st);
static const uint32_t SW_MAX_BLOCKS_PER_CU = 16;   // one-wave blocks per CU at most
static const uint64_t SW_SCRATCH_TOTAL = 2ull << 30;   // k_swtb's grid shrinks before its groups' global scratch passes 2 GiB
uint32_t sw_blocks_per_cu(uint32_t max_len);
void launch_pe_final(const IndexView &ix, const PackGeom &pg, uint32_t n_pairs, const uint32_t *pm, salt_result_t *res, const PePair *pairs,
                     const PeSwRes *sw, void *lvtab, uint32_t *citems, PeCtl *ctl, uint32_t n_blocks, hipStream_t st);

uint32_t heavy_blocks_per_cu();
void launch_polish(const uint8_t *pac, const uint8_t *codes, const uint32_t *offs, const salt_polish_item_t *items, uint32_t n_items, const uint8_t *pool,
                   uint32_t pool_stride, int want_cigar, int32_t *dist, uint16_t *cigars, uint8_t *n_cigar, void *tabs, uint32_t n_blocks, hipStream_t st);
void launch_heads(const salt_result_t *res, uint32_t n, uint8_t *heads, hipStream_t st);   // heads[i] = first 128 bytes of res[i]
void launch_diag_rule(uint32_t n_cases, const uint32_t *pos, const uint8_t *val, const uint32_t *offs, const uint32_t *bound_in,
                      uint32_t L, uint32_t ref_len, int mode, uint32_t *out, hipStream_t st);
uint32_t diag_rule_words();
void launch_diag_verify(const uint32_t *ref, uint32_t ref_len, uint32_t n_cases, const uint8_t *seqs, const uint32_t *offs, const uint32_t *cand,
                        const uint32_t *coffs, int mode, uint8_t *out, hipStream_t st);
// lane_first / lane_n / lane_case: which cases the block of case c hands to the one-candidate-per-lane kernel (k_diag_lv)
void launch_diag_lv(const IndexView &ix, uint32_t n, const uint32_t *pos, const uint32_t *kdiff, const uint8_t *seqs,
                    const uint32_t *offs, const uint32_t *lane_first, const uint32_t *lane_n, const uint32_t *lane_case,
                    int32_t *out, uint16_t *cig, void *lvtab, int lds_tab, hipStream_t st);
bool lv_lanes_fit(uint32_t L, uint32_t k);          // within the lane kernel's limits (LLV_K, LLV_TW)

// ---- FASTQ text in, SAM text out (salt_text.hip) ----
struct FqRec { uint32_t name_off, name_len, seq_off, len, qual_off; };        // one 4-line record: offsets into the raw block
// per record, between k_sam_len and k_sam_write: the formatted head (flag ... the tab in front of SEQ) and tail (the tags) and their lengths
static const uint32_t SAM_HEAD_CAP = 96, SAM_TAIL_CAP = 224, SAM_SLOT = SAM_HEAD_CAP + SAM_TAIL_CAP;
struct SamSeg { uint16_t head_len, tail_len; uint8_t what, strand, over, pad; };      // what: 0 record, 1 empty line, 2 record without tail; over: head or tail outgrew the slot
struct SamDev {                                                               // what the SAM kernels read (by value)
    const uint8_t *raw; const FqRec *rec; const uint8_t *seqs; const uint32_t *offs; const salt_result_t *res;
    const int64_t *c_off; const uint32_t *c_name_off; const char *c_names; int32_t n_contigs;      // contigs (bntann1_t: offset, name)
    const uint32_t *text, *ref;                                                // 2-bit genome, mixRef
    int32_t xa_cigar, nm_md; const char *rg; int32_t rg_len;
    int32_t pe; uint32_t min_tlen, max_tlen;                                   // pe: records 2p, 2p + 1 are the mates of pair p (alnpe_sam)
    char *slot; SamSeg *seg;                                                   // [n] x SAM_SLOT bytes, [n]: written by k_sam_len, read by k_sam_write
    const uint32_t *tb; PackGeom pg;                                           // k_pack's 2-bit records of the reads (MD / NM / XV by words), or null
};
hipError_t text_warm();                                     // forces the load of the text kernels' code object
size_t text_scan_bytes(uint64_t max_items);
hipError_t launch_fq_count(const uint8_t *raw, uint64_t n, uint32_t *tile_cnt, void *tmp, size_t tmp_bytes, hipStream_t st);
hipError_t launch_fq_lines(const uint8_t *raw, uint64_t n, const uint32_t *tile_off, uint32_t *line_start, hipStream_t st);
hipError_t launch_fq_ctl_init(uint32_t *ctl, hipStream_t st);                       // ctl = { 0, 0, 0xFFFFFFFF, 0 }
hipError_t launch_fq_parse(const uint8_t *raw, const uint32_t *line_start, uint32_t n_rec, FqRec *rec, uint32_t *offs, uint32_t *ctl,
                           void *tmp, size_t tmp_bytes, hipStream_t st);
// one file of a pair: the records of the block at raw + base become rec[2 i + which] (offsets relative to raw), their lengths len[2 i + which];
// the caller initialises ctl ({ 0, 0, 0xFFFFFFFF, 0 }) and scans len afterwards (launch_text_scan)
hipError_t launch_fq_parse_mate(const uint8_t *raw, uint32_t base, const uint32_t *line_start, uint32_t n_rec, uint32_t which, FqRec *rec, uint32_t *len,
                                uint32_t *ctl, hipStream_t st);
hipError_t launch_text_scan(uint32_t *v, uint32_t n_plus_1, void *tmp, size_t tmp_bytes, hipStream_t st);       // exclusive scan in place
hipError_t launch_fq_codes(const uint8_t *raw, const FqRec *rec, const uint32_t *offs, uint32_t n_rec, uint8_t *seqs, hipStream_t st);
hipError_t launch_sam_len(const SamDev &d, uint32_t n, uint32_t *off, unsigned long long *total64, void *tmp, size_t tmp_bytes, hipStream_t st);   // *total64: all bytes, 64-bit
hipError_t launch_sam_write(const SamDev &d, uint32_t n, const uint32_t *off, char *out, hipStream_t st);
// the same block as BAM records (salt --bam): same slots, same scan; *err != 0: a read name longer than 254 bytes
hipError_t launch_bam_len(const SamDev &d, uint32_t n, uint32_t *off, unsigned long long *total64, uint32_t *err, void *tmp, size_t tmp_bytes, hipStream_t st);
hipError_t launch_bam_write(const SamDev &d, uint32_t n, const uint32_t *off, char *out, hipStream_t st);
// records and lengths alone, for the caller that puts k_fq_trim between them and the scan (ctl initialised and offs[n_rec] zeroed by the caller)
hipError_t launch_fq_parse_recs(const uint8_t *raw, const uint32_t *line_start, uint32_t n_rec, FqRec *rec, uint32_t *len, uint32_t *ctl, hipStream_t st);
// trimming (salt_trim.hip): behind k_fq_parse, in front of the scan of len.  Rewrites seq_off, qual_off and len of rec[i] and len[i],
// leaves the longest trimmed read in ctl[3], adds to counts[16]; spans (or null): beg, end of every record.  raw[0, n_raw) is what the offsets may reach.
hipError_t launch_fq_trim(const uint8_t *raw, uint64_t n_raw, FqRec *rec, uint32_t *len, uint32_t n_rec, int pe, uint32_t mate, const TrimRule &rule,
                          uint32_t *ctl, unsigned long long *counts, uint32_t *spans, hipStream_t st);
// the same for the interleaved mates of n_pairs pairs with the pair rule (step 2p) on: k_fq_trim_pair, a wave a pair; adds to pair_counts[8] too;
// spans (or null): b1, e1, b2, e2 of every pair
hipError_t launch_fq_trim_pair(const uint8_t *raw, uint64_t n_raw, FqRec *rec, uint32_t *len, uint32_t n_pairs, const TrimRule &rule, const TrimPairRule &pair,
                               uint32_t *ctl, unsigned long long *counts, unsigned long long *pair_counts, uint32_t *spans, hipStream_t st);
static const uint32_t FQ_TILE = 1024;                                          // bytes per newline-count tile (k_fq_count)

// ---- polish over SAM text (salt_polish.hip) ----
// The text state of a polish handle: its device and page-locked buffers (grown when a block needs more) and the sorted contig table.
// polish_text_run: record lines in, polished record lines out (salt_gpu_polish_text); err: the message of a non-zero return.
struct PolishText;
PolishText *polish_text_new();
void polish_text_free(PolishText *t);
const uint64_t *polish_text_stats(const PolishText *t);        // the eight words of salt_gpu_polish_text_stats
int polish_text_set_contigs(PolishText *t, int32_t n, const int64_t *offsets, const char *const *names, std::string &err);
int polish_text_run(PolishText *t, const uint8_t *d_pac, uint64_t l_pac, void *d_tabs, uint32_t n_blocks, int paired, int use_sw, const char *sam, uint64_t n_bytes,
                    const char **out, uint64_t *out_bytes, uint32_t *n_records, int *stopped, std::string &err);
// The fused route (salt_gpu_ws_set_polish): the polished records of the block a text call of the aligner has just aligned, from its result
// rows and its FASTQ text, all device pointers of the caller's; every kernel goes on `st`.  The contig table is the index's own, in its own
// order.  polish_rows_len: everything up to the records' lengths, *total = the bytes they take; polish_rows_write: the records into d_out
// (the caller's, at least *total bytes), enqueued only.  Statuses become the errors of polish_text_run.
struct PolishRows {
    const uint8_t *raw; const FqRec *fq; const uint8_t *codes; const uint32_t *offs; const salt_result_t *res; uint32_t n_rec, max_len;
    const int64_t *c_off; const uint32_t *c_name_off; const char *c_names; int32_t n_contigs;
    const uint8_t *pac; uint64_t l_pac; void *tabs; uint32_t n_blocks; int paired, use_sw; hipStream_t st;
};
int polish_rows_len(PolishText *t, const PolishRows &in, uint64_t *total, std::string &err);
int polish_rows_write(PolishText *t, char *d_out, hipStream_t st, std::string &err);

// ---- BGZF output (salt_bgzf.hip) ----
// text[0 .. n) (readable up to the next multiple of 4) -> out: ceil(n / BGZF_CUT_BYTES) BGZF blocks, contiguous and in order, bgzf_bound(n) bytes at
// most; offs[b] = where block b starts, offs[n_blocks] = all bytes.  slots: n_blocks x BGZF_SLOT_BYTES, sizes: n_blocks words, offs: n_blocks + 1.
static const uint32_t BGZF_CUT_BYTES = 32640, BGZF_SLOT_BYTES = 32768;
inline uint64_t bgzf_blocks(uint64_t n) { return (n + BGZF_CUT_BYTES - 1) / BGZF_CUT_BYTES; }
inline uint64_t bgzf_bound(uint64_t n) { return n + 31 * bgzf_blocks(n); }       // a stored block: 18 + 5 + text + 8
hipError_t launch_bgzf_deflate(const uint8_t *text, uint64_t n, uint32_t *slots, uint32_t *sizes, unsigned long long *offs, uint8_t *out, hipStream_t st);

// ---- BGZF input (salt_inflate.hip) ----
// members[c_off[b] .. c_off[b + 1]) -> text[u_off[b] .. u_off[b + 1]) for every b < n_blocks, one workgroup per member; status[b] = 0 or the
// reason member b is bad (salt_inflate_block.h: nothing of a bad member's text is written).  The offsets are device arrays of n_blocks + 1.
hipError_t launch_bgzf_inflate(const uint8_t *members, const unsigned long long *c_off, const unsigned long long *u_off, uint32_t n_blocks,
                               uint8_t *text, uint32_t *status, hipStream_t st);

// ---- allele counts at the SNP sites (salt_snp.hip) ----
// One record per 64 genome positions: bit b set = position 64 w + b is a site (its mixRef mask lists two or more bases; nothing at or beyond
// ref_len is one), rank = sites in front of the window.  16 bytes, so that a lookup is one request.
struct SnpWin { unsigned long long bits; uint32_t rank, pad; };
static_assert(sizeof(SnpWin) == 16, "one request per window");
struct SnpCount {                                                              // what k_snp_count reads (by value)
    const salt_result_t *res; const uint8_t *seqs; const uint32_t *offs; uint32_t n_rec;      // the batch: rows, codes as sequenced, offsets
    const SnpWin *tab; uint64_t n_win; uint32_t *counts;                       // the index's site table and counts[n_sites][4] (A C G T)
    uint32_t min_mapq; int32_t pe;                                             // pe: rows of a paired-end batch (reverse iff strand == 1, soft clips)
    uint32_t delta;                                                            // 1; 0xFFFFFFFF takes a batch's adds back
};
size_t snp_scan_bytes(uint64_t n_win);
hipError_t launch_snp_table(const uint32_t *ref, uint32_t ref_len, uint64_t n_win, SnpWin *tab, uint32_t *cnt, void *tmp, size_t tmp_bytes, hipStream_t st);
hipError_t launch_snp_pos(const SnpWin *tab, uint64_t n_win, uint32_t *pos, hipStream_t st);
hipError_t launch_snp_count(const SnpCount &c, hipStream_t st);

// ---- coverage (salt_depth.hip) ----
struct DepthMark {                                                             // what k_depth_mark reads (by value)
    const salt_result_t *res; uint32_t n_rec;                                  // the batch's rows
    uint32_t *diff; uint32_t ref_len;                                          // the index's difference array, ref_len + 1 words
    uint32_t min_mapq;
    uint32_t delta;                                                            // 1; 0xFFFFFFFF takes a batch's marks back
};
hipError_t launch_depth_mark(const DepthMark &c, hipStream_t st);
hipError_t launch_depth_add(uint32_t *diff, const uint32_t *in, uint64_t n, hipStream_t st);      // diff[i] += in[i]
// The text of a difference array, piece by piece (salt_gpu_index_depth_text_begin / _next): its device and page-locked buffers and where it
// stands.  Both return SALT_OK or an error code with the message in err.  h_c_off: the contigs' offsets as set_contigs got them.
struct DepthText;
DepthText *depth_text_new();
void depth_text_free(DepthText *t);
int depth_text_begin(DepthText *t, const uint32_t *d_diff, uint32_t ref_len, const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names,
                     const std::vector<int64_t> &h_c_off, uint32_t max_name, uint32_t window, uint32_t tile_positions, int bgzf, std::string &err);
int depth_text_next(DepthText *t, const char **data, uint64_t *n_bytes, std::string &err);

// ---- the error profile (salt_errprof.hip) ----
static constexpr uint32_t SALT_EP_CHUNK = 1024;                                // reads (of one mate) a workgroup of k_errprof owns, a lane each
struct ErrProf {                                                               // what k_errprof reads (by value)
    const salt_result_t *res; const uint8_t *seqs; const uint32_t *offs; uint32_t n_rec;      // the batch: rows, codes as sequenced, offsets
    // the quality bytes (Phred + 33, FASTQ order): null = none (q 94); rec null: read i's lie at quals + offs[i] (parallel to seqs), else at
    // quals + rec[i].qual_off (the text path's raw block); q_bytes: the bytes behind quals, a read whose range leaves them counts in q 94
    const uint8_t *quals; const FqRec *rec; uint64_t q_bytes;
    const uint32_t *ref; uint32_t ref_len;                                     // the 4-bit mixRef
    unsigned long long *cells;                                                 // E[2][512][95][4][4], then R[2][8]
    uint32_t min_mapq; int32_t pe;                                             // pe: rows of a paired-end batch (reverse iff strand == 1, soft clips, mate = i & 1)
    unsigned long long delta;                                                  // 1; 2^64 - 1 takes a batch's adds back
};
hipError_t launch_errprof(const ErrProf &c, hipStream_t st);

// ---- genotypes at the SNP sites (salt_gt.hip) ----
struct GtAdd {                                                                 // what k_gt_add reads (by value)
    const salt_result_t *res; const uint8_t *seqs; const uint32_t *offs; uint32_t n_rec;      // the batch: rows, codes as sequenced, offsets
    const uint8_t *quals; const FqRec *rec; uint64_t q_bytes;                  // the quality bytes, as ErrProf has them; a read without them counts at SALT_GT_Q_NONE
    const SnpWin *tab; uint64_t n_win;                                         // the index's site table (the SNP counts' own)
    unsigned long long *sums; uint64_t n_sites;                                // salt_gt_site_t[n_sites] as words: [site][A C G T][n sm sx sh]
    uint32_t min_mapq; int32_t pe;                                             // pe: rows of a paired-end batch (reverse iff strand == 1, soft clips)
    unsigned long long delta;                                                  // 1; 2^64 - 1 negates the addends: a batch's adds are taken back
};
hipError_t launch_gt_add(const GtAdd &c, hipStream_t st);
hipError_t launch_gt_sum(unsigned long long *sums, const unsigned long long *in, uint64_t n_words, hipStream_t st);      // sums[i] += in[i]
// The records of the sums, piece by piece (salt_gpu_index_gt_text_begin / _next): the device and page-locked buffers and where the text
// stands.  Both return SALT_OK or an error code with the message in err.
struct GtText;
GtText *gt_text_new();
void gt_text_free(GtText *t);
int gt_text_begin(GtText *t, const unsigned long long *d_sums, const SnpWin *d_tab, uint64_t n_win, uint32_t n_sites, const uint32_t *d_ref, const uint32_t *d_text,
                  uint32_t ref_len, uint32_t text_len, const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names, int32_t n_contigs, uint32_t max_name,
                  uint32_t tile_sites, int bgzf, std::string &err);
int gt_text_next(GtText *t, const char **data, uint64_t *n_bytes, std::string &err);

// ---- SNP candidates off the index's sites (salt_discover.hip) ----
struct DiscAdd {                                                               // what k_disc_add reads (by value)
    const salt_result_t *res; const uint8_t *seqs; const uint32_t *offs; uint32_t n_rec;      // the batch: rows, codes as sequenced, offsets
    const uint8_t *quals; const FqRec *rec; uint64_t q_bytes;                  // the quality bytes, as GtAdd has them; a read without them passes the filter
    const uint32_t *ref; uint32_t ref_len;                                     // the 4-bit mixRef, (ref_len + 7) / 8 words
    unsigned long long *alt; uint32_t *diff;                                   // uint64[ref_len] of three 21-bit fields; this tally's own difference array, ref_len + 1 words
    uint32_t min_mapq, min_baseq; int32_t pe;                                  // pe: rows of a paired-end batch (reverse iff strand == 1, soft clips)
    unsigned long long delta;                                                  // 1; 2^64 - 1 negates the addends of both arrays: a batch's adds are taken back
};
hipError_t launch_disc_add(const DiscAdd &c, hipStream_t st);
// The candidate lines of the two arrays, piece by piece (salt_gpu_index_disc_text_begin / _next): the device and page-locked buffers and
// where the text stands.  Both return SALT_OK or an error code with the message in err.
struct DiscText;
DiscText *disc_text_new();
void disc_text_free(DiscText *t);
int disc_text_begin(DiscText *t, const unsigned long long *d_alt, const uint32_t *d_diff, const uint32_t *d_ref, const uint32_t *d_text, uint32_t ref_len, uint32_t text_len,
                    const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names, int32_t n_contigs, uint32_t max_name,
                    uint32_t min_alt, uint32_t min_pct, int all_sites, uint32_t tile_positions, int bgzf, std::string &err);
int disc_text_next(DiscText *t, const char **data, uint64_t *n_bytes, std::string &err);
int disc_text_seen(DiscText *t, uint8_t *seen, uint64_t cap, std::string &err);      // seen[c] = contig c has a line; the text must be complete

// ---- the run's summary (salt_stats.hip) ----
static constexpr uint32_t SALT_STATS_CHUNK = 2048;                             // records a workgroup of k_stats_add owns
struct StatsAdd {                                                              // what k_stats_add reads (by value)
    const salt_result_t *res; const uint8_t *seqs; const uint32_t *offs; uint32_t n_rec;      // the batch: rows, codes as sequenced, offsets
    const int64_t *c_off; int32_t n_contigs; uint32_t ref_len;                 // set_contigs' offsets (n_contigs >= 1)
    unsigned long long *cells, *ct;                                            // SALT_STATS_CELLS cells; CT[n_contigs][8]
    uint32_t min_mapq, min_tlen, max_tlen; int32_t pe;                         // pe: rows of a paired-end batch (mate = i & 1, the mate's row is i ^ 1), with the call's -a / -b window
    unsigned long long delta;                                                  // 1; 2^64 - 1 takes a batch's adds back
};
hipError_t launch_stats_add(const StatsAdd &c, hipStream_t st);

// ---- indel candidates (salt_indel.hip) ----
struct IndelSlot { unsigned long long key, val; };                             // key 0: empty; val: forward observations low, reverse high
struct IndelAdd {                                                              // what k_indel_add reads (by value)
    const salt_result_t *res; const uint8_t *seqs; const uint32_t *offs; uint32_t n_rec;      // the batch: rows, codes as sequenced, offsets
    const uint32_t *text; uint32_t text_len, ref_len;                          // the 2-bit genome, 16 bases a word, and the positions it holds
    const int64_t *c_off; int32_t n_contigs;                                   // set_contigs' offsets (n_contigs >= 1)
    uint32_t *diff; IndelSlot *tab; uint32_t log2_slots; unsigned long long *stat;      // this tally's difference array, ref_len + 1 words; 2^log2_slots slots; stat[4]
    uint32_t min_mapq; int32_t pe;                                             // pe: rows of a paired-end batch (reverse iff strand == 1, soft clips)
    unsigned long long delta;                                                  // 1; 2^64 - 1 takes a batch's adds back
};
hipError_t launch_indel_add(const IndelAdd &c, hipStream_t st);
// n hand-given (key, value) pairs through the insert routine of k_indel_add
hipError_t launch_indel_put(const unsigned long long *pairs, uint64_t n, IndelSlot *tab, uint32_t log2_slots, unsigned long long *stat, hipStream_t st);
// The slots with a non-zero value, sorted by key, into buffers the text state owns (salt_gpu_index_indel_fetch reads them from there), and
// the records of the called ones piece by piece.  All return SALT_OK or an error code with the message in err.
struct IndelText;
IndelText *indel_text_new();
void indel_text_free(IndelText *t);
int indel_sorted(IndelText *t, const IndelSlot *d_tab, uint32_t log2_slots, uint64_t *n, const unsigned long long **d_keys, const unsigned long long **d_vals, std::string &err);
int indel_text_begin(IndelText *t, const IndelSlot *d_tab, uint32_t log2_slots, const uint32_t *d_diff, const uint32_t *d_text, uint32_t ref_len, uint32_t text_len,
                     const int64_t *d_c_off, const uint32_t *d_c_name_off, const char *d_c_names, int32_t n_contigs, uint32_t max_name,
                     uint32_t min_alt, uint32_t min_pct, uint32_t tile_positions, int bgzf, std::string &err);
int indel_text_next(IndelText *t, const char **data, uint64_t *n_bytes, std::string &err);

// attach-time re-packing + expansion kernels (salt_index.hip)
void launch_pack_c_occ(const uint32_t *bwt, uint64_t bwt_words, uint32_t seq_len, uint64_t n_blocks, COcc *out, uint32_t *err, hipStream_t st);
void launch_pack_r_occ(const uint32_t *code, uint64_t code_words, const uint32_t *minor, uint64_t minor_words, const uint32_t *major, uint64_t major_words,
                       uint32_t text_len, uint64_t n_blocks, ROcc *out, uint32_t *err, hipStream_t st);
void launch_build_c_ctx(const IndexView &ix, uint32_t ctx_k, uint4 *out, hipStream_t st);
void launch_build_r_ctx(const IndexView &ix, uint32_t ctx_k, uint4 *out, hipStream_t st);
void launch_build_c_sa(const IndexView &ix, const uint32_t *sa_sampled, uint32_t sa_intv, uint32_t *out, hipStream_t st);
void launch_build_r_pos(const IndexView &ix, const uint32_t *r_sa, uint32_t *out, hipStream_t st);
void launch_build_text(const IndexView &ix, uint32_t *out, hipStream_t st);
void launch_build_wlkt(const IndexView &ix, uint32_t len, uint4 *out, hipStream_t st);
void launch_diag_occ(const IndexView &ix, int mode, uint32_t n, const uint32_t *q, uint32_t *out, hipStream_t st);      // q: n x (x, y, c); out: n x 12 words

} // namespace salt
