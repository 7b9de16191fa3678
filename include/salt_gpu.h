/* include/salt_gpu.h -- C ABI of the MI355X (gfx950) implementation of salt's single-end per-read
 * alignment path.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * What it replaces in the reference (weiquan/salt, paths under Align_src/):
 *
 *   salt_gpu_index_attach      one-time upload after alnse_index_reload()        indexio.c:23-49
 *   salt_gpu_index_detach      alnse_index_destroy() for the device copy         indexio.c:50-60
 *   salt_gpu_align_se          the per-batch call that stands where the pthread  alnse.c:1419-1429
 *                              fan-out over alnse_core1() is: for every read      alnse.c:1316-1352
 *                              alnse_overlap_alt + query_gen_cigar                alnse.c:1045-1104
 *                                                                                 query.c:282-333
 *   salt_gpu_align_se_resident same work on buffers that already live in HBM (what bench.py times)
 *
 * The reference has no FFI of its own (pure C, one process); INTEGRATION.md shows the ~40-line
 * patch to alnse.c that binds these entry points in place of alnse_core1().
 *
 * Error model: the reference reports nothing upward (any failure is exit(1)); here every entry
 * point returns 0 on success or a negative SALT_E_* code, and salt_gpu_last_error() gives text.
 */
#ifndef SALT_GPU_H
#define SALT_GPU_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SALT_OK              0
#define SALT_E_INVAL        -1   /* bad argument / unsupported option value */
#define SALT_E_HIP          -2   /* a HIP runtime call failed */
#define SALT_E_NOMEM        -3
#define SALT_E_INDEX        -4   /* malformed index arrays */
#define SALT_E_CAPACITY     -5   /* batch larger than the workspace was created for */
#define SALT_E_DATA         -6   /* damaged compressed input */

#define SALT_MAX_READ_LEN   512  /* bases per read handled by the kernels */
#define SALT_MAX_HITS       5    /* aln.h:133 */
#define SALT_MAX_LOCATE     1024 /* located rows per strand kept in LDS (reference default -m 1000); -m up to 262144 is accepted, larger lists go to global memory */
#define SALT_MAX_SEED_SLOTS 512  /* seeds per strand, ceil((L-k+1)/overlap): any stride down to -r 1 on reads of SALT_MAX_READ_LEN bases */
#define SALT_MAX_CIGAR_OPS  64

/* Host-side view of index_t (indexio.h:26-33): the arrays exactly as the index files hold them. */
typedef struct {
    /* <P>.C.bwt / <P>.C.sa : bwt_t (bwt.h:40-55, bwtio.c:30-71) */
    uint32_t c_primary, c_L2[5], c_seq_len, c_bwt_size;
    const uint32_t *c_bwt;
    uint32_t c_sa_intv, c_n_sa;
    const uint32_t *c_sa;                       /* c_sa[0] == 0xFFFFFFFF */
    /* <P>.C.lkt : lookupTable_t (lookup.h:21-25) */
    uint32_t lkt_len, lkt_n;
    const uint32_t *lkt;
    /* <P>.R.backward.{bwt,occ,sa} : rbwt_t (rbwt.h:60-80) */
    uint32_t r_text_len, r_inv_sa0, r_cum[6], r_bwt_words;
    const uint32_t *r_bwt;
    uint32_t r_occ_words;   const uint32_t *r_occ;
    uint32_t r_major_words; const uint32_t *r_major;
    uint32_t r_n_sa;        const uint32_t *r_sa;
    /* <P>.ref : mixRef_t (metaref.h) */
    uint32_t ref_len;
    const uint32_t *ref;
    /* <P>.R.seedLen (aln.c:215-224); 0 = unknown.  Bounds the width of the device-side k-mer tables. */
    int32_t  l_seed;
} salt_host_index_t;

/* The fields of aln_opt_t (aln.h:63-89) the single-end path reads. */
typedef struct {
    int32_t  l_seed;         /* <P>.R.seedLen */
    int32_t  l_overlap;      /* -r (defaults to l_seed) */
    uint32_t max_seed;       /* -s, 50 */
    uint32_t max_locate;     /* -m, 1000 */
    int32_t  max_hits;       /* 5 */
    int32_t  seed_only_ref;  /* -v */
    int32_t  collect_counters; /* accumulate the logical-access counters below */
    int32_t  reserved;
} salt_aln_opt_t;

/* hit_t (query.h:28-33) */
typedef struct {
    uint32_t pos;
    uint8_t  n_diff, is_gap;
    uint16_t strand;
} salt_hit_t;

/* The result fields alnse_core1 leaves in query_t (query.h:37-63).  CIGARs are binary:
 * (len << 4) | op with op 0=M 1=I 2=D, in the order the text CIGAR lists them. */
typedef struct {
    uint32_t pos;                               /* 0xFFFFFFFF = unmapped */
    uint8_t  strand, n_diff, is_gap, mapq;      /* strand 3 / n_diff 255 / is_gap 255 when unset */
    int32_t  b0, b1;
    uint16_t seq_start, seq_end;
    uint8_t  n_hits[2];                         /* alternative hits kept per strand (<= 5 in all) */
    uint8_t  n_cigar;                           /* ops in cigar[] (0 when unmapped) */
    uint8_t  skipped;                           /* 1: > 200 N, read left untouched (alnse.c:1328) */
    salt_hit_t hits[2][SALT_MAX_HITS];
    uint8_t  hit_n_cigar[SALT_MAX_HITS];        /* ops of hit_cigar[h]; h counts strand-0 hits, then */
    uint8_t  pad[3];                            /* strand-1 hits; 0 for gap-free hits ("<L>M")        */
    uint16_t cigar[SALT_MAX_CIGAR_OPS];
    uint16_t hit_cigar[SALT_MAX_HITS][SALT_MAX_CIGAR_OPS];
} salt_result_t;                                /* 880 bytes */

/* access counters summed over a batch (only with collect_counters): SA / verify / LV / loci entries count what the align kernels do
 * per located row and candidate; LKT / OCC_C / OCC_R count k_seed's DEVICE accesses (W-mer gathers, Occ blocks fetched) */
enum { SALT_CTR_LKT, SALT_CTR_OCC_C, SALT_CTR_OCC_R, SALT_CTR_SA_C, SALT_CTR_SA_R, SALT_CTR_VERIFY,
       SALT_CTR_VERIFY_WORDS, SALT_CTR_LV, SALT_CTR_READS, SALT_CTR_BASES, SALT_CTR_LOCI,
       /* diagnostics: shader-clock cycles k_heavy waves spent per phase (only with collect_counters) */
       SALT_CTR_T_LOAD, SALT_CTR_T_GATHER, SALT_CTR_T_LOCATE, SALT_CTR_T_SORT, SALT_CTR_T_DEDUP, SALT_CTR_T_VERIFY,
       SALT_CTR_T_SCAN, SALT_CTR_T_GAP, SALT_CTR_T_TAIL, SALT_CTR_HEAVY_READS, SALT_CTR_X0, SALT_CTR_X1, SALT_CTR_X2, SALT_CTR_X3,
       SALT_CTR_LT_SEEDS, SALT_CTR_LT_LOCATE, SALT_CTR_LT_SORT, SALT_CTR_LT_VERIFY, SALT_CTR_LT_OUT, SALT_CTR_LT_SAMPLES,   /* k_light: s_memtime ticks of every 128th read */
       SALT_CTR_MAX_HEAVY, SALT_CTR_MAX_GAPFIN,   /* slowest read of k_heavy / k_gapfin: (s_memrealtime ticks << 32) | read index */
       /* DEVICE-layout accesses (what the kernels' own structures move; bench.py's roofline): k_seed -- 16-byte W-mer table gathers,
        * 32-byte C / 64-byte R Occ blocks fetched, suffix-array loads and 8-byte text loads of the one-row resolve; k_light / k_heavy --
        * 4-byte suffix-array / R-position loads, 16-byte verify lane-loads, result bytes stored */
       SALT_CTR_D_WLKT, SALT_CTR_D_COCC_SEED, SALT_CTR_D_ROCC_SEED, SALT_CTR_D_SA_SEED, SALT_CTR_D_TEXT_SEED,
       SALT_CTR_D_SA_LIGHT, SALT_CTR_D_VERIFY_LIGHT, SALT_CTR_D_OUT_LIGHT, SALT_CTR_D_SA_HEAVY, SALT_CTR_D_VERIFY_HEAVY, SALT_CTR_D_OUT_HEAVY,
       /* context table: 16-byte records read in place of 4-byte suffix-array loads, and the located rows it ruled out (windows never read) */
       SALT_CTR_D_CTX_ROWS, SALT_CTR_D_CTX_REJECTED,
       SALT_CTR_N };

typedef struct salt_gpu_index salt_gpu_index_t;
typedef struct salt_gpu_ws    salt_gpu_ws_t;

/* ---- device index ------------------------------------------------------------------------- */
/* Re-packs the host arrays into the device layout (DESIGN.md "HBM layout") on `device`. */
int  salt_gpu_index_attach(const salt_host_index_t *host, int device, salt_gpu_index_t **out);
void salt_gpu_index_detach(salt_gpu_index_t *ix);
/* The packed device image is one contiguous, position-independent allocation so that a multi-GPU
 * driver can broadcast it (RCCL) instead of re-packing on every rank. */
int  salt_gpu_index_image(const salt_gpu_index_t *ix, void **dev_ptr, uint64_t *bytes);
int  salt_gpu_index_attach_image(void *dev_ptr, uint64_t bytes, int device, salt_gpu_index_t **out);
/* The image ends with the W-mer table (16 B x 4^W: 64 GiB at W = 16, the default on a free MI355X), a pure function of what
 * precedes it.  The part before it is the COMPACT image -- what a multi-GPU driver needs to move: broadcast
 * [dev_ptr, dev_ptr + bytes) of salt_gpu_index_image_compact, then salt_gpu_index_attach_compact on each receiver
 * allocates the full image, copies the compact part in and tabulates the W-mer table there (it owns the result;
 * the broadcast buffer may be freed afterwards). */
int  salt_gpu_index_image_compact(const salt_gpu_index_t *ix, void **dev_ptr, uint64_t *bytes);
int  salt_gpu_index_attach_compact(const void *dev_ptr, uint64_t bytes, int device, salt_gpu_index_t **out);
/* Replicates the image of `src` (attached on devices[0]) onto devices[1..n): one RCCL broadcast of the compact part
 * over xGMI inside this process (ncclCommInitAll + grouped ncclBroadcast); each device then builds its W-mer table.
 * out[0] = src; out[i] owns its copy and is released with salt_gpu_index_detach. */
int  salt_gpu_index_replicate(salt_gpu_index_t *src, const int *devices, int n, salt_gpu_index_t **out);
/* device-to-device copy into a caller-owned buffer (e.g. a broadcast buffer): the full image when dst_bytes >= its
 * size, else its compact part (dst_bytes >= the compact size) */
int  salt_gpu_index_image_copy(const salt_gpu_index_t *ix, void *dst_dev_ptr, uint64_t dst_bytes);

/* ---- per-batch work ----------------------------------------------------------------------- */
int  salt_gpu_ws_create(salt_gpu_index_t *ix, uint32_t max_reads, uint64_t max_bases, salt_gpu_ws_t **out);
void salt_gpu_ws_destroy(salt_gpu_ws_t *ws);

/* Host buffers in, host results out; synchronous.  seqs: base codes 0..4 (A C G T N, query.c:177-183),
 * read i at seqs[offs[i] .. offs[i+1]).  Fills results[0..n_reads). */
int  salt_gpu_align_se(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, uint32_t n_reads,
                       const uint8_t *seqs, const uint32_t *offs, salt_result_t *results);

/* Paired end: the per-batch call that stands where alnpe_core1 runs (Align_src/alnpe.c:482-528, 596-606).
 * Mates are interleaved as query_read_multiPairedSeqs lays them out (query.c:252-268): pair i = reads 2i, 2i+1 of
 * seqs/offs; results[2i], results[2i+1].  Per mate: alnse_overlap (alnse.c:985-1044); per pair: pairing2 /
 * pairing_singleton with Smith-Waterman mate rescue (alnpe.c:94-480, ssw.c); CIGARs by query_gen_cigar or from the
 * rescue.  A rescued mate has seq_start / seq_end set (soft clips), b0 / b1 = SW scores.  `pac`: the 2-bit genome
 * (<P>.C.pac bytes, needed by the singleton rescue), l_pac bases. */
typedef struct { uint32_t min_tlen, max_tlen; } salt_pe_opt_t;      /* -a 250, -b 550 (aln.c:43-44) */
int  salt_gpu_index_set_pac(salt_gpu_index_t *ix, const uint8_t *pac, uint64_t l_pac);
/* The context records of the R rows (16 B per row of the R index, outside the image): built at attach when the C rows have theirs and
 * the device has the room, else by salt_gpu_index_set_pac once it has.  *dev_ptr is NULL and *bytes 0 when the index goes without. */
int  salt_gpu_index_r_ctx(const salt_gpu_index_t *ix, void **dev_ptr, uint64_t *bytes);
/* The epoch the workspace's NEXT alignment call runs at (1 .. 2^24 - 1; the R seed rows of a call carry it, salt_device.h). */
int  salt_gpu_ws_epoch(const salt_gpu_ws_t *ws, uint32_t *next_epoch);
int  salt_gpu_align_pe(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, const salt_pe_opt_t *pe, uint32_t n_pairs,
                       const uint8_t *seqs, const uint32_t *offs, salt_result_t *results);
/* Same on device-resident buffers (2 * n_pairs reads); only enqueues on `hip_stream`; not to be stream-captured and replayed (see salt_gpu_align_se_resident). */
int  salt_gpu_align_pe_resident(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, const salt_pe_opt_t *pe, uint32_t n_pairs,
                                uint32_t max_read_len, const void *d_seqs, const void *d_offs, void *d_results, void *hip_stream);
/* Mate rescues of the LAST paired batch that could not be finished as the reference would (their banded traceback needs
 * a band wider than the build's row buffers: possible only for reads longer than ~270 bases with a gap of that size).
 * salt_gpu_align_pe fails with SALT_E_CAPACITY when this is non-zero; callers of the resident entry check it themselves
 * (it synchronises the device). */
int  salt_gpu_ws_pe_overflow(salt_gpu_ws_t *ws, uint32_t *n);
/* Counters of the LAST paired batch (diagnostics): out[0] = Smith-Waterman rescue requests, out[2] = CIGAR items queued by
 * k_pe_final, out[4] = the overflow count above; the rest is internal. */
int  salt_gpu_ws_pe_counts(salt_gpu_ws_t *ws, uint32_t out[8]);

/* ---- allele counts at the index's SNP sites (`salt --snp-counts`) --------------------------------------------------------
 * A site is a genome position g (0-based in the concatenated coordinate of salt_result_t.pos, 0 <= g < ref_len) whose mixRef mask
 * (ref[g >> 3] >> 4 * (g & 7)) & 15 lists two or more bases; sites are numbered in ascending g.  While counting is on, every entry point that
 * leaves result rows (salt_gpu_align_se / _pe, the resident and the text entry points, under salt_gpu_ws_set_polish too) adds, behind the
 * kernels that finish the rows and on the same stream, what the batch's records show at the sites: a record contributes iff it is mapped
 * (pos != 0xFFFFFFFF), not skipped, and mapq >= min_mapq; its CIGAR is walked as the SAM / BAM writers lay it out (a paired-end row's
 * leading soft clip seq_start, the row's M / I / D ops) from g = pos, s = 0 in SEQ as printed (reverse-complemented iff strand != 0 single
 * end, strand == 1 paired end); every M column where g is a site and SEQ[s] is A, C, G or T adds 1 to counts[site(g)][base].  I and S
 * advance s, D advances g, a read's N counts nowhere, alternative (XA) hits never count.  counts is uint32[n_sites][4] in the order A C G T;
 * the sums do not depend on batch order, stream or workspace.  The table and the counts belong to the device index and are shared by all
 * its workspaces; they lie outside the image (16 bytes per 64 genome positions + 16 per site).  With counting off no kernel is launched,
 * and before the first enable nothing is allocated.
 *   salt_gpu_index_snp_enable  the first enable builds the site table and zeroes the counts (SALT_E_NOMEM names the size when there is no
 *                              room); on = 0 stops counting and keeps both; min_mapq 0 .. 255.  Call with no align call in flight.
 *   salt_gpu_index_snp_sites   *n_sites, and when pos is given (cap >= *n_sites entries) the sites' genome positions, ascending
 *                              (also once salt_gpu_index_gt_enable has built the table)
 *   salt_gpu_index_snp_counts  synchronises the device; counts may be NULL (reset only); cap_words >= 4 * n_sites.  No align call in flight.
 *   salt_gpu_ws_snp_uncount    takes back what the workspace's LAST successful align call added (the call's buffers must be untouched
 *                              since): for a driver that discards a block it has aligned.  Nothing to take back: SALT_OK.
 * SALT_E_INVAL, with a message that says which: counting never enabled on the index, cap / cap_words too small, min_mapq above 255. */
int  salt_gpu_index_snp_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq);
int  salt_gpu_index_snp_sites(salt_gpu_index_t *ix, uint32_t *n_sites, uint32_t *pos, uint64_t cap);
int  salt_gpu_index_snp_counts(salt_gpu_index_t *ix, uint32_t *counts, uint64_t cap_words, int reset);
int  salt_gpu_ws_snp_uncount(salt_gpu_ws_t *ws);

/* ---- coverage: per-base and windowed depth (`salt --depth`) ---------------------------------------------------------------
 * Which records contribute is the rule of the SNP counts: the row is mapped (pos != 0xFFFFFFFF), not skipped, and mapq >= min_mapq; only
 * the primary alignment counts, never an alternative (XA) hit; an unmapped mate printed at its mate's position does not count.
 * The difference array: diff is uint32[ref_len + 1] in the concatenated coordinate of salt_result_t.pos, arithmetic mod 2^32.  The CIGAR is
 * walked as the SAM / BAM writers lay it out (a paired-end row's leading soft clip seq_start advances the read only) from g = pos.  Every
 * M run [g, g + len) is cut to [g, min(g + len, ref_len)); when that is not empty, diff[g] += 1 and diff[end] -= 1.  D advances g and is
 * no coverage (samtools depth's default), I and S advance the read only.  A read across a contig boundary counts at the global positions
 * it covers.
 * Depth: depth[g] = sum of diff[x], x <= g, mod 2^32, for 0 <= g < ref_len: exact while fewer than 2^32 records cover one position.  diff
 * is a sum of integers: it does not depend on batch order, stream, workspace or GPU, and the arrays of several GPUs add word by word.
 * Per-base text (window 0): bedGraph, "contig\tstart\tend\tdepth\n", start and end 0-based, half-open and contig-relative; one line per
 * maximal run of equal depth inside one contig, runs of depth 0 included, ascending in genome order, no header.  The lines of a contig
 * tile it from 0 to its length; a run never crosses a contig end, also when the depth is the same on both sides.  The contigs are those of
 * salt_gpu_index_set_contigs (<P>.C.ann); position ref_len is the last contig's end.
 * Window text (window W >= 1): every contig has the windows [k W, min((k + 1) W, contig_len)); the line is "contig\tstart\tend\tmean\n";
 * with sum the 64-bit sum of depth over the window and len its length, h = (100 sum + len / 2) / len by integer division and the field is
 * h / 100, a dot, h % 100 as two digits.  No floating point anywhere.
 * While depth is on, every entry point that leaves result rows adds its batch behind the kernels that finish the rows, on the same stream
 * (k_depth_mark: about two atomics a read).  The array belongs to the device index and is shared by its workspaces and forks; it lies
 * outside the image (4 bytes a genome position).  With depth off no kernel is launched; before the first enable nothing is allocated, and
 * every other call below fails with SALT_E_INVAL "never enabled".
 *   salt_gpu_index_depth_enable    the first enable allocates and zeroes diff (SALT_E_NOMEM names the size); on = 0 stops and keeps it;
 *                                  min_mapq 0 .. 255 (above: SALT_E_INVAL).  Call with no align call in flight, like the three below.
 *   salt_gpu_index_depth_reset     diff = 0
 *   salt_gpu_index_depth_fetch     out[0 .. n) = diff[first .. first + n); synchronises the device
 *   salt_gpu_index_depth_add       diff[first .. first + n) += in[0 .. n), by a kernel: how the arrays of several GPUs are summed, chunk
 *                                  by chunk, and how any array can be put in front of the text kernels.  A range that leaves
 *                                  [0, ref_len] is SALT_E_INVAL with the range in the message, for both.
 *   salt_gpu_index_depth_text_begin  starts the text of the array as it stands: window 0 = per base; tile_positions = genome positions
 *                                  scanned at a time, 0 = the default (the text does not depend on it); bgzf != 0: whole BGZF blocks
 *                                  instead of text, deflated on the device, without the end-of-file block.  Needs the contig table.
 *                                  An array of window sums that does not fit is SALT_E_NOMEM naming its size.
 *   salt_gpu_index_depth_text_next   the next piece, in genome order: *data points into a buffer the index owns, valid until the next
 *                                  call on the index; *n_bytes == 0: the text is complete.  diff is never written by these two: the
 *                                  text can be made twice with the same bytes, and counting can go on afterwards.
 *   salt_gpu_ws_depth_uncount      takes back what the workspace's LAST successful align call added (delta 2^32 - 1), as
 *                                  salt_gpu_ws_snp_uncount does.  Nothing to take back: SALT_OK. */
typedef struct {
    uint32_t window;            /* 0: per-base runs; W >= 1: mean depth of every window of W positions */
    uint32_t tile_positions;    /* 0: default */
    int32_t  bgzf;              /* the pieces are BGZF blocks */
} salt_depth_text_opt_t;
int  salt_gpu_index_depth_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq);
int  salt_gpu_index_depth_reset(salt_gpu_index_t *ix);
int  salt_gpu_index_depth_fetch(salt_gpu_index_t *ix, uint64_t first, uint64_t n, uint32_t *out);
int  salt_gpu_index_depth_add(salt_gpu_index_t *ix, uint64_t first, uint64_t n, const uint32_t *in);
int  salt_gpu_index_depth_text_begin(salt_gpu_index_t *ix, const salt_depth_text_opt_t *opt);
int  salt_gpu_index_depth_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes);
int  salt_gpu_ws_depth_uncount(salt_gpu_ws_t *ws);

/* ---- the error profile: mismatches by cycle, quality and substitution, SNP sites masked (`salt --error-profile`) ----------
 * Which records contribute is the rule of the SNP counts: the row is mapped (pos != 0xFFFFFFFF), not skipped, and mapq >= min_mapq; only
 * the primary alignment counts, never an alternative (XA) hit.
 * The walk is k_snp_count's: a paired-end row's leading soft clip is seq_start; g = pos, s the index in SEQ as printed (reverse iff
 * strand != 0 single end, strand == 1 paired end); I and S advance s, D advances g; ops beyond SALT_MAX_CIGAR_OPS are ignored.
 * One base event is an M column with g < ref_len and s < L (L the read's length) for which (1) the mixRef mask at g has exactly one bit
 * set -- sites (two or more bits) and N (mask 0) count nowhere -- and (2) the read's code there is 0 .. 3: a read's N counts nowhere.
 * Its coordinates are the sequencer's, not the SAM's:
 *   cycle = rev ? L - 1 - s : s                  0 .. 511
 *   read  = the code as sequenced, seqs[offs[i] + cycle]
 *   ref   = the index of the mask's bit (bit c = base code c), complemented (3 - c) when rev
 *   q     = the FASTQ quality byte at `cycle` minus 33 when the byte is in 33 .. 126; otherwise, and when the call has no qualities, 94 ("none")
 *   mate  = 0 single end and read 2i of a pair, 1 for read 2i + 1
 * Tables, all uint64, owned by the device index and shared by its workspaces and forks, outside the image:
 *   E[2][512][95][4][4]  indexed [mate][cycle][q][ref][read]: SALT_ERRPROF_CELLS cells, 12.45 MB
 *   R[2][8]              per mate: records seen, skipped, unmapped, below min_mapq, counted, counted and reverse, counted with any I, D or
 *                        S op, 0.  Skipped, unmapped and below min_mapq are exclusive and tested in that order; counted is the rest.
 * The sums do not depend on batch order, stream, workspace or GPU, and the cells are 64-bit: nothing wraps silently.  (k_errprof sums
 * per workgroup in 32-bit LDS cells that it flushes behind every tile of 16 cycles; such a cell never passes the workgroup's 1 024 reads.)
 * While the profile is on, every entry point that leaves result rows adds its batch behind the kernels that finish the rows, on the same
 * stream.  The text entry points take the qualities from the raw block on the device; the host-buffer and resident entry points count in
 * q = 94 unless salt_gpu_ws_set_quals was called.  With the profile off no kernel is launched and nothing is copied; before the first
 * enable nothing is allocated.
 *   salt_gpu_index_errprof_enable  the first enable allocates and zeroes the tables (SALT_E_NOMEM names the size); on = 0 stops and keeps
 *                                  them; min_mapq 0 .. 255 (above: SALT_E_INVAL).  Call with no align call in flight, like fetch.
 *   salt_gpu_index_errprof_fetch   synchronises the device; cells (SALT_ERRPROF_CELLS of them) may be NULL (reset only), cap_cells too small
 *                                  is SALT_E_INVAL with the number in the message; rec (may be NULL) gets R; reset != 0 zeroes both
 *                                  afterwards.  Never enabled: SALT_E_INVAL.
 *   salt_gpu_ws_errprof_uncount    takes back what the workspace's LAST successful align call added (the same kernel with delta 2^64 - 1
 *                                  and that call's quality source; the call's buffers must be untouched since).  Nothing to take back: SALT_OK.
 *   salt_gpu_ws_set_quals          quality bytes parallel to seqs, at the same offs, in FASTQ order (Phred + 33), for the NEXT host-buffer
 *                                  or resident align call on this workspace, which consumes them; on_device != 0: a device pointer (a
 *                                  host pointer cannot serve a resident call: SALT_E_INVAL there).  The bytes must stay valid until that
 *                                  call returns (host) or its stream has run and no uncount is wanted any more (device).  NULL: none. */
#define SALT_ERRPROF_Q      95                    /* q 0 .. 93 and "none" */
#define SALT_ERRPROF_CELLS  (2u * SALT_MAX_READ_LEN * SALT_ERRPROF_Q * 16u)
int  salt_gpu_index_errprof_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq);
int  salt_gpu_index_errprof_fetch(salt_gpu_index_t *ix, uint64_t *cells, uint64_t cap_cells, uint64_t rec[16], int reset);
int  salt_gpu_ws_errprof_uncount(salt_gpu_ws_t *ws);
int  salt_gpu_ws_set_quals(salt_gpu_ws_t *ws, const uint8_t *quals, int on_device);

/* ---- genotypes at the index's SNP sites (`salt --genotype`) ---------------------------------------------------------------
 * Sites, their numbering, which records contribute and the CIGAR walk are those of the SNP counts above: a record contributes iff it is
 * mapped (pos != 0xFFFFFFFF), not skipped, and mapq >= min_mapq; only the primary alignment counts, never an alternative (XA) hit; an
 * unmapped mate printed at its mate's position does not count.
 * Events: every M column where g is a site and SEQ[s] is a base b in A C G T is one event (site, b, q).  The quality byte is that of the
 * same sequenced base: it has the index of the code byte, rev ? L - 1 - s : s, in the FASTQ's order; q = byte - 33 when the byte is in
 * 33 .. 126.  In every other case q = SALT_GT_Q_NONE = 20: no qualities on the call, a quality range that leaves the call's quality
 * bytes, a byte outside 33 .. 126, SAM QUAL `*` in the host twin.
 * Penalties: SALT_GT_TABLE[94][3] (salt_gt_table.h) holds uint32 { M, X, H } per q in units of 1 / 4096 Phred; the header states the formula.
 * Sums: salt_gt_site_t, 128 bytes a site: per base A C G T { n, sm, sx, sh }, uint64.  An event adds 1, M[q], X[q], H[q] to its base's four
 * words.  Integer sums: they do not depend on batch order, stream, workspace or GPU, nothing wraps, and the tables of several GPUs add
 * word by word.
 * Call, per site, from the sums, the site's mixRef mask and the 2-bit genome base r alone; flat priors, no floating point:
 *   alleles      allele 0 = r; alleles 1 .. = the mask's other letters in A C G T order (the candidate set is mask + {r})
 *   genotypes    the unordered pairs (i <= j) of allele indices in VCF order k = j (j + 1) / 2 + i: 3, 6 or 10 of them
 *   raw          hom aa: sm[a] + sum of sx[c], c != a; het ab: sh[a] + sh[b] + sum of sx[c], c not in {a, b}; c runs over all four bases, so a
 *                base outside the candidate set is an error under every genotype
 *   PL_k         (raw_k - min_raw + 2048) >> 12, in 64 bits, uncapped
 *   GT           the first genotype in VCF order with raw_k == min_raw;  GQ = min(99, the smallest PL among the other genotypes)
 *   AD[i]        n[allele i];  DP = the sum of n over all four bases;  QUAL = the PL of genotype 0/0
 * Record: "contig\tpos\t.\tREF\tALT[,ALT..]\tQUAL\t.\tDP=dp\tGT:AD:DP:GQ:PL\ta/b:ad,..:dp:gq:pl,..\n", pos 1-based and contig-relative, the
 * contig the one that contains the site's global position (salt_gpu_index_set_contigs' table).  A site with DP == 0 prints QUAL `.` and the
 * sample field "./.:0,..:0:.:." (one 0 per allele).  Every site is printed, in genome order.  The header is salt_gt_header's (salt_host.h).
 * While the tally is on, every entry point that leaves result rows adds its batch behind the kernels that finish the rows, on the same
 * stream (k_gt_add: four 64-bit atomics into one 32-byte sector per event), with the qualities of the error profile's sources: the text
 * entry points' raw block, salt_gpu_ws_set_quals' bytes, or none.  The sums belong to the device index and are shared by its workspaces and
 * forks; they lie outside the image (128 bytes a site: 1.9 GB at 14.8 M sites; there is no narrower mode).  The site table is the SNP
 * counts' own, built by whichever of the two is enabled first.  With the tally off no kernel is launched; before the first enable nothing
 * is allocated, and every other call below fails with SALT_E_INVAL "never enabled".
 *   salt_gpu_index_gt_enable      the first enable builds the site table if need be and zeroes the sums (SALT_E_NOMEM names the size); on = 0
 *                                 stops and keeps them; min_mapq 0 .. 255 (above: SALT_E_INVAL).  No align call in flight, like the rest.
 *   salt_gpu_index_gt_reset       sums = 0
 *   salt_gpu_index_gt_fetch       out[0 .. n) = sums[first_site .. first_site + n); synchronises the device
 *   salt_gpu_index_gt_add         sums[first_site .. first_site + n) += in[0 .. n), by a kernel: how the tables of several GPUs are summed,
 *                                 chunk by chunk, and how any sums can be put in front of the call kernels.  A range that leaves
 *                                 [0, n_sites) is SALT_E_INVAL with the range in the message, for both.
 *   salt_gpu_index_gt_text_begin  starts the records of the sums as they stand: tile_sites = sites called at a time, 0 = the default (the
 *                                 text does not depend on it); bgzf != 0: whole BGZF blocks instead of text, deflated on the device,
 *                                 without the end-of-file block.  Needs the contig table.  No header.
 *   salt_gpu_index_gt_text_next   the next piece, in genome order: *data points into a buffer the index owns, valid until the next call on
 *                                 the index; *n_bytes == 0: complete.  The sums are never written by these two: the text can be made
 *                                 twice with the same bytes, and counting can go on afterwards.
 *   salt_gpu_ws_gt_uncount        takes back what the workspace's LAST successful align call added (the same kernel with the negated
 *                                 addends and that call's quality source).  Nothing to take back: SALT_OK. */
#define SALT_GT_Q_NONE 20
typedef struct { uint64_t n, sm, sx, sh; } salt_gt_base_t;
typedef struct { salt_gt_base_t b[4]; } salt_gt_site_t;                     /* A C G T; 128 bytes */
typedef struct {
    uint32_t tile_sites;        /* 0: default */
    int32_t  bgzf;              /* the pieces are BGZF blocks */
} salt_gt_text_opt_t;
int  salt_gpu_index_gt_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq);
int  salt_gpu_index_gt_reset(salt_gpu_index_t *ix);
int  salt_gpu_index_gt_fetch(salt_gpu_index_t *ix, uint64_t first_site, uint64_t n, salt_gt_site_t *out);
int  salt_gpu_index_gt_add(salt_gpu_index_t *ix, uint64_t first_site, uint64_t n, const salt_gt_site_t *in);
int  salt_gpu_index_gt_text_begin(salt_gpu_index_t *ix, const salt_gt_text_opt_t *opt);
int  salt_gpu_index_gt_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes);
int  salt_gpu_ws_gt_uncount(salt_gpu_ws_t *ws);

/* ---- SNP candidates off the index's sites (`salt --discover`) -----------------------------------------------------------
 * Which records contribute and the CIGAR walk are those of the SNP counts above (4.6): a record contributes iff it is mapped
 * (pos != 0xFFFFFFFF), not skipped, and mapq >= min_mapq; only the primary alignment counts, never an alternative (XA) hit; the record is
 * walked as the SAM / BAM writers lay it out (leading soft clip, M / I / D).
 * Events: an M column (genome position g, base s of SEQ as printed, L bases) is an event iff g < ref_len and s < L, SEQ[s] is a base b in
 * A C G T (0 .. 3), and the mixRef mask m = (ref[g >> 3] >> 4 * (g & 7)) & 15 has m != 0 and bit b CLEAR: the read shows a base the index
 * does not have there.  That holds at a plain position (one bit set) and at a known site (two or three bits: a third allele) alike; a
 * genome N (m == 0) and a mask of 15 give no event.
 * Quality: the FASTQ byte of the same sequenced base (index rev ? L - 1 - s : s in the FASTQ's order) minus 33, from the sources of the
 * genotype sums (the text entry points' raw block, salt_gpu_ws_set_quals' bytes, or none).  The event counts iff that quality is
 * >= min_baseq, or there is no usable quality: no qualities on the call, a quality range that leaves the call's quality bytes, a byte
 * outside 33 .. 126, SAM QUAL `*` in the host twin.
 * alt: uint64[ref_len], three fields of 21 bits a position.  Field k = popcount(~m & 15 & ((1 << b) - 1)) is the rank of b among the bases
 * outside the mask, in A C G T order; an event that counts adds 1 << 21 k.  Taking a batch back adds the two's complement, so the sums are
 * modular: they do not depend on batch order, stream, workspace or GPU, and the tables of several GPUs add word by word.  A field wraps
 * INTO ITS NEIGHBOUR beyond 2 097 151 observations of one base at one position.
 * diff: this tally's OWN uint32[ref_len + 1] difference array by the rule of the coverage above (4.7): every M run [g, end) cut at ref_len
 * adds 1 at g and takes 1 at end; depth[g] is the prefix sum, mod 2^32.  It is marked under THIS tally's MAPQ floor and counts every M
 * column, whatever its base (a read's N too) and whatever its quality: the denominator is the coverage by counted records, not the
 * bases that passed the quality filter.  It is not `--depth`'s array, whose floor is its own.
 * Call, per position, in integers: with n_b the field of a base b outside the mask, b is CALLED at g iff n_b >= min_alt and
 * 100 * n_b >= min_pct * depth[g].  A position is a candidate iff its mask is not 0 and a base is called there.
 * Defaults (definitions): min_mapq 20 (the only tally whose default floor is not 0: mismapped paralogs are what makes false SNPs),
 * min_baseq 20, min_alt 3, min_pct 20.  Ranges: min_mapq 0 .. 255, min_baseq 0 .. 93, min_alt 1 .. 2 097 151, min_pct 0 .. 100.
 * File: one line per candidate, in genome order, no header line (salt-idx's SNP-file reader has no comment syntax):
 *   "contig\tpos\talleles\tref\tdepth\tcA,cC,cG,cT\n"
 * pos 1-based and contig-relative, the contig the one that contains g (salt_gpu_index_set_contigs' table); alleles the letters of the mask
 * and of the called bases in A C G T order joined by '/' ("C/G"); ref the 2-bit genome's letter; depth = depth[g]; c* the count of a base
 * outside the mask and `.` for a base in it.  Columns 1 .. 4 are salt-idx's SNP-file format; it ignores the rest.  With all_sites the
 * index's sites (two or more bits in the mask) without a called base are printed too, their mask as alleles: the file is then a whole SNP
 * file for the rebuilt index.
 * While the tally is on, every entry point that leaves result rows adds its batch behind the kernels that finish the rows, on the same
 * stream (k_disc_add: two 32-bit atomics per M run, the columns compared with the mixRef eight at a time, one 64-bit atomic per event that
 * counts).  Both arrays belong to the device index and are shared by its workspaces and forks; they lie outside the image: 12 bytes a
 * genome position (there is no narrower mode).  With the tally off no kernel is launched; before the first enable nothing is allocated,
 * and every other call below fails with SALT_E_INVAL "never enabled".
 *   salt_gpu_index_disc_enable      the first enable allocates and zeroes both arrays (SALT_E_NOMEM names the size); on = 0 stops and keeps
 *                                   them; min_mapq 0 .. 255, min_baseq 0 .. 93 (above: SALT_E_INVAL).  No align call in flight.
 *   salt_gpu_index_disc_reset       both arrays = 0
 *   salt_gpu_index_disc_fetch       which = SALT_DISC_ALT: out is uint64[n], words [first, first + n) of alt, inside [0, ref_len);
 *                                   which = SALT_DISC_DIFF: out is uint32[n], words of diff, inside [0, ref_len].  Synchronises the device.
 *   salt_gpu_index_disc_add         array[first .. first + n) += in[0 .. n), by a kernel (64-bit words for alt, 32-bit for diff): how the
 *                                   arrays of several GPUs are summed, chunk by chunk, and how any arrays can be put in front of the text
 *                                   kernels.  A range that leaves the array is SALT_E_INVAL with the range in the message, for both.
 *   salt_gpu_index_disc_text_begin  starts the lines of the arrays as they stand: tile_positions = genome positions scanned at a time, 0 =
 *                                   the default (the text does not depend on it); bgzf != 0: whole BGZF blocks instead of text, deflated
 *                                   on the device, without the end-of-file block.  Needs the contig table.
 *   salt_gpu_index_disc_text_next   the next piece, in genome order: *data points into a buffer the index owns, valid until the next call on
 *                                   the index; *n_bytes == 0: complete.  A tile without a line yields no piece.  The arrays are never
 *                                   written by these two: the text can be made twice with the same bytes, and counting can go on.
 *   salt_gpu_index_disc_text_seen   once the text is complete: seen[c] = 1 iff contig c has a line, else 0 (cap >= the contigs' number)
 *   salt_gpu_ws_disc_uncount        takes back what the workspace's LAST successful align call added (the same kernel with the negated
 *                                   addends and that call's quality source).  Nothing to take back: SALT_OK. */
#define SALT_DISC_ALT  0
#define SALT_DISC_DIFF 1
#define SALT_DISC_FIELD_BITS 21
#define SALT_DISC_FIELD_MAX  2097151u
typedef struct {
    uint32_t min_alt;           /* 1 .. 2 097 151 */
    uint32_t min_pct;           /* 0 .. 100 */
    int32_t  all_sites;         /* also the index's sites without a called base */
    uint32_t tile_positions;    /* 0: default */
    int32_t  bgzf;              /* the pieces are BGZF blocks */
} salt_disc_text_opt_t;
int  salt_gpu_index_disc_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq, uint32_t min_baseq);
int  salt_gpu_index_disc_reset(salt_gpu_index_t *ix);
int  salt_gpu_index_disc_fetch(salt_gpu_index_t *ix, int which, uint64_t first, uint64_t n, void *out);
int  salt_gpu_index_disc_add(salt_gpu_index_t *ix, int which, uint64_t first, uint64_t n, const void *in);
int  salt_gpu_index_disc_text_begin(salt_gpu_index_t *ix, const salt_disc_text_opt_t *opt);
int  salt_gpu_index_disc_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes);
int  salt_gpu_index_disc_text_seen(salt_gpu_index_t *ix, uint8_t *seen, uint64_t cap);
int  salt_gpu_ws_disc_uncount(salt_gpu_ws_t *ws);

/* ---- the run's summary: mapping counts, histograms and per-contig counts (`salt --stats`) --------------------------------
 * The five tallies above are about the genome; this one is about the run: what `samtools flagstat`, `stats` and `idxstats` would be asked
 * for after a second pass over the output.
 * A record's fate is the error profile's R: skipped, unmapped (pos == 0xFFFFFFFF) and below min_mapq are exclusive and tested in that
 * order; the rest is COUNTED, and MAPPED means below or counted.  Only the primary alignment is read, never an alternative (XA) hit.
 * mate = 0 single end and read 2i of a pair, 1 for read 2i + 1.  L is the read's length from the offsets.  "Printed" is what the SAM / BAM
 * writers print: reverse iff strand != 0 single end, strand == 1 paired end; a paired-end row's soft clips seq_start and L - 1 - seq_end
 * (single end prints none); an XA entry for every listed hit whose pos differs from the row's; for a pair, flag 0x2, RNEXT, PNEXT and
 * TLEN by the rule of alnpe_sam (sam.c:350-358) with the -a / -b window of the call's salt_pe_opt_t: both mates mapped on one contig, the
 * template inside the window and not 0.  The contig of a position is the one salt_gpu_index_set_contigs' table gives (the SAM writer's
 * search); POS is 1-based and contig-relative.
 * Tables, all uint64, owned by the device index and shared by its workspaces and forks, outside the image.  SALT_STATS_CELLS cells at the
 * offsets below, then, apart, CT:
 *   SN[2][16]   per mate: 0 records seen, 1 skipped, 2 unmapped, 3 below the floor, 4 counted, 5 counted and printed reverse, 6 counted
 *               with any I, D or printed soft clip, 7 counted with at least one printed XA entry, 8 counted with flag 0x2, 9 counted with
 *               the mate unmapped, 10 counted with the mate mapped on another contig, 11 bases of records not skipped (sum of L), 12 M
 *               columns of counted records with g < ref_len (the walk and the cut of the coverage above), 13 / 14 / 15 I, D and printed S
 *               bases of counted records
 *   MQ[2][256]  mapped records by MAPQ
 *   RL[2][513]  records not skipped, by L
 *   GC[2][102]  records not skipped, by GC percent: gc = bases with code 1 or 2, n = bases with code 0 .. 3, bin (200 gc + n) / (2 n) in
 *               integers (the percentage, halves rounded up); bin 101: n == 0
 *   XA[2][8]    counted records by their number of printed XA entries (0 .. 5; more would count in 7)
 *   IS[4097]    one entry per pair, from the mate-0 record when it is counted and its printed TLEN is not 0: index min(|TLEN|, 4096)
 *   OR[4]       mate-0 counted records whose mate is mapped on the same contig: 0 inward (the strands differ and POS of the forward mate
 *               <= POS of the reverse mate), 1 outward (the strands differ otherwise), 2 the same strand; 3 stays 0
 *   ID[2][65]   the I ops (row 0) and D ops (row 1) of counted records by min(length, 64)
 *   CT[n][8]    per contig of the table, by the contig of the record's pos: 0 / 1 mapped records of mate 0 / 1, 2 / 3 counted records of
 *               mate 0 / 1, 4 counted and printed reverse, 5 the record's SN 12 columns, 6 and 7 stay 0
 * The sums do not depend on batch order, stream, workspace or GPU, and the cells are 64-bit: the tables of several GPUs add cell by cell.
 * (k_stats_add sums per workgroup in 32-bit LDS cells that it sends on once: such a cell grows by less than 2^18 a record and a
 * workgroup owns 2 048 records.)  While the tally is on, every entry point that leaves result rows adds its batch behind the kernels that
 * finish the rows, on the same stream, under salt_gpu_ws_set_polish too.  With it off no kernel is launched; before the first enable
 * nothing is allocated.
 *   salt_gpu_index_stats_enable   the first enable allocates and zeroes the tables (SALT_E_NOMEM names the size) and needs the contig table
 *                                 (salt_gpu_index_set_contigs; without it SALT_E_INVAL names it); on = 0 stops and keeps them; min_mapq
 *                                 0 .. 255 (above: SALT_E_INVAL).  Call with no align call in flight, like fetch.  A contig table of another
 *                                 size set afterwards makes the align calls fail with SALT_E_INVAL while the tally is on.
 *   salt_gpu_index_stats_fetch    synchronises the device; cells (SALT_STATS_CELLS of them) and ct (8 per contig) may each be NULL; a cap
 *                                 that is too small is SALT_E_INVAL with the numbers in the message; reset != 0 zeroes all tables
 *                                 afterwards.  Never enabled: SALT_E_INVAL.
 *   salt_gpu_ws_stats_uncount     takes back what the workspace's LAST successful align call added (the same kernel with delta 2^64 - 1;
 *                                 the call's buffers must be untouched since).  Nothing to take back: SALT_OK. */
#define SALT_STATS_SN       0u                    /* [2][16] */
#define SALT_STATS_MQ       32u                   /* [2][256] */
#define SALT_STATS_RL       544u                  /* [2][513] */
#define SALT_STATS_GC       1570u                 /* [2][102] */
#define SALT_STATS_XA       1774u                 /* [2][8] */
#define SALT_STATS_IS       1790u                 /* [4097] */
#define SALT_STATS_OR       5887u                 /* [4] */
#define SALT_STATS_ID       5891u                 /* [2][65] */
#define SALT_STATS_CELLS    6021u
#define SALT_STATS_IS_MAX   4096u                 /* the last bin of IS: templates of this length and longer */
#define SALT_STATS_CT_LDS   64u                   /* contigs whose CT rows a workgroup of k_stats_add sums in LDS; the others' go to global memory directly */
int  salt_gpu_index_stats_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq);
int  salt_gpu_index_stats_fetch(salt_gpu_index_t *ix, uint64_t *cells, uint64_t cap_cells, uint64_t *ct, uint64_t cap_ct, int reset);
int  salt_gpu_ws_stats_uncount(salt_gpu_ws_t *ws);

/* ---- indel candidates (`salt --indels`) -----------------------------------------------------------------------------------
 * The seventh row tally, and the first whose table is not indexed by position: a hash table of allele keys.  This is the definition; it
 * is implemented three times (the kernels of salt_indel.hip, the host twin salt_indel_add_sam / salt_indel_text, tests/indel_check.py).
 * Contributing records are those of the SNP counts (4.6): mapped (pos != 0xFFFFFFFF), not skipped, mapq >= min_mapq (default 20, as for
 * the SNP candidates); only the primary alignment, never an alternative (XA) hit.  The row's ops are walked as tally_m_runs walks them: g
 * starts at pos and s at the leading soft clip (0 single end); M advances both, I advances s, D advances g, an op of 3 advances neither.
 * L is the read's length from the offsets.  n_ops is the row's op count (the soft clips the writers print are not ops).
 * Genome letters: letter(x) = the 2-bit genome's base at x (text, which the SAM writers read; a genome N reads as its pac letter) for
 * x < the 2-bit genome's length, else A.  Contigs: those of salt_gpu_index_set_contigs' table; contig c is [off[c], end[c]) with end[c] =
 * off[c + 1], and ref_len for the last one; the contig of a position is the last one that begins at or in front of it.
 * Events: an I or D op k of length n, met at (g, s), is an EVENT iff all of
 *   (length)  I: 1 <= n <= 12; D: 1 <= n <= 63;
 *   (anchor)  0 < k < n_ops - 1, and ops k - 1 and k + 1 are both M with a length of at least 1;
 *   (contig)  with c the contig of the anchor g - 1: g < end[c]; for D also g + n <= end[c] and g + n <= ref_len;
 *   (bases)   for I: s + n <= L and the n bases of SEQ as printed at [s, s + n) are all A, C, G or T (for a row printed reverse they are
 *             the sequenced bases L - 1 - x, complemented).
 * An I or D op that is no event goes to exactly one counter: `long` when (length) fails, else `unanchored`.
 * Left shift (normalisation), against the 2-bit genome alone.  D: while g - 1 > off[c] and letter(g - 1) == letter(g + n - 1): g -= 1.
 * I with bases b[0 .. n): while g - 1 > off[c] and letter(g - 1) == b[n - 1]: b is rotated right by one, letter(g - 1) entering at the
 * front, and g -= 1.  At most SALT_INDEL_MAX_SHIFT steps are taken: the bound on work is part of the definition.  The anchor never
 * leaves the contig: the leftmost allele has its anchor on the contig's first position.
 * Key, 64 bits, never 0: bit 63 = 1; bits 62 .. 31 = g (the first position behind the anchor); bit 30 = 1 for D; bits 29 .. 24 = n; bits
 * 23 .. 0 = the inserted bases, 2 bits each, b[0] highest, left-justified in the 24 bits (0 for D).  Keys sorted as integers are in genome
 * order.  A word is a WELL-FORMED key iff bit 63 is set, 1 <= g <= ref_len, n is in its type's range, and for I the bits below the 2 n
 * used ones are 0, for D all 24; only well-formed keys are ever printed (others can only come from salt_gpu_index_indel_add).
 * Value, one 64-bit word: observations from rows printed forward in the low 32 bits, from rows printed reverse in the high 32.  An event
 * adds 1 or 1 << 32; taking a batch back adds the two's complement.
 * Table: 2^log2_slots slots of 16 bytes (key, value), 2^6 .. 2^28 slots, fixed at the first enable; default 2^24 (256 MB).  The home slot
 * of a key is (key * 0x9E3779B97F4A7C15) >> (64 - log2_slots); probing is linear over at most SALT_INDEL_PROBE slots (and at most all of
 * them) and wraps at the table's end.  On each slot atomicCAS(&slot.key, 0, key): 0 or key returned means the slot is this allele's, and
 * one 64-bit atomicAdd on its value follows; anything else moves on.  A probe run that ends without a slot adds the event to `dropped`
 * instead.  Nothing waits for another thread.  Taking back (a negative addend) claims nothing: it looks the key up along the same run, and
 * a key that is not found (an empty slot, or the run's end) takes its event back from `dropped`.  A slot is never emptied, so a key that
 * was dropped once is dropped always, and tabled + dropped is the number of events added, whatever the order.
 * stat, uint64[4]: SALT_INDEL_TABLED, _DROPPED (events), _LONG, _UNANCHORED (ops).
 * diff: this tally's OWN uint32[ref_len + 1] difference array under its own floor, marked per M run exactly as the SNP candidates' (4.10).
 * Call, in integers, for a well-formed key with value (fwd, rev) and depth = depth[g - 1] (the anchor's): the allele is called iff
 * fwd + rev >= min_alt and 100 * (fwd + rev) >= min_pct * depth.  Defaults 3 and 20; ranges min_alt 1 .. 2^32 - 1, min_pct 0 .. 100.
 * File: one VCF 4.2 record per called allele, in key order: "CHROM\tPOS\t.\tREF\tALT\t.\t.\tINFO\n"; CHROM the contig of the anchor, POS
 * the anchor, 1-based and contig-relative; for D REF = letter(g - 1) letter(g) .. letter(g + n - 1) and ALT = letter(g - 1); for I REF =
 * letter(g - 1) and ALT = letter(g - 1) b[0] .. b[n - 1]; INFO = "TYPE=INS|DEL;LEN=n;DP=depth;AO=fwd+rev;AOF=fwd;AOR=rev".
 * While the tally is on, every entry point that leaves result rows adds its batch behind the kernels that finish the rows, on the same
 * stream (k_indel_add: a thread per record, no queue, no spin).  Table, counters and diff belong to the device index, outside the image.
 * With the tally off no kernel is launched; before the first enable nothing is allocated and every other call below is SALT_E_INVAL.
 *   salt_gpu_index_indel_enable      the first enable allocates and zeroes table, counters and diff (SALT_E_NOMEM names the size) and
 *                                    needs the contig table (salt_gpu_index_set_contigs); log2_slots 6 .. 28, 0 = the default, and later
 *                                    enables must name the same size or 0; on = 0 stops and keeps everything.  No align call in flight.
 *   salt_gpu_index_indel_reset       table, counters and diff = 0
 *   salt_gpu_index_indel_stats       the four counters; synchronises the device
 *   salt_gpu_index_indel_fetch       the slots with a non-zero value as (key, value) pairs, uint64[2 n], in key order; *n is their number
 *                                    whatever cap (in pairs) is, and min(cap, *n) pairs are written
 *   salt_gpu_index_indel_add         inserts n hand-given (key, value) pairs by a kernel with the insert routine above, the value as the
 *                                    addend and its two halves' sum as the events: how the tables of several GPUs are summed
 *   salt_gpu_index_indel_fetch_diff / _add_diff   words [first, first + n) of diff, inside [0, ref_len], as the SNP candidates'
 *   salt_gpu_index_indel_text_begin  starts the records of table and diff as they stand; tile_positions = genome positions of diff scanned
 *                                    at a time, 0 = the default (the text does not depend on it); bgzf != 0: whole BGZF blocks, without
 *                                    the end-of-file block
 *   salt_gpu_index_indel_text_next   the next piece, cut at a line end: *data points into a buffer the index owns, valid until the next
 *                                    call on the index; *n_bytes == 0: complete.  Table and diff are only read: the text can be made
 *                                    twice, and counting can go on.
 *   salt_gpu_ws_indel_uncount        takes back what the workspace's LAST successful align call added.  Nothing to take back: SALT_OK. */
#define SALT_INDEL_MAX_INS    12u
#define SALT_INDEL_MAX_DEL    63u
#define SALT_INDEL_MAX_SHIFT  4096u
#define SALT_INDEL_PROBE      128u
#define SALT_INDEL_LOG2_MIN   6u
#define SALT_INDEL_LOG2_MAX   28u
#define SALT_INDEL_LOG2_DEFAULT 24u
#define SALT_INDEL_TABLED     0
#define SALT_INDEL_DROPPED    1
#define SALT_INDEL_LONG       2
#define SALT_INDEL_UNANCHORED 3
typedef struct {
    uint32_t min_alt;           /* 1 .. 2^32 - 1 */
    uint32_t min_pct;           /* 0 .. 100 */
    uint32_t tile_positions;    /* 0: default */
    int32_t  bgzf;              /* the pieces are BGZF blocks */
} salt_indel_text_opt_t;
int  salt_gpu_index_indel_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq, uint32_t log2_slots);
int  salt_gpu_index_indel_reset(salt_gpu_index_t *ix);
int  salt_gpu_index_indel_stats(salt_gpu_index_t *ix, uint64_t out[4]);
int  salt_gpu_index_indel_fetch(salt_gpu_index_t *ix, uint64_t cap, uint64_t *entries, uint64_t *n);
int  salt_gpu_index_indel_add(salt_gpu_index_t *ix, const uint64_t *entries, uint64_t n);
int  salt_gpu_index_indel_fetch_diff(salt_gpu_index_t *ix, uint64_t first, uint64_t n, uint32_t *out);
int  salt_gpu_index_indel_add_diff(salt_gpu_index_t *ix, uint64_t first, uint64_t n, const uint32_t *in);
int  salt_gpu_index_indel_text_begin(salt_gpu_index_t *ix, const salt_indel_text_opt_t *opt);
int  salt_gpu_index_indel_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes);
int  salt_gpu_ws_indel_uncount(salt_gpu_ws_t *ws);

/* ---- FASTQ text in, SAM text out ------------------------------------------------------------------------------------
 * query_read_seq (query.c:146-239) + alnse_core1 + aln_samse / sam_add_xa / sam_add_md_nm (sam.c:87-328) for one block of whole,
 * strict 4-line FASTQ records: the block is parsed, aligned and formatted on the device; the host only hands over the text and
 * gets the SAM records of the block back (one line per read, input order, a skipped read = an empty line).  `fastq` should be
 * page-locked (salt_gpu_host_alloc) and must end with a newline; *sam points into a page-locked buffer the workspace owns and
 * stays valid until the next call on it.  Needs the contig table (bntann1_t offset + name per sequence, bntseq.h) for RNAME / POS.
 * Multi-line FASTQ records are not read here (SALT_E_INVAL names the record); callers fall back to their host parser. */
typedef struct { int32_t print_xa_cigar, print_nm_md; const char *rg_id; } salt_text_opt_t;      /* -c, -d, -g */
int  salt_gpu_index_set_contigs(salt_gpu_index_t *ix, int32_t n, const int64_t *offsets, const char *const *names);
/* Paired end (alnpe_core1 + alnpe_sam, sam.c:331-457): fastq1 / fastq2 hold the same number of whole 4-line records, mate 1 and mate 2 of
 * pair p at the same record index; the SAM block holds both records of every pair in order, each followed by the reference's empty
 * line (alnpe.c:640-648).  Needs salt_gpu_index_set_pac and the contig table. */
int  salt_gpu_align_pe_text(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, const salt_pe_opt_t *pe, const salt_text_opt_t *topt,
                            const char *fastq1, uint64_t n1_bytes, const char *fastq2, uint64_t n2_bytes,
                            const char **sam, uint64_t *sam_bytes, uint32_t *n_pairs);
/* optional: size the workspace's text buffers ahead of the first call (blocks of up to max_block_bytes with about est_reads reads of
 * up to max_read_len bases, about est_sam_bytes of SAM); what a later block needs beyond that is grown then.  host_sam (may be NULL):
 * page-locked memory of the caller's (salt_gpu_host_alloc, e.g. allocated while the index was loading) the SAM text is returned in as
 * long as it suffices; it stays the caller's to free, after the workspace is destroyed. */
int  salt_gpu_ws_reserve_text(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, uint64_t max_block_bytes, uint32_t est_reads, uint32_t max_read_len,
                              uint64_t est_sam_bytes, void *host_sam, uint64_t host_sam_bytes);
int  salt_gpu_align_se_text(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, const salt_text_opt_t *topt, const char *fastq, uint64_t n_bytes,
                            const char **sam, uint64_t *sam_bytes, uint32_t *n_reads);
/* BGZF output (`salt --bgzf`): after salt_gpu_ws_set_sam_bgzf(ws, 1) the two text entry points deflate the SAM block on the device, right
 * behind the kernel that wrote it, and return whole BGZF blocks in *sam / *sam_bytes (htslib's blocked gzip: independent gzip members with
 * a 'BC' extra field, each holding at most 32 640 bytes of the text; no end-of-file block -- that one is the caller's, after its last
 * block).  Only the compressed bytes cross to the host.  A block of text that does not compress leaves as a stored block, 31 bytes larger
 * than its text; the workspace's buffers (and what it takes from the host_sam of salt_gpu_ws_reserve_text) allow for that. */
int  salt_gpu_ws_set_sam_bgzf(salt_gpu_ws_t *ws, int on);
/* BAM output (`salt --bam`): after salt_gpu_ws_set_sam_bam(ws, 1) the two text entry points write the block's records as BAM records (SAM
 * specification 4.2; k_bam_len / k_bam_write) where they wrote SAM lines: one record per read or mate in input order, none for a skipped read
 * and none for the paired-end driver's blank lines; NM in the smallest unsigned type that holds it, XV always as an array B:I; no file header
 * (salt_bam_header of salt_host.h writes that).  The bytes equal salt_bam_from_sam of the SAM lines the same call would have returned.
 * Whether they then pass through the device compressor is still salt_gpu_ws_set_sam_bgzf's decision: with it *sam holds BGZF blocks cut
 * every 32 640 bytes of the record stream (records straddle blocks, as the format allows), without it the raw records.  A read name longer
 * than 254 bytes cannot be a BAM name: the call fails with SALT_E_INVAL and a message that starts with "BAM:". */
int  salt_gpu_ws_set_sam_bam(salt_gpu_ws_t *ws, int on);
/* Polished output (`salt --polish`): after salt_gpu_ws_set_polish(ws, mode) -- 0 off, 1 Landau-Vishkin re-scoring (polish's default), 2
 * Smith-Waterman (polish -s) -- salt_gpu_align_se_text, salt_gpu_align_se_text_dev and salt_gpu_align_pe_text return in *sam the records the
 * reference's `polish` prints for the block's SAM lines, and no SAM line is ever formatted: the hits go from the result rows straight into
 * the polish kernels (salt_polish.hip, k_pl_rows), on the call's stream, where the SAM kernels ran.  No header.  A skipped read (more than
 * 200 N) gives no record; a pair with a skipped mate gives none for either mate.  *n_reads / *n_pairs count the input as before.  The
 * records pass through the device compressor when salt_gpu_ws_set_sam_bgzf is on.  -c / -d / the read group change nothing here.
 * Needs salt_gpu_index_set_pac (single end too: the index's own device copy of the 2-bit genome is what the windows are read from) and the
 * contig table; SALT_E_INVAL names what is missing.  Cannot be combined with salt_gpu_ws_set_sam_bam (SALT_E_INVAL, whichever is set second).
 * A failed record gives the errors of salt_gpu_polish_text: "Out of reference length", the band message under mode 2, "push cigar error".
 * The polish buffers and Landau-Vishkin tables are the workspace's own, allocated by the first call and freed with it.
 * Outside the contract: a read with an empty name (in SAM text the leading tab vanishes under strtok and `polish` shifts the fields; here the
 * record is printed with its empty name); an index with two contigs of one name (`polish` resolves the name to the last of them; here a hit
 * keeps the contig it lies in). */
int  salt_gpu_ws_set_polish(salt_gpu_ws_t *ws, int mode);
/* Trimming (`salt --trim-*`): after salt_gpu_ws_set_trim(ws, &opt) the text entry points (salt_gpu_align_se_text, _se_text_dev,
 * salt_gpu_align_pe_text) trim every read of the block on the device, between the parser and the aligner (k_fq_trim), and everything behind
 * it -- the aligner, the SAM, BAM and polish writers, the tallies -- sees the trimmed read: the block equals the block the same call returns,
 * trimming off, for a FASTQ trimmed beforehand by salt_host.h's salt_trim_fastq.  The rule, integers only (csrc/salt_trim_rule.h is its one
 * definition, for the device and the host), on a read of L >= 1 bases, each step on the span [beg, end) the one before left:
 *   1. front, tail   0 .. 511: beg += front, end -= tail, saturating (end >= beg)
 *   2. qual          0 off, 1 .. 93: s = best = 0, cut = end; for i = end - 1 down to beg: s += qual - (byte[i] - 33) (a byte below 33
 *                    counts as quality 0); stop when s < 0; when s > best: best = s, cut = i.  end = cut.  (bwa aln -q, cutadapt -q)
 *   3. adapter       1 .. 64 letters of ACGTacgt; adapter searches mate 0 (single end: every read), adapter2 mate 1 (without it mate 1 is
 *                    searched with adapter).  Every start p from beg upward, ov = min(A, end - p); the search ends at the first p with
 *                    ov < min_overlap (1 .. 64); mm = the j < ov where the read's letter p + j differs from the adapter's letter j (case
 *                    ignored, a read letter outside ACGTacgt always differs); the leftmost p with 100 mm <= error_pct ov (0 .. 50) wins:
 *                    end = p.  No indels, no wildcards.
 *   4. floor         end <= beg: beg = min(beg, L - 1), end = beg + 1 -- no record is dropped and none becomes empty.
 * SALT_MAX_READ_LEN applies to the trimmed length.  A null pointer or an all-zero struct switches trimming off, and the calls launch what
 * they launch today.  A value out of range, adapter2 without adapter, min_overlap or error_pct without an adapter: SALT_E_INVAL, and
 * salt_gpu_last_error() names the field.  The strings are copied.
 * Counters: uint64 out[16], eight per mate (mate 0 first; single end counts as mate 0): 0 reads, 1 bases in, 2 bases out, 3 reads the
 * quality step shortened, 4 bases it removed, 5 reads the adapter step shortened, 6 bases it removed, 7 reads the floor applied to.
 * (Reads the clips shortened: all of them when front or tail is set.)  They add up over the workspace's calls until reset.  A block comes
 * back with the parser's control words and is added once the parser has accepted it -- a block refused as "not 4-line FASTQ" adds nothing, its
 * caller reads those records another way -- so salt_gpu_ws_trim_counts waits for nothing; salt_gpu_ws_trim_uncount takes back what the
 * workspace's last call added (a block the caller aligned and then drops), as the tallies' _uncount calls do.
 * salt_gpu_trim_spans: the parser and k_fq_trim alone on one block of 4-line FASTQ (at most max_reads records), every record as mate `mate`:
 * beg_end[2 i], beg_end[2 i + 1] = the span of record i in its untrimmed read.  The block's counters are added too. */
typedef struct salt_trim_opt {
    const char *adapter;  uint32_t adapter_len;      /* NULL / 0: no adapter search */
    const char *adapter2; uint32_t adapter2_len;     /* NULL / 0: mate 1 is searched with `adapter` */
    uint32_t front, tail, qual, min_overlap, error_pct;
} salt_trim_opt_t;
int  salt_gpu_ws_set_trim(salt_gpu_ws_t *ws, const salt_trim_opt_t *opt);
int  salt_gpu_ws_trim_counts(salt_gpu_ws_t *ws, uint64_t out[16], int reset);
int  salt_gpu_ws_trim_uncount(salt_gpu_ws_t *ws);
int  salt_gpu_trim_spans(salt_gpu_ws_t *ws, const char *fastq, uint64_t n_bytes, int mate, uint32_t *beg_end);
/* The pair rule (`salt --trim-pair-overlap`): after salt_gpu_ws_set_trim_pair(ws, &opt) salt_gpu_align_pe_text finds each
 * pair's adapters from the mates' overlap, as step 2p between steps 2 and 3 above (k_fq_trim_pair, a wave a pair, in k_fq_trim's place).  It
 * works with or without salt_gpu_ws_set_trim; the single-end entry points ignore it.  All positions are in the untrimmed reads of L1 and L2
 * letters; [b1, e1) and [b2, e2) are what steps 1 and 2 left:
 *   2p. for a candidate insert length I >= 1, column j of mate 1 faces letter I - 1 - j of mate 2, complemented.  Compared are the columns
 *       max(b1, I - e2) <= j < min(e1, I - b2): ov(I) of them, mm(I) of those where the two letters are no complementary pair (case ignored,
 *       a letter outside ACGTacgt on either side always differs).  I is accepted when ov >= min_overlap (1 .. 512) and
 *       100 mm <= error_pct ov (0 .. 50).  The LARGEST accepted I in 1 .. e1 + e2 - min_overlap wins: e1 = min(e1, I), e2 = min(e2, I).
 *       A pair with a mate longer than SALT_MAX_READ_LEN skips the step.  Mates are not merged and no base is corrected.
 * A null pointer or an all-zero struct switches the rule off, and the call launches what it launches today; a value out of range:
 * SALT_E_INVAL, the field named.  Pair counters, uint64 out[8]: 0 pairs, 1 pairs with an accepted layout, 2 pairs in which a mate was
 * shortened, 3 mate-1 reads shortened, 4 bases taken from mate 1, 5 mate-2 reads shortened, 6 bases taken from mate 2, 7 pairs that skipped the
 * step for a mate's length.  The sixteen above keep their meaning: 5 and 6 count what step 3 took from what step 2p left, 2 is the final span.
 * The pair counters travel and add up with the sixteen, and salt_gpu_ws_trim_uncount takes both back.
 * salt_gpu_trim_pair_spans: the parser and k_fq_trim_pair alone on two blocks (at most max_reads records together): beg_end[4 p ..] =
 * b1, e1, b2, e2 of pair p.  The blocks' counters of both kinds are added too. */
typedef struct salt_trim_pair_opt { uint32_t min_overlap, error_pct; } salt_trim_pair_opt_t;
int  salt_gpu_ws_set_trim_pair(salt_gpu_ws_t *ws, const salt_trim_pair_opt_t *opt);
int  salt_gpu_ws_trim_pair_counts(salt_gpu_ws_t *ws, uint64_t out[8], int reset);
int  salt_gpu_trim_pair_spans(salt_gpu_ws_t *ws, const char *fastq1, uint64_t n1, const char *fastq2, uint64_t n2, uint32_t *beg_end);
/* The same kernels on their own, host buffers in and out: text[0 .. n_bytes) -> ceil(n_bytes / 32640) BGZF blocks in out, *out_bytes of them
 * (0 for an empty text; no end-of-file block).  The same text gives the same bytes on every run.  SALT_E_CAPACITY when out_cap is too
 * small: n_bytes + 31 bytes per block is the exact bound, 65 536 bytes per block always suffice. */
int  salt_gpu_bgzf_deflate(int device, const void *text, uint64_t n_bytes, void *out, uint64_t out_cap, uint64_t *out_bytes);
/* BGZF input (blocked-gzip FASTQ): the members of a file inflated on the device (k_bgzf_inflate, one workgroup per member: stored, fixed and
 * dynamic blocks, any number per member; the CRC-32 and ISIZE of every member checked there).  Only the compressed bytes cross to the device.
 * A member that does not inflate to exactly its ISIZE bytes with its CRC-32 makes the call return SALT_E_DATA; salt_gpu_last_error() names the
 * first such member and the reason.  Damaged input cannot make a kernel read or write outside the member's bytes and its own text range.
 *
 * salt_gpu_bgzf_inflate: host buffers in and out.  bgzf[0 .. n_bytes) must be whole members (an end-of-file block is one, of no text); they are
 * found by their BSIZE fields.  *out_bytes = the text's length, also with SALT_E_CAPACITY (out_cap smaller than that; nothing is written then). */
int  salt_gpu_bgzf_inflate(int device, const void *bgzf, uint64_t n_bytes, void *out, uint64_t out_cap, uint64_t *out_bytes);
/* The members of one chunk -> the workspace's device text buffer, which holds them until the next call.  blocks[0 .. n_cbytes) (page-locked for
 * an asynchronous copy) holds n_blocks members back to back; c_off / u_off (n_blocks + 1 entries each, ascending, from 0) say where every
 * member starts in blocks and where its text starts in the text: the caller has them from the BSIZE and ISIZE fields, without inflating. */
int  salt_gpu_ws_inflate_bgzf(salt_gpu_ws_t *ws, const void *blocks, uint64_t n_cbytes, uint32_t n_blocks, const uint32_t *c_off, const uint32_t *u_off);
/* Bytes [off, off + n) of that text to the host: the caller looks for record boundaries in a window, not in the whole text. */
int  salt_gpu_ws_text_peek(salt_gpu_ws_t *ws, uint64_t off, uint64_t n, void *dst);
/* salt_gpu_align_se_text over bytes [off, off + n_bytes) of that text (a device-to-device copy where the other takes its block from the host);
 * add_newline: a newline is put behind the range (the file's last record lacks its own).  Results and returns as salt_gpu_align_se_text,
 * SALT_E_INVAL for a range that is not whole 4-line FASTQ records included. */
int  salt_gpu_align_se_text_dev(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, const salt_text_opt_t *topt, uint64_t off, uint64_t n_bytes, int add_newline,
                                const char **sam, uint64_t *sam_bytes, uint32_t *n_reads);
int  salt_gpu_host_alloc(uint64_t bytes, void **ptr);      /* page-locked host memory for the text buffers */
void salt_gpu_host_free(void *ptr);
/* Multi-GPU drivers (`salt --gpus N`, which stands where alnse_core's pthread fan-out is, alnse.c:1419-1429): the host NUMA node of a device
 * (-1 = unknown), so that a device's worker threads and their page-locked buffers can be kept on the socket it is attached to. */
int  salt_gpu_device_numa_node(int device, int *node);
int  salt_gpu_device_count(int *n);

/* Same work on device-resident buffers; only enqueues on `hip_stream` (a hipStream_t, NULL = default).  Every call is its own enqueue:
 * the kernels take the call's epoch by value from the workspace (the R seed rows of another call are dead by it), so a call must not
 * be captured into a hipGraph and replayed -- a replay would run at the captured epoch and take the previous replay's rows for live. */
int  salt_gpu_align_se_resident(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, uint32_t n_reads,
                                uint32_t max_read_len, const void *d_seqs, const void *d_offs,
                                void *d_results, void *hip_stream);

/* Per-kernel device time.  After salt_gpu_ws_timing(ws, 1) every resident/host align call brackets its
 * kernels with HIP events on the stream it launches on; salt_gpu_ws_kernel_ms synchronises, adds the
 * elapsed times of all calls since the last read into ms[0] k_pack, ms[1] k_seed, ms[2] k_light, ms[3] k_heavy,
 * ms[4] k_gap, ms[5] k_gapfin, ms[6] k_cigar, and for paired-end calls ms[7] k_pair, ms[8] k_sw (the Smith-Waterman kernels k_swf, k_swf1, k_swr, k_swtb together), ms[9] k_pe_final (with the k_cigar pass
 * behind it); returns the number of calls in *n_calls and resets.  At most 256 calls are kept. */
#define SALT_N_KERNELS 10
int  salt_gpu_ws_timing(salt_gpu_ws_t *ws, int enable);
int  salt_gpu_ws_kernel_ms(salt_gpu_ws_t *ws, double ms[SALT_N_KERNELS], uint32_t *n_calls);

/* The reads of the LAST batch that k_light handed to k_heavy (diagnostics / per-kernel accounting):
 * *n = how many; ids[0..min(*n,cap)) = their indices in the batch, in queue order. */
int  salt_gpu_ws_heavy_reads(salt_gpu_ws_t *ws, uint32_t *ids, uint32_t cap, uint32_t *n);

/* Plain device buffers for callers without a HIP runtime of their own (resident inputs / results, image copies). */
int  salt_gpu_buffer_alloc(int device, uint64_t bytes, void **dev_ptr);
int  salt_gpu_buffer_free(int device, void *dev_ptr);
/* *equal = 1 iff the two device buffers hold the same bytes (bytes % 4 == 0); tests compare index images with it */
int  salt_gpu_buffer_equal(int device, const void *a, const void *b, uint64_t bytes, int *equal);

/* Unit entry of the candidate rule the kernels evaluate on UNSORTED lists: case i has candidates
 * pos/val[offs[i]..offs[i+1]) (val > vmax = no candidate) and the incoming bound bound_in[i].  mode 0: gap-free rule
 * (code_kmismatch, alnse.c:348-369; distances 0..3, range filter pos < ref_len) by rule_unsorted; 1: the same by
 * rule_sparse; 2: gapped rule (code_kdiff, alnse.c:371-393; distances 0..12, filter !(pos + L + 4 >= ref_len)); 3: as 1 by
 * rule_sparse on half-waves (32 lanes, what k_light2 runs), cases 2b and 2b + 1 side by side in the halves of wave b; 4: as 1 on
 * quarters of a wave (16 lanes, what k_light4 runs), cases 4b .. 4b + 3 side by side in the quarters of wave b; 5: as 2 through
 * the front end for lists in global memory (what k_gapfin runs: several trips of 64 rows in flight, the first batch asked for ahead).
 * out[i][18] = found, best_pos, best_dist, n_hits, a0, bound_out, then 6 x (hit_pos, hit_dist) in position order. */
int  salt_gpu_diag_rule(uint32_t n_cases, const uint32_t *pos, const uint8_t *val, const uint32_t *offs, const uint32_t *bound_in,
                        uint32_t L, uint32_t ref_len, int mode, uint32_t *out);

/* Unit entry of the candidate verifiers (tests): case i = read seqs[offs[i]..offs[i+1]) against candidates
 * cand[cand_offs[i]..cand_offs[i+1]) (<= 256) on the 4-bit mixRef `ref_words`; mode 0 = one candidate per lane, 1 / 2 = four / eight lanes
 * per candidate (reads <= 120 / 248 bases), 3 / 4 = the two-strand variants of 1 / 2, 5 / 6 = 3 / 4 on half-waves (32 lanes, what
 * k_light2 runs), cases 2b and 2b + 1 side by side in the halves of wave b, 7 = 3 on quarters of a wave (16 lanes, what k_light4
 * runs), cases 4b .. 4b + 3 side by side in the quarters of wave b.  out[j] = masked Hamming distance 0..3 of candidate
 * j or 255 (more, or a candidate at or beyond ref_len -- a locate that wrapped below 0, alnse.c:672-673,762 -- which must never be
 * dereferenced).  Mirrors ed_mismatch (editdistance.c:88-163) under code_kmismatch's cap (alnse.c:348-369). */
int  salt_gpu_diag_verify(const uint32_t *ref_words, uint32_t ref_len, uint32_t n_cases, const uint8_t *seqs, const uint32_t *offs,
                          const uint32_t *cand, const uint32_t *cand_offs, int mode, uint8_t *out);

/* Unit entry of the rank primitives (salt_device.h) over an attached index: query i = queries[3i..] = (x, y, c), answered by every
 * restatement of the rank query.  mode 0, the C index: x and y in {0xFFFFFFFF} or [0, c_seq_len], c in 0..3.  mode 1, the R index: x and
 * y in [0, r_text_len + 1], c in 0..4 ('#' = 4).  Anything else: SALT_E_INVAL, and nothing is launched.  out[12i..]:
 *   [0] Occ(x, c), [1] Occ(y, c)            by c_occ / r_occ
 *   [2], [3] the same pair                  by c_occ2 / r_occ2, [6] the number of blocks it says it fetched
 *   [4], [5] the same pair                  by c_occ2_addr + c_occ2_eval / r_occ2_addr + r_occ2_eval over exactly the blocks _addr
 *                                           names (a half it does not name holds all ones), [7] _eval's block count, [8] the number
 *                                           of blocks _addr named
 *   [9] the BWT symbol of row x             by c_sym as the suffix-array expansion reads it (4: the '$' row, 0xFFFFFFFF) / r_bwt2nt
 *                                           (5: x = r_text_len + 1, which is no row)
 *   [10], [11] 0 */
int  salt_gpu_diag_occ(const salt_gpu_index_t *ix, int mode, uint32_t n, const uint32_t *queries, uint32_t *out);

/* Unit entry of k_pack (tests): the launch the align and text entries make, on the caller's device buffers; it needs no index.  d_seqs:
 * the reads' codes (0..3, 4 = N, above 4 read as N), at any byte alignment; d_offs: n_reads + 1 uint32 offsets into d_seqs.  With
 * nw8 = ceil(max_read_len / 8), nw16 = ceil(/ 16), nw32 = ceil(/ 32), read r gets
 *   d_pm[r * pm_stride ..], pm_stride = (2 nw8 + 1) rounded up to 4 words: one-hot nibble words, LSB first, N = 15, no base = 0:
 *       [0, nw8) forward, [nw8, 2 nw8) reverse complement, [2 nw8] = L (the read's length, at most 8 nw8: longer reads are truncated);
 *   d_tb[r * tb_stride ..], tb_stride = (2 nw16 + 2 nw32 + 1) rounded up to 4 words: 2-bit codes, first base in the high bits, N read as
 *       0: [0, nw16) forward, [nw16, 2 nw16) reverse complement; 'is N' flags, first base highest: [2 nw16, + nw32) forward, then nw32
 *       words reverse; then L.
 * Words between a record's L word and its stride are not written.  The launch is queued on hip_stream and not waited for. */
int  salt_gpu_diag_pack(int device, uint32_t n_reads, uint32_t max_read_len, const void *d_seqs, const void *d_offs,
                        void *d_pm, void *d_tb, void *hip_stream);

/* Unit entry of the text stage (tests): the FASTQ scan, k_pack's records and k_sam_len / k_sam_write or k_bam_len / k_bam_write, on result rows
 * of the caller's choosing.  It runs the stages of salt_gpu_align_se_text (pe == NULL: one block, fastq2 ignored) or salt_gpu_align_pe_text
 * (pe given: two blocks, row 2p + m belongs to mate m of pair p) through the same two functions -- the parse stage and the output stage --
 * with the align kernels between them replaced by k_pack and a copy of rows[0 .. n_rows) into the workspace's result rows.  Output as the
 * production entries give it: *out points into the workspace's page-locked buffer, salt_gpu_ws_set_sam_bam and salt_gpu_ws_set_sam_bgzf
 * are honoured, *n_records = the number of parsed records (both mates counted).  With salt_gpu_ws_set_polish or salt_gpu_ws_set_trim on: SALT_E_INVAL.
 * The rows are checked on the host before a kernel reads one, with the read lengths the parse kernels found; SALT_E_INVAL and a message
 * "text rows: ..." (the row is named) for:
 *   n_rows different from the number of parsed records; a read longer than SALT_MAX_READ_LEN;
 *   any row:       n_hits[0] + n_hits[1] > SALT_MAX_HITS, a hit_n_cigar of a listed hit > SALT_MAX_CIGAR_OPS, a listed hit's pos >= ref_len
 *                  (paired end prints XA for an unmapped mate too);
 *   a mapped row (pos != 0xFFFFFFFF; single end: and not skipped -- the paired-end kernels do not read `skipped`):
 *                  n_cigar > SALT_MAX_CIGAR_OPS, pos >= ref_len, pos + (sum of M and D) > ref_len, seq_start + (sum of M and I) > the read's
 *                  length, seq_end >= the read's length.
 * The tallies (SNP counts, depth, error profile, genotype, discover) do not see these rows. */
int  salt_gpu_diag_text_rows(salt_gpu_ws_t *ws, const salt_text_opt_t *topt, const salt_pe_opt_t *pe, const char *fastq1, uint64_t n1_bytes,
                             const char *fastq2, uint64_t n2_bytes, const salt_result_t *rows, uint32_t n_rows,
                             const char **out, uint64_t *out_bytes, uint32_t *n_records);

/* Work-queue counters of the LAST batch (diagnostics): [0] reads k_light handed to k_heavy, [2] reads whose gapped pass
 * was deferred, [5] k_gap items (32 candidates each), [6] k_cigar items, [7] k_cigar's queue head; [1] / [3] the longest R / C list among
 * the 64 segments of the seed walk queues; [4] reads the quarter-wave light kernel (k_light4: four reads a wave, for reads of at most 120
 * bases with at most 4 seed slots a strand) left to its retry launch because one of their seed lists has more than 16 rows; 0 when
 * another shape of the light pass ran. */
int  salt_gpu_ws_queue_counts(salt_gpu_ws_t *ws, uint32_t out[8]);

/* counters of the last batch(es) since the previous call; resets them */
int  salt_gpu_ws_counters(salt_gpu_ws_t *ws, uint64_t out[SALT_CTR_N]);

/* Unit access (tests): for each case c -- a read seqs[offs[c]..offs[c+1]) against the 4-bit mixRef
 * `ref_words` at pos[c] -- out4[4c+0] = masked Hamming distance capped at 3 (255 = more; -2 = window
 * past the end), out4[4c+1] = LV distance with bound kdiff[c] from the diagonal-per-lane kernel, out4[4c+2]
 * = the same from the candidate-per-lane kernel (-2 when kdiff/L are outside its range), out4[4c+3] =
 * number of CIGAR ops written to cigars[64c..] (-2 when there is no alignment).  Mirrors ed_mismatch,
 * ed_diff, ed_diff_withcigar (editdistance.c:88,174,234). */
int  salt_gpu_diag_lv(const uint32_t *ref_words, uint32_t ref_len, uint32_t n_cases, const uint32_t *pos,
                      const uint32_t *kdiff, const uint8_t *seqs, const uint32_t *offs, int32_t *out4, uint16_t *cigars);
/* The same with lv_cigar's tables placed as k_cigar places them when lds_tab != 0: in the block's LDS for a distance of at most 12,
 * in global memory above that.  lds_tab == 0 is salt_gpu_diag_lv. */
int  salt_gpu_diag_lv_tab(const uint32_t *ref_words, uint32_t ref_len, uint32_t n_cases, const uint32_t *pos,
                          const uint32_t *kdiff, const uint8_t *seqs, const uint32_t *offs, int32_t *out4, uint16_t *cigars, int lds_tab);

/* Unit entry of the Smith-Waterman mate-rescue kernel (ssw_init + ssw_align as snpaln_sw[_snpaware] call them,
 * alnpe.c:260-393; ssw.c): case i aligns codes[read_offs[i]..read_offs[i+1]) against reference symbols
 * ref_syms[ref_offs[i]..ref_offs[i+1]) -- 4-bit allele masks when aware[i], bases 0..3 otherwise.
 * out6[6i..]: score1, score2, ref_begin1, ref_end1, read_begin1, read_end1; cigars[i][SALT_MAX_CIGAR_OPS], n_cigar[i].
 * Cases whose CIGAR needs more than SALT_MAX_CIGAR_OPS operations (or a band beyond the build's) keep their six numbers, get
 * n_cigar 0, and make the call return SALT_E_CAPACITY after every row is written. */
int  salt_gpu_diag_ssw(uint32_t n_cases, const uint8_t *aware, const uint8_t *ref_syms, const uint32_t *ref_offs,
                       const uint8_t *codes, const uint32_t *read_offs, int32_t *out6, uint16_t *cigars, uint16_t *n_cigar);

/* ---- polish (row N4): the re-scoring step of the reference's SAM post-processor (Polish_src/polish.c:461-497 scores, 190-249 CIGAR) ---
 * For every item = (read, strand, offset into the 2-bit genome): the plain edit distance between the read (strand 1: its reverse
 * complement) and the `tlen` bases at `offset`, by stock Landau-Vishkin with bound k (computeEditDistance, Polish_src/lv.c; -1 = more than
 * k), and with want_cigar the CIGAR of computeEditDistanceWithCigar (useM; binary ops as in salt_result_t).  `pool`: explicit windows
 * (pool_stride code bytes each) for the few items whose window the reference clips at the genome end and pads with what its buffer
 * held before (polish.c:84-92); item.pool = 0xFFFFFFFF for everything else.  salt_amd/host/polish_main.cc is the caller. */
typedef struct { uint32_t read, offset, pool; uint16_t tlen; uint8_t strand, k; } salt_polish_item_t;
typedef struct salt_gpu_polish salt_gpu_polish_t;
int  salt_gpu_polish_open(int device, const uint8_t *pac, uint64_t l_pac, salt_gpu_polish_t **out);
void salt_gpu_polish_close(salt_gpu_polish_t *p);
int  salt_gpu_polish_lv(salt_gpu_polish_t *p, const uint8_t *codes, const uint32_t *offs, uint32_t n_reads, const salt_polish_item_t *items,
                        uint32_t n_items, const uint8_t *pool, uint32_t pool_stride, uint32_t n_pool, int want_cigar,
                        int32_t *dist, uint16_t *cigars, uint8_t *n_cigar);

/* polish -s: the same items by Smith-Waterman (ssw_init + ssw_align over polish's own matrix: +2 / -2, N 0, gaps 3 / 1; polish.c:48-52,
 * 209-222, 509-510).  score[i] = score1; with want_cigar also read_span[2i], [2i+1] = read_begin1, read_end1 (the soft clips) and the
 * banded traceback's CIGAR.  item.tlen is the (possibly clipped) window length; item.pool and item.k are not used. */
int  salt_gpu_polish_sw(salt_gpu_polish_t *p, const uint8_t *codes, const uint32_t *offs, uint32_t n_reads, const salt_polish_item_t *items,
                        uint32_t n_items, int want_cigar, int32_t *score, int32_t *read_span, uint16_t *cigars, uint16_t *n_cigar);

/* polish over text: SAM record lines in, polished record lines out -- what the reference's `polish` does between reading a record and
 * printing it (samParser.c:84-190; polish.c:448-816), for one block on the device: the strtok field rules, the XA items, contig names ->
 * genome offsets, the offset sort and rm_repeat_hits, the shrinking window, every score (k_polish, or Smith-Waterman under use_sw), the
 * winners, under `paired` the pairing walk and pair choice, the winners' CIGARs and the records of polish_sam_se / polish_sam_pe.
 * Needs the contig table (bntann1_t offset + name per sequence).
 * In:  sam[0 .. n_bytes), n_bytes < 2^31: whole record lines only (the header is the caller's); a last line without its newline is
 *      allowed; under `paired` an even number of records (a last record without its mate is dropped, polish.c:455-456).
 * Out: *out points into a page-locked buffer the handle owns, valid until the next call on it: the polished records in input order.
 *      An empty line ends the input as in the reference (samParser.c:87-90): the records before it are polished, *stopped = 1, nothing
 *      behind it is looked at.
 * Errors (SALT_E_INVAL, no records returned; salt_gpu_last_error() has the text): a record with fewer than 11 fields (its index in the
 * block is named), a contig that is not in the table (named), a read of more than SALT_MAX_READ_LEN bases, a hit beyond the genome
 * ("Out of reference length"), under use_sw an alignment beyond the build's band, a winner without an alignment within 13 edits.
 * Of several bad records the one reported is the smallest index the stage that found it refuses: a malformed record or an over-long
 * read (found while counting) is reported before an unknown contig or a hit beyond the genome in an earlier record (found while filling).
 * The handle keeps its device and page-locked buffers and grows them when a block needs more. */
int  salt_gpu_polish_set_contigs(salt_gpu_polish_t *p, int32_t n, const int64_t *offsets, const char *const *names);
typedef struct { int32_t paired, use_sw; } salt_polish_opt_t;              /* -p, -s */
int  salt_gpu_polish_text(salt_gpu_polish_t *p, const salt_polish_opt_t *opt, const char *sam, uint64_t n_bytes,
                          const char **out, uint64_t *out_bytes, uint32_t *n_records, int *stopped);
/* of the last call: records, hits parsed, unique hits scored, clipped windows, CIGAR items, proper pairs, output bytes, 0 */
int  salt_gpu_polish_text_stats(salt_gpu_polish_t *p, uint64_t out[8]);

/* ---- index construction on the device (salt-idx's heavy steps; row N1) ----------------------------------------------
 * Replaces, for texts of any length the 32-bit formats admit (n < 2^32 - 16): bwt_bwtgen / Rbwt_bwt_bwtgen (Index_src/bwt_gen.c,
 * 4bit_bwt_gen.c:1044-1130), bwt_bwtupdate_core (bwtmisc.c:121-143), bwt_cal_sa (bwt.c:48-68), LKT_build_lookuptable
 * (LookUpTable.c:70-150), Rbwt_gen_sa (rbwt.c:424-475).  Host buffers in and out; the suffix sorter (prefix doubling over a
 * radix sort) and every derived array run on `device`.  salt_amd/host/salt_idx.cc is the caller.
 *
 * salt_gpu_suffix_array: sa_out[0..n] = suffix array of text[0..n) with the empty suffix first (sa_out[0] = n); text holds one symbol
 *     per byte, values < 2^bits, bits = 2 or 3.
 * salt_gpu_idx_build_c: text = n base codes 0..3.  Writes the words of <P>.C.bwt behind its 5-word header (salt_gpu_idx_c_bwt_words(n)
 *     of them: 2-bit BWT with the interleaved Occ counts, bwt.h:57-64), primary and L2[0..4], the (n + sa_intv) / sa_intv suffix-array
 *     samples (sa[0] = 0xFFFFFFFF) and the 4^lkt_len + 1 items of the k-mer table.
 * salt_gpu_idx_build_r: rtext = n symbols 0..4 ('#' = 4) of the local-pattern text; sharp_off[j] = offset of the j-th '#', sharp_hdr[j]
 *     = header value of its record (localPattern.c:269-271, 304-307), cum4 = number of symbols < 4.  Writes inverseSa0, the
 *     code_words words of the 4-bit BWT (zero padded) and the n_sharp + 1 entries of saValueSharp (the last one is the caller's). */
int  salt_gpu_suffix_array(int device, const uint8_t *text, uint64_t n, int bits, uint32_t *sa_out);
uint64_t salt_gpu_idx_c_bwt_words(uint64_t n);
int  salt_gpu_idx_build_c(int device, const uint8_t *text, uint64_t n, uint32_t sa_intv, uint32_t *primary, uint32_t L2[5],
                          uint32_t *bwt, uint32_t *sa, uint32_t *lkt, uint32_t lkt_len);
int  salt_gpu_idx_build_r(int device, const uint8_t *rtext, uint64_t n, const uint32_t *sharp_off, const uint32_t *sharp_hdr, uint64_t n_sharp,
                          uint32_t cum4, uint32_t *inv_sa0, uint32_t *code, uint64_t code_words, uint32_t *rsa);
const char *salt_gpu_idx_last_error(void);

/* ---- SNP sites from a VCF, parsed on the device (`salt-idx --gpu --vcf`; the rule is DESIGN.md 2.2) -------------------
 * A handle holds the genome's bases, the contig names a CHROM may carry in a hash table, and one mask byte per genome position.
 * Text goes in as whole lines, in any number of calls and cut anywhere between lines; the result does not depend on the cuts or on the
 * order of the lines.  One thread parses one line as far as ALT (FILTER with pass_only) and ORs its allele mask into the position's byte;
 * finish compacts the non-zero bytes into per-contig site lists, what salt_idx_build_mem takes as salt_idx_snps_t.
 *   salt_gpu_vcf_open    seq[i]: the len[i] base LETTERS of contig i, as the FASTA holds them.  keys[k] (n_keys of them, NUL-terminated,
 *                        distinct) is a name a CHROM may carry and key_contig[k] the contig it means: the FASTA names after the rename
 *                        map.  Needs two bytes of device memory per genome position; SALT_E_NOMEM names the size.
 *   salt_gpu_vcf_add     n bytes of whole lines from a host buffer; only the last line of the last call may lack its '\n'.  The text is
 *                        cut at line ends into chunks of about opt.chunk_bytes (0: 16 MiB), and a longer line grows the chunk; the
 *                        copy of one chunk runs beside the parse of the one before.  Returns when the text has been copied out of `text`.
 *   salt_gpu_vcf_finish  waits for the parse, compacts, and gives the counters and (n_per_contig may be NULL) the sites of every contig.
 *                        A malformed line (fewer than 5 fields, POS not 1-10 digits) makes it return SALT_E_DATA; the message names the
 *                        smallest 1-based line number of such a line, counted over all calls of salt_gpu_vcf_add.
 *   salt_gpu_vcf_fetch   contig i's sites, ascending: 0-based positions, allele masks (bit A=0 C=1 G=2 T=3), reference codes; each array
 *                        holds n_per_contig[i] entries.  After finish only.
 * The host twin, which gives the same lists and counters, is declared in salt_host.h. */
typedef struct {
    uint64_t lines, kept, sites, unknown_contig, out_of_range, not_snv, ref_mismatch, filtered;
    uint64_t first_unknown_line;        /* 1-based line of the first CHROM that matched no contig; 0: none */
} salt_vcf_counters_t;
typedef struct { int32_t pass_only, reserved; uint64_t chunk_bytes; } salt_gpu_vcf_opt_t;
typedef struct salt_gpu_vcf salt_gpu_vcf_t;
int  salt_gpu_vcf_open(int device, int32_t n_contigs, const char *const *seq, const uint64_t *len, int32_t n_keys, const char *const *keys,
                       const int32_t *key_contig, const salt_gpu_vcf_opt_t *opt, salt_gpu_vcf_t **out);
int  salt_gpu_vcf_add(salt_gpu_vcf_t *h, const char *text, uint64_t n);
int  salt_gpu_vcf_finish(salt_gpu_vcf_t *h, salt_vcf_counters_t *counters, uint32_t *n_per_contig);
int  salt_gpu_vcf_fetch(salt_gpu_vcf_t *h, int32_t contig, uint32_t *pos, uint8_t *alleles, uint8_t *ref);
void salt_gpu_vcf_close(salt_gpu_vcf_t *h);

const char *salt_gpu_last_error(void);
uint32_t    salt_gpu_result_size(void);         /* sizeof(salt_result_t), for bindings */

#ifdef __cplusplus
}
#endif
#endif
