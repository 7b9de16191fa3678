/* include/salt_host.h -- C ABI of the host side that surrounds the GPU path: index-file loading
 * (the reference's on-disk formats are the surface) and SAM text formatting.
 *
 * Reference interfaces mirrored (paths under Align_src/):
 *   salt_index_load / _free      alnse_index_reload / alnse_index_destroy        indexio.c:23-60
 *   salt_index_host_view         the arrays of index_t                            indexio.h:26-33
 *   salt_sam_header              aln_samhead (without the dated @PG line)         sam.c:56-84
 *   salt_sam_se                  aln_samse + sam_add_xa + sam_add_md_nm           sam.c:87-328
 *   salt_sam_pe                  alnpe_sam                                        sam.c:331-457
 *   salt_lkt_build               LKT_build_lookuptable                            Index_src/LookUpTable.c:70-150
 */
#ifndef SALT_HOST_H
#define SALT_HOST_H
#include <stdint.h>
#include <stddef.h>
#include "salt_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct salt_index salt_index_t;

/* Loads <prefix>.R.seedLen, .C.bwt, .C.sa, .C.lkt, .C.pac, .C.ann, .C.amb, .R.backward.{bwt,occ,sa},
 * .ref.  If .C.lkt is absent and rebuild_lkt != 0 the table is rebuilt from .C.pac in memory.
 * Returns NULL on failure; salt_host_last_error() has the message (the reference would exit(1)). */
salt_index_t *salt_index_load(const char *prefix, int rebuild_lkt);
void          salt_index_free(salt_index_t *ix);
const salt_host_index_t *salt_index_host_view(const salt_index_t *ix);
int32_t       salt_index_seed_len(const salt_index_t *ix);
int32_t       salt_index_n_seqs(const salt_index_t *ix);
/* sequence i of <P>.C.ann (bntann1_t, bntseq.h): its offset in the concatenated genome, length and name -- what salt_gpu_index_set_contigs takes */
int           salt_index_seq(const salt_index_t *ix, int32_t i, int64_t *offset, int32_t *len, const char **name);
const uint8_t *salt_index_pac(const salt_index_t *ix, uint64_t *l_pac);   /* <P>.C.pac bytes (bntseq.c 2-bit packing) for salt_gpu_index_set_pac */
const char   *salt_host_last_error(void);

/* 12-mer table exactly as salt-idx writes it; out must hold 4^len + 1 entries. */
void salt_lkt_build(const uint8_t *pac, uint32_t l_ref, int len, uint32_t *out);

typedef struct {
    int32_t print_xa_cigar;     /* -c */
    int32_t print_nm_md;        /* -d */
    const char *rg_id;          /* -g, or NULL */
} salt_sam_opt_t;

/* Both return the number of bytes written (no trailing NUL counted), or -1 when cap is too small.
 * salt_sam_se writes one record without the newline; a skipped read (> 200 N) yields 0 bytes,
 * which the reference prints as an empty line (alnse.c:1328,1437). */
int salt_sam_header(const salt_index_t *ix, const salt_sam_opt_t *opt, char *buf, size_t cap);
int salt_sam_se(const salt_index_t *ix, const salt_sam_opt_t *opt, const char *name, const uint8_t *seq,
                int32_t l_seq, const char *qual, const salt_result_t *res, char *buf, size_t cap);

/* alnpe_sam (sam.c:331-457): both records of a pair (q[0], q[1]), each followed by "\n\n" as the reference's
 * driver prints them (alnpe.c:640-648).  Names are the mates' names with a trailing /1 /2 already removed. */
int salt_sam_pe(const salt_index_t *ix, const salt_sam_opt_t *opt, const salt_pe_opt_t *pe, const char *const name[2],
                const uint8_t *const seq[2], const int32_t l_seq[2], const char *const qual[2],
                const salt_result_t *q, char *buf, size_t cap);

/* BAM (SAM specification 4.2), the uncompressed bytes that `salt --bam` wraps in BGZF blocks.  Written from the format definition, without
 * any code of the device's record kernels (k_bam_len / k_bam_write): it is the model their bytes are compared with, and it encodes whatever
 * does not come from them (the host pipeline, the blocks behind a hand-over, a libsalt_gpu without salt_gpu_ws_set_sam_bam, SALT_BAM_HOST=1).
 *   salt_bam_header    "BAM\1", l_text, header_text as given (no NUL padding), n_ref and per sequence of the index l_name, name NUL, l_ref
 *   salt_bam_from_sam  one record per non-empty line of this program's own SAM records (no header lines), in order.  refID from RNAME
 *                      ('*': -1), pos = POS - 1, bin = reg2bin(pos, pos + reference length of the CIGAR, 1 without one), next_refID from
 *                      RNEXT ('=': refID), QUAL - 33; tags in the line's order: Z verbatim, integers in the smallest unsigned type that
 *                      holds them (C, S, I; c, s, i below zero), XV always as an array B:I of its comma-separated offsets.
 * Both return the bytes written, SALT_BAM_E_CAP when cap is too small (SALT_BAM_BOUND(n) always suffices for salt_bam_from_sam) or
 * SALT_BAM_E_INVAL with salt_host_last_error() set: a line that is no SAM record of this program, an RNAME the index does not hold, a read
 * name longer than SALT_BAM_MAX_NAME bytes (l_read_name is one byte and counts the NUL).  *n_records, when given: records written. */
#define SALT_BAM_MAX_NAME 254
#define SALT_BAM_E_INVAL (-1)
#define SALT_BAM_E_CAP   (-2)
#define SALT_BAM_BOUND(n_sam_bytes) (4 * (uint64_t)(n_sam_bytes) + 64)
int64_t salt_bam_header(const salt_index_t *ix, const char *header_text, size_t n_text, uint8_t *out, size_t cap);
int64_t salt_bam_from_sam(const salt_index_t *ix, const char *sam, size_t n, uint8_t *out, size_t cap, uint64_t *n_records);

/* Allele counts at the index's SNP sites (`salt --snp-counts`): the host twin of salt_gpu_index_snp_sites / _snp_counts, written from the
 * definition in salt_gpu.h without any code of the device's kernel.  It is the model the device counts are compared with, and what `salt`
 * counts with when its libsalt_gpu has no salt_gpu_index_snp_enable.
 *   salt_snp_sites      the genome positions (0-based, concatenated coordinate) whose mixRef mask lists two or more bases, ascending: the
 *                       first min(cap, n_sites) of them into pos (may be NULL); returns n_sites
 *   salt_snp_count_sam  counts[site][A C G T] += what the record lines of this program's own SAM text show at the sites: a record counts
 *                       iff FLAG bit 4 is clear and MAPQ >= min_mapq; global position = contig offset + POS - 1; M columns count where SEQ
 *                       holds A, C, G or T, I and S advance in SEQ, D on the genome.  Header lines ('@') and empty lines are skipped; any
 *                       other line that is no SAM record is an error.  n_sites must be the index's.  Returns the records that counted.
 * Both return -1 with salt_host_last_error() set on failure. */
int64_t salt_snp_sites(const salt_index_t *ix, uint32_t *pos, uint64_t cap);
int64_t salt_snp_count_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint32_t *counts, uint64_t n_sites);

/* Coverage (`salt --depth`): the host twins of the device's difference array and text kernels, written from the definition in salt_gpu.h
 * without any code of the kernels'.  They are the model the device is compared with, and what `salt` uses when its libsalt_gpu has no
 * salt_gpu_index_depth_enable.  diff is uint32[n_words], n_words = ref_len + 1 (anything else is an error).
 *   salt_depth_add_sam  diff += the M runs of the record lines of this program's own SAM text: a record counts iff FLAG bit 4 is clear and
 *                       MAPQ >= min_mapq; global position = contig offset + POS - 1; every M run [g, g + len) is cut at ref_len and, when
 *                       something is left, adds 1 at g and takes 1 at its end; D advances on the genome, I and S in the read.  Header
 *                       lines ('@') and empty lines are skipped; any other line that is no SAM record is an error, and nothing of that
 *                       line is added.  Returns the records that counted.
 *   salt_depth_text     the text of the array: window == 0 the per-base bedGraph (one line per maximal run of equal depth inside a contig),
 *                       else one line per window of `window` positions with the mean as h / 100 '.' h % 100.  Returns the bytes the text
 *                       takes; the first min(cap, that) of them are in out (out may be NULL with cap 0: the size only).
 * Both return -1 with salt_host_last_error() set on failure. */
int64_t salt_depth_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint32_t *diff, uint64_t n_words);
int64_t salt_depth_text(const salt_index_t *ix, const uint32_t *diff, uint64_t n_words, uint32_t window, char *out, uint64_t cap);

/* The error profile (`salt --error-profile`): the host twins of the device's k_errprof and the one printer of the file, written from the
 * definition in salt_gpu.h without any code of the kernel's.  cells is uint64[n_cells], n_cells = 2 x 512 x 95 x 4 x 4 = 1 556 480 (anything
 * else is an error), indexed [mate][cycle][q][ref][read]; rec is uint64[16], R[2][8] of salt_gpu.h.
 *   salt_errprof_add_sam  cells and rec += the base events of the record lines of this program's own SAM text: mate from FLAG 0x80, reverse
 *                         from 0x10, unmapped from 0x4; a record counts iff it is mapped and MAPQ >= min_mapq; global position = contig
 *                         offset + POS - 1; q = QUAL[s] as printed, minus 33 when the byte is in 33 .. 126, else 94; QUAL `*` gives 94
 *                         everywhere; SEQ letters are complemented back for reverse reads, cycle = L - 1 - s there.  Header lines ('@')
 *                         and empty lines are skipped; any other line that is no SAM record of at most 512 bases is an error, and nothing
 *                         of that line is added.  A skipped read prints as an empty line, so rec[1] and rec[9] ("skipped") stay 0 here and
 *                         "seen" does not count such reads: the device's seen - skipped is this function's seen.  Returns the records
 *                         that counted.
 *   salt_errprof_text     the bytes of the file: tab-separated, '\n' line ends; "#salt-error-profile v1 min_mapq=<n>", then the sections
 *                         R (per mate the seven counters), Q (mate, q 0 .. 93 then "none", bases, mismatches, empirical = -10 log10((mismatches
 *                         + 1) / (bases + 2)) as %.2f), C (mate, cycle from 1, bases, mismatches), S (mate, ref, read as letters, count: 16
 *                         rows a mate) and, with full != 0, E (mate, cycle, q, ref, read, count: the non-zero cells), each behind its '#'
 *                         header line and ascending in its keys.  Only mates with records seen are printed; Q and C rows without bases are
 *                         left out.  Returns the bytes the text takes; the first min(cap, that) of them are in out (out may be NULL with
 *                         cap 0: the size only).  Both paths of `salt` print through this function.
 * Both return -1 with salt_host_last_error() set on failure. */
int64_t salt_errprof_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint64_t *cells, uint64_t n_cells, uint64_t rec[16]);
int64_t salt_errprof_text(const uint64_t *cells, const uint64_t rec[16], uint32_t min_mapq, int full, char *out, uint64_t cap);

/* Genotypes at the SNP sites (`salt --genotype`): the host twins of the device's k_gt_add and of its call and text kernels, and the one
 * header of the file, written from the definition in salt_gpu.h; they share the penalty table (salt_gt_table.h) with the kernels and
 * nothing else.  sites is salt_gt_site_t[n_sites], n_sites = salt_snp_sites' count (anything else is an error).
 *   salt_gt_add_sam  sites += the events of the record lines of this program's own SAM text: a record counts iff it is mapped (FLAG 0x4
 *                    clear) and MAPQ >= min_mapq; global position = contig offset + POS - 1; an M column at a site whose SEQ letter is A, C, G
 *                    or T adds 1, M[q], X[q], H[q] to that letter's words, q = QUAL[s] as printed minus 33 when the byte is in 33 .. 126,
 *                    else SALT_GT_Q_NONE; QUAL `*` gives SALT_GT_Q_NONE everywhere.  Header lines ('@') and empty lines are skipped; any
 *                    other line that is no SAM record of this program's is an error; a line is checked whole before anything of it is added.
 *                    Returns the records that counted.
 *   salt_gt_text     the records of sites [first, first + n) of the index from sites[0 .. n): the call of salt_gpu.h and its VCF line, no
 *                    header.  Returns the bytes the text takes; the first min(cap, that) of them are in out (out may be NULL with cap 0:
 *                    the size only).  The model of the device's text, and what `salt` prints on the host path.
 *   salt_gt_header   the header of the file, one function for both paths: ##fileformat=VCFv4.2, ##source, one ##contig=<ID=,length=> per
 *                    sequence of <P>.C.ann, the INFO line, the five FORMAT lines, the #CHROM line ending in `sample` (NULL or empty:
 *                    "sample").  Sizes as salt_gt_text.
 * All return -1 with salt_host_last_error() set on failure. */
int64_t salt_gt_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, salt_gt_site_t *sites, uint64_t n_sites);
int64_t salt_gt_text(const salt_index_t *ix, const salt_gt_site_t *sites, uint64_t first, uint64_t n, char *out, uint64_t cap);
int64_t salt_gt_header(const salt_index_t *ix, const char *sample, char *out, uint64_t cap);
const uint32_t *salt_gt_table(void);      /* SALT_GT_TABLE as this library holds it: 94 x 3 words, for bindings */

/* SNP candidates off the index's sites (`salt --discover`): the host twins of the device's k_disc_add and of its flag and line kernels,
 * written from the definition in salt_gpu.h; they share nothing with the kernels.  alt is uint64[n_pos] and diff uint32[n_pos + 1],
 * n_pos = the index's ref_len (anything else is an error).
 *   salt_disc_add_sam  both arrays += the record lines of this program's own SAM text: a record counts iff it is mapped (FLAG 0x4 clear)
 *                      and MAPQ >= min_mapq; global position = contig offset + POS - 1; every M run, cut at ref_len, marks diff; an M
 *                      column whose SEQ letter is A, C, G or T and not in the position's mixRef mask (mask != 0) is an event, and adds
 *                      1 << 21 k (k: the letter's rank among the bases outside the mask) to alt iff QUAL[s] as printed minus 33 is
 *                      >= min_baseq or the byte is outside 33 .. 126; QUAL `*` passes everywhere.  Header lines ('@') and empty lines
 *                      are skipped; any other line that is no SAM record of this program's is an error; a line is checked whole before
 *                      anything of it is added.  Returns the records that counted.
 *   salt_disc_text     the candidate lines of the arrays: the call rule of salt_gpu.h and its line, no header; all_sites: also the
 *                      index's sites without a called base.  Returns the bytes the text takes; the first min(cap, that) of them are in
 *                      out (out may be NULL with cap 0: the size only).  seen, when given, has a byte per sequence of the index:
 *                      1 iff the sequence has a line.  The model of the device's text, and what `salt` prints on the host path.
 * Both return -1 with salt_host_last_error() set on failure. */
int64_t salt_disc_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint32_t min_baseq, uint64_t *alt, uint32_t *diff, uint64_t n_pos);
int64_t salt_disc_text(const salt_index_t *ix, const uint64_t *alt, const uint32_t *diff, uint64_t n_pos, uint32_t min_alt, uint32_t min_pct, int all_sites,
                       char *out, uint64_t cap, uint8_t *seen);

/* The run's summary (`salt --stats`): the host twin of the device's k_stats_add and the one printer of the file, written from the
 * definition in salt_gpu.h without any code of the kernel's.  cells is uint64[n_cells], n_cells = SALT_STATS_CELLS = 6 021, the fixed tables
 * at salt_gpu.h's offsets; ct is uint64[n_ct], n_ct = 8 x the index's sequences (anything else is an error for both).
 *   salt_stats_add_sam  the tables += the record lines of this program's own SAM text: mate from FLAG 0x80, reverse from 0x10, unmapped from
 *                       0x4, the pair's fields from 0x1, 0x2, 0x8 and 0x20, RNAME, POS, MAPQ, CIGAR (M I D S), RNEXT, PNEXT, TLEN, SEQ
 *                       (length and letters) and the entries of the XA tag.  Header lines ('@') and empty lines are skipped; any other
 *                       line that is no SAM record of this program's of at most 512 bases is an error, and a line is checked whole before
 *                       anything of it is added.  A skipped read prints as an empty line, so SN's "skipped" stays 0 here and "seen" does
 *                       not count such reads: the device's seen - skipped is this function's seen.  Returns the records that counted.
 *   salt_stats_text     the bytes of the file: tab-separated, '\n' line ends, one tag per line, integers only.
 *                         #salt-stats v1 min_mapq=<n> <a remark on ISQ>
 *                         SN mate key value     the 16 cells of SN under fixed keys (seen skipped unmapped low_mapq counted reverse gapped
 *                                               with_xa proper mate_unmapped mate_other_contig bases m_bases i_bases d_bases s_bases)
 *                         MQ mate mapq n, RL mate len n, GC mate pct n (pct "none": no A, C, G or T), XA mate k n: the non-zero cells
 *                         IS tlen n             the non-zero cells, the last bin as ">=4096"
 *                         ISQ pairs q25 q50 q75 mean   q: the smallest length at which the cumulative count reaches that share of the pairs
 *                                               (">=4096" in the last bin); mean: (100 sum + n / 2) / n as h / 100 '.' h % 100 over the bins
 *                                               below 4096; "." where there is nothing to divide by
 *                         OR inward outward tandem
 *                         ID len ins del        the lengths with an I or D op, the last as ">=64"
 *                         CT name length mapped0 mapped1 counted0 counted1 reverse mbases   every sequence, in index order
 *                       Mate 1's lines are printed only when mate 1 has seen records.  Returns the bytes the text takes; the first
 *                       min(cap, that) of them are in out (out may be NULL with cap 0: the size only).  Both paths of `salt` print
 *                       through this function.
 * Both return -1 with salt_host_last_error() set on failure. */
int64_t salt_stats_add_sam(const salt_index_t *ix, const char *sam, size_t n, uint32_t min_mapq, uint64_t *cells, uint64_t n_cells, uint64_t *ct, uint64_t n_ct);
int64_t salt_stats_text(const salt_index_t *ix, const uint64_t *cells, uint64_t n_cells, const uint64_t *ct, uint64_t n_ct, uint32_t min_mapq, char *out, uint64_t cap);

/* Indel candidates (`salt --indels`): the host twins of the device's k_indel_add and of its text kernels, written from the definition in
 * salt_gpu.h; they share nothing with the kernels.  A salt_indel_t holds what the device's table and counters hold: a sorted map from
 * allele key to value (forward observations low, reverse high) and the four counters tabled, dropped (always 0 here: a map has room),
 * long, unanchored.  diff is the tally's own uint32[n_pos + 1] difference array, n_pos = the index's ref_len (anything else is an error).
 *   salt_indel_add_sam  map, counters and diff += the record lines of this program's own SAM text: a record counts iff it is mapped
 *                       (FLAG 0x4 clear) and MAPQ >= min_mapq; global position = contig offset + POS - 1; reverse from FLAG 0x10; the ops
 *                       are those of the CIGAR without its S ops, whose lengths only advance in SEQ; every M run, cut at ref_len, marks
 *                       diff; every I and D op is an event, long or unanchored by the definition, and an event is left-shifted against the
 *                       index's 2-bit genome and added under its key.  Header lines ('@') and empty lines are skipped; any other line
 *                       that is no SAM record of this program's is an error; a line is checked whole before anything of it is added.
 *                       Returns the records that counted.
 *   salt_indel_entries  the map's (key, value) pairs with a non-zero value, in key order, uint64[2 n]: returns n; the first min(cap, n)
 *                       pairs are in out (out may be NULL with cap 0)
 *   salt_indel_stats    the four counters
 *   salt_indel_text     the VCF records of n (key, value) pairs in key order (a map's, or the device's salt_gpu_index_indel_fetch) and a
 *                       difference array: the call rule of salt_gpu.h and its line, no header; pairs out of order are an error, keys that
 *                       are not well-formed and values of 0 get no line.  Returns the bytes the text takes; the first min(cap, that) of
 *                       them are in out (out may be NULL with cap 0: the size only).  The model of the device's text, and what `salt`
 *                       prints on the host path.
 *   salt_indel_header   the header of the file, one function for both paths: ##fileformat=VCFv4.2, ##source, one ##contig=<ID=,length=>
 *                       per sequence of the index, the INFO definitions, ##salt_indels_parameters=<min_mapq=,min_alt=,min_pct=>,
 *                       ##salt_indels_dropped=N, the #CHROM line.
 * The int64_t functions return -1 with salt_host_last_error() set on failure. */
typedef struct salt_indel salt_indel_t;
salt_indel_t *salt_indel_new(void);
void    salt_indel_free(salt_indel_t *t);
int64_t salt_indel_add_sam(const salt_index_t *ix, salt_indel_t *t, const char *sam, size_t n, uint32_t min_mapq, uint32_t *diff, uint64_t n_pos);
int64_t salt_indel_entries(const salt_indel_t *t, uint64_t *out, uint64_t cap);
void    salt_indel_stats(const salt_indel_t *t, uint64_t out[4]);
int64_t salt_indel_text(const salt_index_t *ix, const uint64_t *entries, uint64_t n, const uint32_t *diff, uint64_t n_pos, uint32_t min_alt, uint32_t min_pct,
                        char *out, uint64_t cap);
int64_t salt_indel_header(const salt_index_t *ix, uint32_t min_mapq, uint32_t min_alt, uint32_t min_pct, uint64_t dropped, char *out, uint64_t cap);

/* Index builder (row N1): writes <prefix>.{R.seedLen,C.pac,C.ann,C.amb,C.lkt,C.bwt,C.sa,lp,
 * R.backward.bwt,R.backward.occ,R.backward.sa,ref} in salt-idx's formats from a FASTA (plain or .gz)
 * and salt's 4-column SNP file (chr, 1-based pos, alleles "A/G", ref; no header; grouped by
 * chromosome in FASTA order).  Mirrors index_main (Index_src/index1.c:46-185).  0 on success.
 *
 * The two suffix-array-bound steps go through a backend: NULL = SA-IS on the host (any machine; 64-bit indices beyond
 * 2^31 symbols), or the device builder of libsalt_gpu.so -- { device, salt_gpu_idx_build_c, salt_gpu_idx_build_r,
 * salt_gpu_idx_last_error } (include/salt_gpu.h) -- which is what indexes a GRCh38-sized genome in seconds.  Both give
 * the same bytes.  Nothing is chosen silently: the caller names the backend. */
typedef struct {
    int device;
    int (*build_c)(int device, const uint8_t *text, uint64_t n, uint32_t sa_intv, uint32_t *primary, uint32_t L2[5],
                   uint32_t *bwt, uint32_t *sa, uint32_t *lkt, uint32_t lkt_len);
    int (*build_r)(int device, const uint8_t *rtext, uint64_t n, const uint32_t *sharp_off, const uint32_t *sharp_hdr, uint64_t n_sharp,
                   uint32_t cum4, uint32_t *inv_sa0, uint32_t *code, uint64_t code_words, uint32_t *rsa);
    const char *(*last_error)(void);
} salt_idx_backend_t;
#define SALT_IDX_NO_LP 1            /* flags: do not write <prefix>.lp (the local patterns as text; `salt` never reads it) */
#define SALT_IDX_ALL_FILES 2        /* also write what the reference indexer writes and `salt` never reads: <prefix>.R.pac, .R.rpac, .R.ann, .R.amb,
                                       .R.forward.bwt / .occ / .sa (Index_src/index1.c:150-176): the directory then equals the reference's file for file */
int salt_idx_build(const char *fn_fa, const char *fn_snp, const char *prefix, int l_seed);
int salt_idx_build_ex(const char *fn_fa, const char *fn_snp, const char *prefix, int l_seed, const salt_idx_backend_t *backend, int flags);
/* The same from memory (what bench.py and the tests use for generated genomes): contigs as base letters (as a FASTA would hold
 * them), SNP groups in file order -- group i belongs to contig i, like the reference matches them (mixRef.c:149-152) --
 * with 0-based positions, allele masks (bit b = base b listed) and reference base codes. */
typedef struct { const char *name, *comment; const char *seq; uint64_t len; } salt_idx_contig_t;
typedef struct { const char *chr; const uint32_t *pos; const uint8_t *alleles; const uint8_t *ref; uint32_t n; } salt_idx_snps_t;
int salt_idx_build_mem(const salt_idx_contig_t *contigs, int n_contigs, const salt_idx_snps_t *snps, int n_groups, const char *prefix,
                       int l_seed, const salt_idx_backend_t *backend, int flags);
/* SNP sites straight from a VCF (`salt-idx --vcf`; the rule is DESIGN.md 2.2): per contig of the FASTA, in FASTA order, the ascending
 * 0-based positions of the sites with their allele masks and reference codes -- one salt_idx_snps_t per contig, by NAME, an empty group
 * for a contig without sites -- and the eight counters.  CHROM goes through the rename map (n_rename pairs: VCF name, FASTA name; a name
 * the map does not hold stays as it is) and is then compared byte for byte with the FASTA names.
 *   salt_vcf_snps       the whole text (plain, already inflated) in one call.  device == NULL: the host twin, plain C++ on one thread, which
 *                       compiles the same per-line function as the device's kernel (salt_amd/csrc/salt_vcf_line.h); else the entry
 *                       points of libsalt_gpu.so, where opt.chunk_bytes cuts the text into device chunks (0: the default).  NULL on
 *                       failure with salt_idx_last_error() set; a malformed line names its 1-based line number there.
 *   salt_vcf_counters / salt_vcf_group   the result; a group's arrays live as long as the handle, chr is the FASTA name
 *   salt_idx_build_vcf  salt_idx_build_ex with a VCF (plain, BGZF or gzip) in place of the SNP file: reads the FASTA once, ingests the VCF
 *                       in pieces cut at line ends, and goes on as salt_idx_build_mem does.  vcf_opts (may be NULL) also carries the
 *                       rename map's file, the SNP file to write beside the index, and where the counters and the first unknown CHROM go.
 * In the memory path a contig without sites keeps its place in the genome's coordinates: the local patterns of the contigs behind it
 * carry their own offsets (the file path keeps the reference's by-order behaviour, which tests/golden/index_cases/gap_short pins). */
typedef struct {
    int device;
    int  (*open)(int device, int32_t n_contigs, const char *const *seq, const uint64_t *len, int32_t n_keys, const char *const *keys,
                 const int32_t *key_contig, const salt_gpu_vcf_opt_t *opt, salt_gpu_vcf_t **out);
    int  (*add)(salt_gpu_vcf_t *h, const char *text, uint64_t n);
    int  (*finish)(salt_gpu_vcf_t *h, salt_vcf_counters_t *counters, uint32_t *n_per_contig);
    int  (*fetch)(salt_gpu_vcf_t *h, int32_t contig, uint32_t *pos, uint8_t *alleles, uint8_t *ref);
    void (*close)(salt_gpu_vcf_t *h);
    const char *(*last_error)(void);
} salt_vcf_device_t;                /* salt_gpu_vcf_open, _add, _finish, _fetch, _close and salt_gpu_last_error of libsalt_gpu.so */
typedef struct {
    int32_t pass_only;                              /* --vcf-pass-only */
    int32_t n_rename;
    const char *const *rename_from, *const *rename_to;
    uint64_t chunk_bytes;                           /* device ingest: bytes per chunk, 0 = the default */
    const salt_vcf_device_t *device;                /* NULL: the host twin */
    /* salt_idx_build_vcf only */
    const char *rename_file;                        /* --vcf-contigs: two TAB-separated columns, read in front of the pairs above; NULL: none */
    const char *snp_out;                            /* --snp-out: the sites as a four-column SNP file; NULL: none */
    salt_vcf_counters_t *counters;                  /* out, may be NULL */
    char *unknown_name; uint32_t unknown_name_cap;  /* out, may be NULL: the CHROM of line counters->first_unknown_line, cut to the room */
} salt_vcf_opt_t;
typedef struct salt_vcf salt_vcf_t;
salt_vcf_t *salt_vcf_snps(const salt_idx_contig_t *contigs, int n_contigs, const char *vcf, uint64_t n, const salt_vcf_opt_t *opt);
void salt_vcf_counters(const salt_vcf_t *v, salt_vcf_counters_t *out);
int  salt_vcf_group(const salt_vcf_t *v, int contig, salt_idx_snps_t *out);
void salt_vcf_free(salt_vcf_t *v);
int  salt_idx_build_vcf(const char *fn_fa, const char *fn_vcf, const char *prefix, int l_seed, const salt_idx_backend_t *backend, int flags,
                        const salt_vcf_opt_t *vcf_opts);
/* the host suffix sorter alone: sa_out[0..n] for text[0..n) of `bits`-bit symbols (2 or 3), empty suffix first */
int salt_idx_suffix_array_cpu(const uint8_t *text, uint64_t n, int bits, uint32_t *sa_out);
const char *salt_idx_last_error(void);

/* N3 -- insert-size window from the first batch of a paired-end run (`salt -p -b 0`; the reference prints "infer isize func haven't
 * been implemented" there and stops, Align_src/alnpe.c:586-589, so the definition is this build's; oracle/salt_oracle.c states it).
 * res: the 2 * n_pairs mates (pair i = rows 2i, 2i+1) aligned as SINGLE-END reads (salt_gpu_align_se).  A pair counts when both mates
 * map gap-free without alternative hits, on opposite strands of one sequence, forward mate first, template <= 100000; from the
 * sorted templates: quartiles, mean / sd inside [q1 - 2 iqr, q3 + 2 iqr] (integers, sd rounded up), window = mean -+ 4 sd widened
 * to [q1 - 3 iqr, q3 + 3 iqr].  Returns 0, or -1 when fewer than 25 pairs count (*n_used tells how many did). */
int salt_isize_infer(const salt_index_t *ix, uint32_t n_pairs, const uint32_t *offs, const salt_result_t *res,
                     uint32_t *min_tlen, uint32_t *max_tlen, uint32_t *n_used);

/* Trimming (`salt --trim-*`): the host twins of the device's k_fq_trim.  They compile the rule's one definition, csrc/salt_trim_rule.h, which the
 * kernel compiles too (salt_gpu.h states the rule and the options); the independent statement is the Python model of the tests.  They are what
 * the device is compared with, what `salt` trims with wherever its host pipeline parses the reads, and what gives a user the trimmed reads.
 *   salt_trim_span    one read: seq and qual are its len >= 1 letters and quality bytes, mate 0 or 1 -> *beg, *end, its span; counts: NULL,
 *                     or uint64[16] to which the read's counters are added at the mate's eight.  Returns 0.
 *   salt_trim_fastq   a block of whole 4-line FASTQ records (LF or CR LF), every record as mate `mate` -> the same records trimmed, LF line
 *                     ends, the header and '+' lines as they were: the block that, aligned without trimming, gives what the untrimmed block
 *                     gives with it.  Returns the bytes of the trimmed block (never more than n); they are written when out holds them.
 * Both return -1 with salt_host_last_error() set on failure: an option out of range (the message names the field), a block that is not
 * 4-line FASTQ. */
int     salt_trim_span(const salt_trim_opt_t *opt, int mate, const char *seq, const char *qual, uint32_t len, uint32_t *beg, uint32_t *end, uint64_t *counts);
int64_t salt_trim_fastq(const salt_trim_opt_t *opt, int mate, const char *in, uint64_t n, char *out, uint64_t cap, uint64_t *counts);
/* The pair forms (`salt --trim-pair-overlap`; salt_gpu.h states step 2p): the host twins of k_fq_trim_pair, compiled from the header's
 * one-thread trim_pair_span.  opt and pair: NULL or all zero = that part of the rule is off.
 *   salt_trim_pair_span    one pair -> span[4] = b1, e1, b2, e2; counts: NULL or uint64[16]; pair_counts: NULL or uint64[8].  Returns 0.
 *   salt_trim_fastq_pair   two blocks of whole 4-line FASTQ records, as many in each -> the two trimmed blocks (as salt_trim_fastq writes
 *                          them); *w1 and *w2 = their bytes, written when out1 / out2 hold them (never more than n1 / n2).  Returns 0. */
int salt_trim_pair_span(const salt_trim_opt_t *opt, const salt_trim_pair_opt_t *pair, const char *seq1, const char *qual1, uint32_t len1,
                        const char *seq2, const char *qual2, uint32_t len2, uint32_t span[4], uint64_t *counts, uint64_t *pair_counts);
int salt_trim_fastq_pair(const salt_trim_opt_t *opt, const salt_trim_pair_opt_t *pair, const char *in1, uint64_t n1, const char *in2, uint64_t n2,
                         char *out1, uint64_t cap1, uint64_t *w1, char *out2, uint64_t cap2, uint64_t *w2, uint64_t *counts, uint64_t *pair_counts);

/* "<len><op>..." text of a binary CIGAR (ops as in salt_result_t); returns bytes written or -1 */
int salt_cigar_text(const uint16_t *ops, int n_ops, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
