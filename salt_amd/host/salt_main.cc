// salt_amd/host/salt_main.cc -- `salt [opts] <idx-prefix> <reads.fq[.gz]>`: the reference's command line
// (Align_src/aln.c:102-227), index files and SAM stream, with the per-batch work on the GPU(s).
//
// It is the batch driver of alnse_core (Align_src/alnse.c:1353-1480) re-done for a device:
//   reader thread : FASTQ(.gz) -> batches of N_SEQS = 100000 reads          (query_read_multiSeqs, aln.h:27)
//   one worker per GPU : salt_gpu_align_se on its batch                     (stands where alnse_core1 ran)
//   formatter threads (-t) : SAM text per read                              (aln_samse, sam.c:87-182)
//   writer : records in input order                                         (the puts() loop, alnse.c:1433-1439)
// Extra long options (not in the reference): --gpus N (default 1); --bgzf: everything written to stdout is one BGZF stream (blocked gzip,
// htslib's .sam.gz container), the SAM blocks deflated on the device before they cross to the host; --bam: the stream is a BAM file -- the same
// container around binary records (SAM spec 4.2), which the device writes in place of the SAM text.
// --polish[=lv|sw]: stdout carries the records the reference's second program, `polish` (Polish_src/polish.c), prints for this run's SAM
// lines -- every reported hit re-scored against the plain genome by Landau-Vishkin (lv, polish's default) or Smith-Waterman (sw, polish -s)
// -- and no SAM text exists in between: on the text path the hits go from the result rows into the polish kernels
// (salt_gpu_ws_set_polish); the host pipeline formats a batch's lines, drops the empty ones and passes the rest through
// salt_gpu_polish_text.  No header (`polish` prints none).  A skipped read (more than 200 N) gives no record, a pair with a skipped mate
// none for either mate.  -c -d -g change nothing in this output.  Not with --bam.
// Flags the reference parses but ignores stay ignored (-n -e -M -O -E -l -X).  -p <mate1> <mate2>: paired end
// (alnpe_core, Align_src/alnpe.c:530-661) through salt_gpu_align_pe.
#include "../../include/salt_host.h"
#include <fcntl.h>
#include <getopt.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cerrno>
#include <ctime>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// Taken weakly: `salt` also links and runs against a libsalt_gpu without the device compressor (an older build, the tests' stub), and
// --bgzf then deflates on the host.
extern "C" int salt_gpu_ws_set_sam_bgzf(salt_gpu_ws_t *ws, int on) __attribute__((weak));
// Likewise the device's BAM record kernels: without them --bam encodes the records on the host, from the SAM text (salt_bam_from_sam).
extern "C" int salt_gpu_ws_set_sam_bam(salt_gpu_ws_t *ws, int on) __attribute__((weak));
// Blocked gzip input inflated on the device: the same way, and only with SALT_INFLATE_DEVICE=1 -- one decoding lane per CU is slower than the
// workers' zlib threads ("BGZF input").  Without all three, without the variable or with SALT_INFLATE_HOST=1 the workers inflate with zlib.
extern "C" int salt_gpu_ws_inflate_bgzf(salt_gpu_ws_t *ws, const void *blocks, uint64_t n_cbytes, uint32_t n_blocks, const uint32_t *c_off, const uint32_t *u_off) __attribute__((weak));
extern "C" int salt_gpu_ws_text_peek(salt_gpu_ws_t *ws, uint64_t off, uint64_t n, void *dst) __attribute__((weak));
extern "C" int salt_gpu_align_se_text_dev(salt_gpu_ws_t *ws, const salt_aln_opt_t *opt, const salt_text_opt_t *topt, uint64_t off, uint64_t n_bytes, int add_newline,
                                          const char **sam, uint64_t *sam_bytes, uint32_t *n_reads) __attribute__((weak));

// Likewise the trim kernel in front of the aligner (--trim-*): without it the run trims on the host, through the host pipeline.
extern "C" int salt_gpu_ws_set_trim(salt_gpu_ws_t *ws, const salt_trim_opt_t *opt) __attribute__((weak));
extern "C" int salt_gpu_ws_trim_counts(salt_gpu_ws_t *ws, uint64_t out[16], int reset) __attribute__((weak));
extern "C" int salt_gpu_ws_trim_uncount(salt_gpu_ws_t *ws) __attribute__((weak));
// And the pair rule's kernel (--trim-pair-overlap): without it the run finds the overlaps on the host, through the host pipeline.
extern "C" int salt_gpu_ws_set_trim_pair(salt_gpu_ws_t *ws, const salt_trim_pair_opt_t *opt) __attribute__((weak));
extern "C" int salt_gpu_ws_trim_pair_counts(salt_gpu_ws_t *ws, uint64_t out[8], int reset) __attribute__((weak));
// Likewise the polish stage behind the aligner (--polish) and the polish handle the host pipeline passes its lines through.
extern "C" int salt_gpu_ws_set_polish(salt_gpu_ws_t *ws, int mode) __attribute__((weak));
extern "C" int salt_gpu_polish_open(int device, const uint8_t *pac, uint64_t l_pac, salt_gpu_polish_t **out) __attribute__((weak));
extern "C" void salt_gpu_polish_close(salt_gpu_polish_t *p) __attribute__((weak));
extern "C" int salt_gpu_polish_set_contigs(salt_gpu_polish_t *p, int32_t n, const int64_t *offsets, const char *const *names) __attribute__((weak));
extern "C" int salt_gpu_polish_text(salt_gpu_polish_t *p, const salt_polish_opt_t *opt, const char *sam, uint64_t n_bytes,
                                    const char **out, uint64_t *out_bytes, uint32_t *n_records, int *stopped) __attribute__((weak));

// Likewise the allele counts at the SNP sites (--snp-counts): without the device's table and kernel the counts come from the SAM lines,
// through the host twin (salt_snp_count_sam).
extern "C" int salt_gpu_index_snp_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq) __attribute__((weak));
extern "C" int salt_gpu_index_snp_sites(salt_gpu_index_t *ix, uint32_t *n_sites, uint32_t *pos, uint64_t cap) __attribute__((weak));
extern "C" int salt_gpu_index_snp_counts(salt_gpu_index_t *ix, uint32_t *counts, uint64_t cap_words, int reset) __attribute__((weak));
extern "C" int salt_gpu_ws_snp_uncount(salt_gpu_ws_t *ws) __attribute__((weak));

// And the coverage (--depth): without the device's difference array and text kernels it is summed from the SAM lines and printed by the
// host twins (salt_depth_add_sam, salt_depth_text).
extern "C" int salt_gpu_index_depth_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq) __attribute__((weak));
extern "C" int salt_gpu_index_depth_fetch(salt_gpu_index_t *ix, uint64_t first, uint64_t n, uint32_t *out) __attribute__((weak));
extern "C" int salt_gpu_index_depth_add(salt_gpu_index_t *ix, uint64_t first, uint64_t n, const uint32_t *in) __attribute__((weak));
extern "C" int salt_gpu_index_depth_text_begin(salt_gpu_index_t *ix, const salt_depth_text_opt_t *opt) __attribute__((weak));
extern "C" int salt_gpu_index_depth_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes) __attribute__((weak));
extern "C" int salt_gpu_ws_depth_uncount(salt_gpu_ws_t *ws) __attribute__((weak));

// And the error profile (--error-profile): without the device's tables and kernel it is summed from the SAM lines by the host twin
// (salt_errprof_add_sam); the file is printed by salt_errprof_text either way.
extern "C" int salt_gpu_index_errprof_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq) __attribute__((weak));
extern "C" int salt_gpu_index_errprof_fetch(salt_gpu_index_t *ix, uint64_t *cells, uint64_t cap_cells, uint64_t rec[16], int reset) __attribute__((weak));
extern "C" int salt_gpu_ws_errprof_uncount(salt_gpu_ws_t *ws) __attribute__((weak));
extern "C" int salt_gpu_ws_set_quals(salt_gpu_ws_t *ws, const uint8_t *quals, int on_device) __attribute__((weak));
// Likewise the genotypes at the SNP sites (--genotype): without the device's sums and call kernels the sums come from the SAM lines
// (salt_gt_add_sam) and the records from the host twin's printer (salt_gt_text); the header is salt_gt_header's either way.
extern "C" int salt_gpu_index_gt_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq) __attribute__((weak));
extern "C" int salt_gpu_index_gt_fetch(salt_gpu_index_t *ix, uint64_t first_site, uint64_t n, salt_gt_site_t *out) __attribute__((weak));
extern "C" int salt_gpu_index_gt_add(salt_gpu_index_t *ix, uint64_t first_site, uint64_t n, const salt_gt_site_t *in) __attribute__((weak));
extern "C" int salt_gpu_index_gt_text_begin(salt_gpu_index_t *ix, const salt_gt_text_opt_t *opt) __attribute__((weak));
extern "C" int salt_gpu_index_gt_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes) __attribute__((weak));
extern "C" int salt_gpu_ws_gt_uncount(salt_gpu_ws_t *ws) __attribute__((weak));
// Likewise the SNP candidates off the sites (--discover): without the device's arrays and text kernels the arrays come from the SAM lines
// (salt_disc_add_sam) and the lines from the host twin's printer (salt_disc_text).
extern "C" int salt_gpu_index_disc_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq, uint32_t min_baseq) __attribute__((weak));
extern "C" int salt_gpu_index_disc_fetch(salt_gpu_index_t *ix, int which, uint64_t first, uint64_t n, void *out) __attribute__((weak));
extern "C" int salt_gpu_index_disc_add(salt_gpu_index_t *ix, int which, uint64_t first, uint64_t n, const void *in) __attribute__((weak));
extern "C" int salt_gpu_index_disc_text_begin(salt_gpu_index_t *ix, const salt_disc_text_opt_t *opt) __attribute__((weak));
extern "C" int salt_gpu_index_disc_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes) __attribute__((weak));
extern "C" int salt_gpu_index_disc_text_seen(salt_gpu_index_t *ix, uint8_t *seen, uint64_t cap) __attribute__((weak));
extern "C" int salt_gpu_ws_disc_uncount(salt_gpu_ws_t *ws) __attribute__((weak));
// Likewise the run's summary (--stats): without the device's tables and kernel it is summed from the SAM lines by the host twin
// (salt_stats_add_sam); the file is printed by salt_stats_text either way.
extern "C" int salt_gpu_index_stats_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq) __attribute__((weak));
extern "C" int salt_gpu_index_stats_fetch(salt_gpu_index_t *ix, uint64_t *cells, uint64_t cap_cells, uint64_t *ct, uint64_t cap_ct, int reset) __attribute__((weak));
extern "C" int salt_gpu_ws_stats_uncount(salt_gpu_ws_t *ws) __attribute__((weak));
// Likewise the indel candidates (--indels): without the device's table and text kernels the map comes from the SAM lines
// (salt_indel_add_sam) and the records from the host twin's printer (salt_indel_text).
extern "C" int salt_gpu_index_indel_enable(salt_gpu_index_t *ix, int on, uint32_t min_mapq, uint32_t log2_slots) __attribute__((weak));
extern "C" int salt_gpu_index_indel_stats(salt_gpu_index_t *ix, uint64_t out[4]) __attribute__((weak));
extern "C" int salt_gpu_index_indel_fetch(salt_gpu_index_t *ix, uint64_t cap, uint64_t *entries, uint64_t *n) __attribute__((weak));
extern "C" int salt_gpu_index_indel_add(salt_gpu_index_t *ix, const uint64_t *entries, uint64_t n) __attribute__((weak));
extern "C" int salt_gpu_index_indel_fetch_diff(salt_gpu_index_t *ix, uint64_t first, uint64_t n, uint32_t *out) __attribute__((weak));
extern "C" int salt_gpu_index_indel_add_diff(salt_gpu_index_t *ix, uint64_t first, uint64_t n, const uint32_t *in) __attribute__((weak));
extern "C" int salt_gpu_index_indel_text_begin(salt_gpu_index_t *ix, const salt_indel_text_opt_t *opt) __attribute__((weak));
extern "C" int salt_gpu_index_indel_text_next(salt_gpu_index_t *ix, const char **data, uint64_t *n_bytes) __attribute__((weak));
extern "C" int salt_gpu_ws_indel_uncount(salt_gpu_ws_t *ws) __attribute__((weak));

namespace {

const int N_SEQS = 100000;
int g_polish = 0;                             // --polish: 0 off, 1 Landau-Vishkin, 2 Smith-Waterman

// --trim-*: the reads are trimmed in front of the aligner -- on the text path by the device's k_fq_trim (salt_gpu_ws_set_trim on every
// workspace), wherever the host parses the reads (parse_batch: the host pipeline, the continuation behind a hand-over, the first batch of
// infer_isize) by the host twin salt_trim_span, which compiles the same rule.  The sixteen counters of both sides end in one line on stderr.
// With --trim-pair-overlap the pairs go through k_fq_trim_pair there and salt_trim_pair_span here (parse_batch_pe); a second line follows.
struct TrimRun {
    bool on = false, device = false;                         // device: the text path's workspaces trim
    bool instead_of_text_path = false;                       // the host pipeline reads a file the text path would have read: records of any shape, as behind a hand-over
    salt_trim_opt_t opt{}; bool has_overlap = false, has_error = false;
    std::atomic<uint64_t> counts[16]; std::atomic<bool> by_device{ false }, by_host{ false };
    void add(const uint64_t *c, bool dev) { bool any = false; for (int k = 0; k < 16; ++k) if (c[k]) { counts[k] += c[k]; any = true; } if (any) (dev ? by_device : by_host) = true; }
    // --trim-pair-overlap: step 2p of the rule, for pairs (k_fq_trim_pair on the text path, salt_trim_pair_span in parse_batch_pe); `on` stays
    // the per-read steps' switch, any() says whether the run trims at all; eight counters of their own, a second line on stderr
    bool pair_on = false, has_pair_overlap = false, has_pair_error = false; salt_trim_pair_opt_t pair_opt{};
    std::atomic<uint64_t> pair_counts[8];
    bool any() const { return on || pair_on; }
    void add_pairs(const uint64_t *c, bool dev) { bool some = false; for (int k = 0; k < 8; ++k) if (c[k]) { pair_counts[k] += c[k]; some = true; } if (some) (dev ? by_device : by_host) = true; }
} g_trim;
// a workspace of the text path is about to go: its counters join the run's
void trim_collect(salt_gpu_ws_t *ws)
{
    uint64_t c[16];
    if (ws && g_trim.device && salt_gpu_ws_trim_counts(ws, c, 1) == 0) g_trim.add(c, true);
    if (ws && g_trim.device && g_trim.pair_on && salt_gpu_ws_trim_pair_counts(ws, c, 1) == 0) g_trim.add_pairs(c, true);
}
void trim_report()
{
    if (!g_trim.any()) return;
    const bool clip = g_trim.opt.front || g_trim.opt.tail;
    std::string line = std::string("[salt] trim: ") + (g_trim.by_device && g_trim.by_host ? "device, and host behind the hand-over" : g_trim.by_host || !g_trim.device ? "host" : "device");
    for (int m = 0; m < 2; ++m) {
        uint64_t c[8]; for (int k = 0; k < 8; ++k) c[k] = g_trim.counts[8 * m + k];
        if (m && !c[0]) break;
        char buf[400];
        snprintf(buf, sizeof buf, "%s mate %d: reads %llu bases_in %llu bases_out %llu reads_clipped %llu reads_qual %llu bases_qual %llu reads_adapter %llu bases_adapter %llu reads_floored %llu",
                 m ? ";" : ":", m + 1, (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)(clip ? c[0] : 0), (unsigned long long)c[3],
                 (unsigned long long)c[4], (unsigned long long)c[5], (unsigned long long)c[6], (unsigned long long)c[7]);
        line += buf;
    }
    fprintf(stderr, "%s\n", line.c_str());
    if (!g_trim.pair_on) return;
    uint64_t c[8]; for (int k = 0; k < 8; ++k) c[k] = g_trim.pair_counts[k];
    fprintf(stderr, "[salt] trim: pairs: pairs %llu overlapping %llu trimmed %llu mate 1: reads %llu bases %llu mate 2: reads %llu bases %llu skipped_long %llu\n",
            (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5],
            (unsigned long long)c[6], (unsigned long long)c[7]);
}

struct Batch {
    long seq_no = 0;
    std::vector<char> raw;                    // the FASTQ text; names and qualities are NUL-terminated in place
    std::vector<uint32_t> rec;                // offset of every record's '@' line in raw (found by the reader)
    std::vector<uint32_t> name, qual;         // offsets into raw
    std::vector<uint8_t> seqs;
    std::vector<uint32_t> offs{ 0 };
    std::vector<salt_result_t> res;
    std::vector<std::string> sam;                    // the batch's SAM text in order, one piece per formatting thread
    std::unique_ptr<Batch> mate;              // -p: the second file's records of the same pairs
    int n() const { return (int)name.size(); }
};

inline uint8_t nt4(int c)
{
    switch (c) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                 case 'T': case 't': return 3; default: return 4; }
}

// True when every complete record in the first 256 KiB of the (possibly gzipped) file is strict 4-line FASTQ:
// '@' line, one sequence line, '+' line, one quality line of the same length.
static bool sniff_four_line(const char *fn)
{
    gzFile f = gzopen(fn, "r");
    if (!f) return true;
    std::vector<char> b(256u << 10);
    int n = gzread(f, b.data(), (unsigned)b.size());
    gzclose(f);
    if (n <= 0) return true;
    size_t p = 0; const size_t e = (size_t)n;
    if (b[0] != '@') return false;
    for (;;) {
        size_t st[5]; st[0] = p; bool whole = true;
        for (int k = 0; k < 4; ++k) {
            const char *nl = (const char *)memchr(b.data() + st[k], '\n', e - st[k]);
            if (!nl) { whole = false; break; }
            st[k + 1] = (size_t)(nl - b.data()) + 1;
        }
        if (!whole) return true;
        auto len = [&](int k) { size_t l = st[k + 1] - st[k] - 1; while (l > 0 && b[st[k] + l - 1] == '\r') --l; return l; };
        if (b[st[0]] != '@' || b[st[2]] != '+' || len(1) != len(3)) return false;
        p = st[4];
        if (p >= e) return true;
    }
}

// Raw text of up to N_SEQS FASTQ records.  The reader thread only finds record boundaries (4 lines per
// record, like the 4-line FASTQ the reference's test data uses); parsing runs on the worker threads.
// The general mode (chosen when the head of the file is not strict 4-line FASTQ, sniff_four_line) reads records the way
// the reference's kseq.h does -- sequence and quality may span lines -- and hands them on re-written as 4 lines.
struct RawReader {
    gzFile fp; std::vector<char> buf; size_t have = 0, pos = 0; bool eof = false; bool general = false;
    explicit RawReader(gzFile f, bool general_ = false) : fp(f), buf(8u << 20), general(general_) {}
    // kseq_read (kseq.h): '@name comment' line; sequence lines up to a line starting with '+'; that line; quality lines
    // until as many characters as the sequence has.  A '>' record (FASTA) has no quality: the reference cannot print it.
    int take_general(std::vector<char> &out, int n_rec, std::vector<uint32_t> &rec)
    {
        int got = 0;
        rec.clear();
        std::string line, seq, qual;
        auto getline = [&](std::string &l) -> bool {
            l.clear();
            int c;
            while ((c = gzgetc(fp)) != -1 && c != '\n') l.push_back((char)c);
            if (c == -1 && l.empty()) return false;
            while (!l.empty() && l.back() == '\r') l.pop_back();
            return true;
        };
        while (got < n_rec) {
            int c;
            while ((c = gzgetc(fp)) != -1 && c != '@' && c != '>') {}          // to the next header, as kseq does
            if (c == -1) { eof = true; break; }
            if (c == '>') { fprintf(stderr, "[salt] FASTA input has no base qualities: the reference cannot print SAM for it either\n"); exit(1); }
            if (!getline(line)) { eof = true; break; }
            const std::string head = line;
            seq.clear(); qual.clear();
            bool plus = false;
            for (;;) {
                c = gzgetc(fp);
                if (c == -1) break;
                if (c == '+') { getline(line); plus = true; break; }
                if (c == '>' || c == '@') { gzungetc(c, fp); break; }
                gzungetc(c, fp);
                if (!getline(line)) break;
                for (char ch : line) if (!isspace((unsigned char)ch)) seq.push_back(ch);
            }
            if (!plus) { fprintf(stderr, "[salt] record '%s' has no quality line\n", head.c_str()); exit(1); }
            while (qual.size() < seq.size() && getline(line)) for (char ch : line) if (!isspace((unsigned char)ch)) qual.push_back(ch);
            if (qual.size() != seq.size()) { fprintf(stderr, "[salt] record '%s': %zu bases but %zu qualities\n", head.c_str(), seq.size(), qual.size()); exit(1); }
            rec.push_back((uint32_t)out.size());
            out.push_back('@'); out.insert(out.end(), head.begin(), head.end()); out.push_back('\n');
            out.insert(out.end(), seq.begin(), seq.end()); out.push_back('\n');
            out.push_back('+'); out.push_back('\n');
            out.insert(out.end(), qual.begin(), qual.end()); out.push_back('\n');
            ++got;
        }
        return got;
    }
    bool fill()
    {
        if (eof) return false;
        if (pos > 0) { memmove(buf.data(), buf.data() + pos, have - pos); have -= pos; pos = 0; }
        if (have == buf.size()) buf.resize(buf.size() * 2);
        int n = gzread(fp, buf.data() + have, (unsigned)(buf.size() - have));
        if (n <= 0) { eof = true; return false; }
        have += (size_t)n;
        return true;
    }
    // appends whole records to out until n_rec records or end of file; returns records appended
    int take(std::vector<char> &out, int n_rec, std::vector<uint32_t> &rec)
    {
        if (general) return take_general(out, n_rec, rec);
        int got = 0;
        rec.clear();
        for (;;) {
            size_t scan = pos; int lines = 0; size_t rec_end = pos, rec_start = pos;
            while (got < n_rec) {
                const char *nl = (const char *)memchr(buf.data() + scan, '\n', have - scan);
                if (!nl) break;
                if (lines == 0) rec_start = scan;
                scan = (size_t)(nl - buf.data()) + 1;
                if (++lines == 4) { lines = 0; ++got; rec_end = scan; rec.push_back((uint32_t)(out.size() + (rec_start - pos))); }
            }
            out.insert(out.end(), buf.begin() + (long)pos, buf.begin() + (long)rec_end);
            pos = rec_end;
            if (got >= n_rec) return got;
            if (!fill()) {                                  // end of file: a last record without trailing newline
                if (have > pos) {
                    int nl = 0; for (size_t i = pos; i < have; ++i) nl += buf[i] == '\n';
                    if (nl >= 3) { rec.push_back((uint32_t)out.size()); out.insert(out.end(), buf.begin() + (long)pos, buf.begin() + (long)have); out.push_back('\n'); ++got; }
                    pos = have;
                }
                return got;
            }
        }
    }
};

// Helper threads of one align worker, created once (a batch needs three parallel loops; spawning threads for each costs more
// than the loops' bodies at 100 000 reads per batch).
class Pool {
    std::vector<std::thread> th;
    std::mutex mu; std::condition_variable cv_go, cv_done;
    std::function<void(int)> fn; int n_tasks = 0, next = 0, pending = 0; long gen = 0; bool stop = false;
    void run() {
        long seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu);
            cv_go.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            while (next < n_tasks) { int t = next++; lk.unlock(); fn(t); lk.lock(); if (--pending == 0) cv_done.notify_all(); }
        }
    }
public:
    const int n;
    explicit Pool(int n_threads) : n(n_threads < 1 ? 1 : n_threads) { for (int i = 1; i < n; ++i) th.emplace_back([this] { run(); }); }
    ~Pool() { { std::unique_lock<std::mutex> lk(mu); stop = true; } cv_go.notify_all(); for (auto &t : th) t.join(); }
    // fn(t) for t in [0, n): the calling thread takes part
    void parallel(const std::function<void(int)> &f) {
        if (n == 1) { f(0); return; }
        std::unique_lock<std::mutex> lk(mu);
        fn = f; n_tasks = n; next = 0; pending = n; ++gen;
        cv_go.notify_all();
        while (next < n_tasks) { int t = next++; lk.unlock(); fn(t); lk.lock(); --pending; }
        cv_done.wait(lk, [&] { return pending == 0; });
    }
};

void parse_batch(std::vector<char> &raw, Batch &b, Pool &pool, int mate = 0, bool count = true);
void parse_batch_pe(Batch &b1, Batch &b2, Pool &pool, bool count = true);

void format_batch(const salt_index_t *ix, const salt_sam_opt_t *so, Batch &b, Pool &pool)
{
    const int n = b.n(), n_threads = pool.n;
    std::vector<std::string> &part = b.sam;
    part.assign((size_t)n_threads, std::string());
    pool.parallel([&](int t) {
            std::vector<char> buf(1 << 16);
            int lo = (int)((long)n * t / n_threads), hi = (int)((long)n * (t + 1) / n_threads);
            std::string &out = part[(size_t)t];
            out.reserve((size_t)(hi - lo) * 400);
            for (int i = lo; i < hi; ++i) {
                const int L = (int)(b.offs[i + 1] - b.offs[i]);
                if ((size_t)L * 4 + 4096 > buf.size()) buf.resize((size_t)L * 4 + 4096);
                int w = salt_sam_se(ix, so, b.raw.data() + b.name[i], b.seqs.data() + b.offs[i], L, b.raw.data() + b.qual[i], &b.res[i], buf.data(), buf.size());
                if (w < 0) { fprintf(stderr, "[salt] SAM record too long for read %s\n", b.raw.data() + b.name[i]); exit(1); }
                out.append(buf.data(), (size_t)w);
                out.push_back('\n');
            }
    });
}

// -p: both SAM records of every pair (alnpe_sam, sam.c:331-457); res holds the mates interleaved
void format_batch_pe(const salt_index_t *ix, const salt_sam_opt_t *so, const salt_pe_opt_t *po, Batch &b, Pool &pool)
{
    const int n = b.n(), n_threads = pool.n;
    const Batch &m = *b.mate;
    std::vector<std::string> &part = b.sam;
    part.assign((size_t)n_threads, std::string());
    pool.parallel([&](int t) {
            std::vector<char> buf(1 << 17);
            int lo = (int)((long)n * t / n_threads), hi = (int)((long)n * (t + 1) / n_threads);
            std::string &out = part[(size_t)t];
            out.reserve((size_t)(hi - lo) * 900);
            for (int i = lo; i < hi; ++i) {
                const char *nm[2] = { b.raw.data() + b.name[i], m.raw.data() + m.name[i] };
                const char *ql[2] = { b.raw.data() + b.qual[i], m.raw.data() + m.qual[i] };
                const uint8_t *sq[2] = { b.seqs.data() + b.offs[i], m.seqs.data() + m.offs[i] };
                const int32_t ls[2] = { (int32_t)(b.offs[i + 1] - b.offs[i]), (int32_t)(m.offs[i + 1] - m.offs[i]) };
                if ((size_t)(ls[0] + ls[1]) * 8 + 16384 > buf.size()) buf.resize((size_t)(ls[0] + ls[1]) * 8 + 16384);
                int w = salt_sam_pe(ix, so, po, nm, sq, ls, ql, &b.res[2 * (size_t)i], buf.data(), buf.size());
                if (w < 0) { fprintf(stderr, "[salt] SAM record too long for pair %s\n", nm[0]); exit(1); }
                out.append(buf.data(), (size_t)w);
            }
    });
}

// mate: which adapter --trim-* searches the batch's reads with; count: their trim counters join the run's (not for infer_isize's look at the first batch)
// The three steps of parse_batch, apart for --trim-pair-overlap, which needs both mates' records before either is trimmed:
// batch_locate (the records' lines; names terminated), the trimming of the spans, batch_finish (qualities terminated, offsets, codes).
struct RecSpan { size_t s0, se, q0; };                         // bases [s0, se), qualities from q0
void batch_locate(std::vector<char> &raw, Batch &b, Pool &pool, std::vector<RecSpan> &span)
{
    const std::vector<uint32_t> &rec = b.rec;                  // record starts, found by the reader
    const int n = (int)rec.size(), n_threads = pool.n;
    b.name.assign((size_t)n, 0u); b.qual.assign((size_t)n, 0u);
    span.assign((size_t)n, RecSpan{ 0, 0, 0 });
    auto line_end = [&](size_t p) { const char *nl = (const char *)memchr(raw.data() + p, '\n', raw.size() - p); size_t e = nl ? (size_t)(nl - raw.data()) : raw.size(); return e; };
    pool.parallel([&](int t) {
        for (int i = (int)((long)n * t / n_threads); i < (int)((long)n * (t + 1) / n_threads); ++i) {
            size_t p = rec[(size_t)i], e = line_end(p);
            size_t ne = p + 1;
            while (ne < e && !isspace((unsigned char)raw[ne])) ++ne;
            size_t nl_ = ne - (p + 1);
            if (nl_ > 2 && raw[ne - 2] == '/' && isdigit((unsigned char)raw[ne - 1])) ne -= 2;   // trim_readno (query.c:139-143)
            b.name[(size_t)i] = (uint32_t)(p + 1);
            const size_t name_end = ne;
            size_t s0 = e + 1, s1 = line_end(s0);
            size_t se = s1; while (se > s0 && raw[se - 1] == '\r') --se;
            size_t p2 = s1 + 1, e2 = line_end(p2);           // '+' line
            size_t q0 = e2 + 1, q1 = line_end(q0);
            while (q1 > q0 && raw[q1 - 1] == '\r') --q1;
            if (raw[p] != '@' || p2 >= raw.size() || raw[p2] != '+' || q1 - q0 != se - s0) {
                fprintf(stderr, "[salt] input is not 4-line FASTQ at record %d of a batch ('%.60s'): multi-line records are only read when "
                                "the head of the file shows them\n", i, raw.data() + p);
                exit(1);
            }
            span[(size_t)i] = RecSpan{ s0, se, q0 };
            raw[name_end] = 0;                               // terminate in place (after every read of these lines)
        }
    });
}
void batch_finish(std::vector<char> &raw, Batch &b, Pool &pool, const std::vector<RecSpan> &span)
{
    const int n = (int)span.size(), n_threads = pool.n;
    b.offs.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const RecSpan &r = span[(size_t)i];
        b.qual[(size_t)i] = (uint32_t)r.q0;
        if (r.q0 + (r.se - r.s0) < raw.size()) raw[r.q0 + (r.se - r.s0)] = 0;
        b.offs[(size_t)i + 1] = b.offs[(size_t)i] + (uint32_t)(r.se - r.s0);
    }
    b.seqs.resize(b.offs[(size_t)n]);
    pool.parallel([&](int t) {
        for (int i = (int)((long)n * t / n_threads); i < (int)((long)n * (t + 1) / n_threads); ++i) {
            uint8_t *d = b.seqs.data() + b.offs[(size_t)i];
            const char *sp = raw.data() + span[(size_t)i].s0;
            for (size_t j = 0, L = span[(size_t)i].se - span[(size_t)i].s0; j < L; ++j) d[j] = nt4((unsigned char)sp[j]);
        }
    });
}
void parse_batch(std::vector<char> &raw, Batch &b, Pool &pool, int mate, bool count)
{
    std::vector<RecSpan> span;
    batch_locate(raw, b, pool, span);
    const int n = (int)span.size(), n_threads = pool.n;
    if (g_trim.on) pool.parallel([&](int t) {
        uint64_t trimmed[16] = {};
        for (int i = (int)((long)n * t / n_threads); i < (int)((long)n * (t + 1) / n_threads); ++i) {
            RecSpan &r = span[(size_t)i];
            if (r.se == r.s0) continue;
            uint32_t tb = 0, te = 0;                         // the span of the rule: bases, qualities and length move with it
            if (salt_trim_span(&g_trim.opt, mate, raw.data() + r.s0, raw.data() + r.q0, (uint32_t)(r.se - r.s0), &tb, &te, trimmed)) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); exit(1); }
            r = RecSpan{ r.s0 + tb, r.s0 + te, r.q0 + tb };
        }
        if (count) g_trim.add(trimmed, false);
    });
    batch_finish(raw, b, pool, span);
}
// Both mates' batches of a paired-end run (b2's reads are mate 2).  With --trim-pair-overlap every pair is trimmed as one (salt_trim_pair_span).
void parse_batch_pe(Batch &b1, Batch &b2, Pool &pool, bool count)
{
    if (!g_trim.pair_on || b1.rec.size() != b2.rec.size()) {   // (unequal numbers: the caller refuses the batches)
        parse_batch(b1.raw, b1, pool, 0, count); parse_batch(b2.raw, b2, pool, 1, count);
        return;
    }
    std::vector<RecSpan> s1, s2;
    batch_locate(b1.raw, b1, pool, s1); batch_locate(b2.raw, b2, pool, s2);
    const int n = (int)s1.size(), n_threads = pool.n;
    pool.parallel([&](int t) {
        uint64_t trimmed[16] = {}, pairs[8] = {};
        for (int i = (int)((long)n * t / n_threads); i < (int)((long)n * (t + 1) / n_threads); ++i) {
            RecSpan &r1 = s1[(size_t)i], &r2 = s2[(size_t)i];
            if (r1.se == r1.s0 || r2.se == r2.s0) continue;
            uint32_t sp[4];
            if (salt_trim_pair_span(g_trim.on ? &g_trim.opt : nullptr, &g_trim.pair_opt, b1.raw.data() + r1.s0, b1.raw.data() + r1.q0, (uint32_t)(r1.se - r1.s0),
                                    b2.raw.data() + r2.s0, b2.raw.data() + r2.q0, (uint32_t)(r2.se - r2.s0), sp, trimmed, pairs)) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); exit(1); }
            r1 = RecSpan{ r1.s0 + sp[0], r1.s0 + sp[1], r1.q0 + sp[0] };
            r2 = RecSpan{ r2.s0 + sp[2], r2.s0 + sp[3], r2.q0 + sp[2] };
        }
        if (count) { g_trim.add(trimmed, false); g_trim.add_pairs(pairs, false); }
    });
    batch_finish(b1.raw, b1, pool, s1); batch_finish(b2.raw, b2, pool, s2);
}

// The calling thread (and the threads it creates) onto the host NUMA node its GPU is attached to: the chunk a worker preads, the page-locked
// buffers allocated from it and the SAM text it writes then stay on that socket, and with --gpus N every GPU's workers use their own
// socket's cores and memory instead of contending for one.  Nothing happens when the platform does not name a node (or SALT_NO_PIN=1).
void pin_to_device_node(int device)
{
    static const bool off = getenv("SALT_NO_PIN") && atoi(getenv("SALT_NO_PIN"));
    int node = -1;
    if (off || salt_gpu_device_numa_node(device, &node) || node < 0) return;
    char path[96]; snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    FILE *f = fopen(path, "r");
    if (!f) return;
    cpu_set_t set; CPU_ZERO(&set);
    int a, b, any = 0; char sep;
    while (fscanf(f, "%d", &a) == 1) {                        // "0-63,128-191"
        b = a;
        if (fscanf(f, "%c", &sep) == 1 && sep == '-') { if (fscanf(f, "%d", &b) != 1) break; if (fscanf(f, "%c", &sep) != 1) sep = 0; }
        for (int c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET(c, &set); any = 1; }
        if (sep != ',') break;
    }
    fclose(f);
    if (any) sched_setaffinity(0, sizeof set, &set);
}

// ---------------------------------------------------------------------------------------------
// --polish on the host pipeline: the lines of a formatted batch that `polish` is to see -- no empty line (a skipped read's, the paired-end
// driver's), and neither record of a pair with a skipped mate -- through salt_gpu_polish_text; the batch's text becomes the polished records.
bool polish_batch(salt_gpu_polish_t *gp, bool pe, Batch &b)
{
    std::string lines;
    size_t total = 0;
    for (const std::string &p : b.sam) total += p.size();
    lines.reserve(total);
    size_t j = 0;                                            // line of the batch: single end record j; paired end record j / 2, then its blank line
    for (const std::string &p : b.sam)
        for (size_t at = 0; at < p.size(); ++j) {
            const char *e = (const char *)memchr(p.data() + at, '\n', p.size() - at);
            const size_t end = e ? (size_t)(e - p.data()) + 1 : p.size();
            bool keep = end - at > 1;
            if (keep && pe) { const size_t r = j / 2; keep = r < b.res.size() && !b.res[r].skipped && !b.res[r ^ 1].skipped; }
            if (keep) lines.append(p, at, end - at);
            at = end;
        }
    const salt_polish_opt_t po = { pe ? 1 : 0, g_polish == 2 ? 1 : 0 };
    const char *out = nullptr; uint64_t out_bytes = 0; uint32_t n = 0; int stopped = 0;
    if (salt_gpu_polish_text(gp, &po, lines.data(), lines.size(), &out, &out_bytes, &n, &stopped)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    b.sam.assign(1, std::string(out, (size_t)out_bytes));
    return true;
}

// --bgzf: the header, every SAM block in input order and htslib's empty end-of-file block, as independent gzip members of at most
// BGZF_CUT text bytes each.  On the text path the device deflates the SAM block behind the kernel that wrote it
// (salt_gpu_ws_set_sam_bgzf); everything else -- the header, the host pipeline, a libsalt_gpu without that entry point, and the text
// path under SALT_BGZF_HOST=1 -- goes through zlib level 1 here, on the worker that produced the text.  The writers do not change:
// whole blocks concatenate in order.
// ---------------------------------------------------------------------------------------------
const size_t BGZF_CUT = 32640;                               // the device's cut (salt_bgzf_block.h): both compressors cut the text the same way
const unsigned char BGZF_EOF[28] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
struct BgzfRun {
    bool on = false, device = false;                         // device: the text path's workspaces deflate
    std::atomic<bool> host_blocks{ false };                  // SAM blocks (not only the header) went through zlib
    std::atomic<uint64_t> text_bytes{ 0 }, file_bytes{ 0 };
} g_bgzf;

// text[0 .. n) -> BGZF blocks appended to out
bool bgzf_deflate_host(const char *text, size_t n, std::string &out)
{
    z_stream z; memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    bool ok = true;
    for (size_t at = 0; at < n && ok; at += BGZF_CUT) {
        const size_t len = std::min(BGZF_CUT, n - at), base = out.size(), bound = deflateBound(&z, (uLong)len);
        out.resize(base + 18 + bound + 8);
        unsigned char *o = reinterpret_cast<unsigned char *>(&out[base]);
        deflateReset(&z);
        z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(text + at)); z.avail_in = (uInt)len;
        z.next_out = o + 18; z.avail_out = (uInt)bound;
        ok = deflate(&z, Z_FINISH) == Z_STREAM_END && 18 + z.total_out + 8 <= 65536;
        if (!ok) break;
        const size_t clen = z.total_out, bsize = 18 + clen + 8 - 1;
        memcpy(o, BGZF_EOF, 16); o[16] = (unsigned char)bsize; o[17] = (unsigned char)(bsize >> 8);
        const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef *>(text + at), (uInt)len), isize = (uint32_t)len;
        for (int i = 0; i < 4; ++i) { o[18 + clen + i] = (unsigned char)(crc >> (8 * i)); o[18 + clen + 4 + i] = (unsigned char)(isize >> (8 * i)); }
        out.resize(base + 18 + clen + 8);
    }
    deflateEnd(&z);
    return ok;
}

// the text bytes a run of whole BGZF blocks holds (the ISIZE fields, found by the BSIZE fields)
uint64_t bgzf_text_bytes(const char *blocks, uint64_t n)
{
    const unsigned char *b = reinterpret_cast<const unsigned char *>(blocks);
    uint64_t text = 0;
    for (uint64_t at = 0; at + 26 <= n; ) {
        const uint64_t bsize = (uint64_t)(b[at + 16] | (b[at + 17] << 8)) + 1;
        if (at + bsize > n) break;
        const unsigned char *t = b + at + bsize - 4;
        text += t[0] | (t[1] << 8) | (t[2] << 16) | ((uint64_t)t[3] << 24);
        at += bsize;
    }
    return text;
}

// --bam: the records come from the device's BAM kernels on the text path (salt_gpu_ws_set_sam_bam), deflated behind them like SAM text;
// everywhere else the SAM text of a block or batch becomes records here (salt_bam_from_sam), on the thread that deflates it next.
struct BamRun {
    bool on = false, device = false;                         // device: the text path's workspaces write the records
    std::atomic<bool> host_records{ false };                 // records (not only the header) were encoded on the host
    const salt_index_t *ix = nullptr;
} g_bam;

// The seven row tallies (--snp-counts, --depth, --error-profile, --genotype, --discover, --stats, --indels) run alike.  On the device the table belongs to each GPU's index and every
// align call adds into it (salt_gpu_index_*_enable); a block the text path has aligned and then drops at a hand-over is taken back
// (salt_gpu_ws_*_uncount): the host pipeline aligns those reads again.  Without the device's symbols the SAM lines of every block and
// batch that is written go through the tally's host twin, one caller at a time.
struct TallyRun {
    bool on = false, device = false; const char *fn = nullptr; FILE *fp = nullptr; uint32_t min_mapq = 0;
    const salt_index_t *ix = nullptr; std::mutex mu;
    bool host() const { return on && !device; }
};
// --snp-counts FILE: how many reads show which base at every SNP site of the index; the GPUs' tables are summed after the last block.
struct SnpRun : TallyRun { std::vector<uint32_t> host_counts; uint64_t n_sites = 0; } g_snp;
// --depth FILE: coverage along the genome, per base or per window.  After the last block the GPUs' difference arrays are added into the first
// GPU's and its text kernels print the file.
struct DepthRun : TallyRun { bool gz = false; uint32_t window = 0; std::vector<uint32_t> host_diff; } g_depth;
// --error-profile FILE: mismatches by cycle, quality and substitution, the index's SNP sites masked.  The host pipeline hands its batches'
// qualities over with salt_gpu_ws_set_quals; after the last block the GPUs' tables are fetched and summed on the host.  salt_errprof_text
// prints the file on both paths.
const size_t ERRPROF_CELLS = 2u * 512u * 95u * 16u;
const size_t STATS_CELLS = 6021;                 // SALT_STATS_CELLS of salt_gpu.h
struct ErrprofRun : TallyRun { bool full = false; std::vector<uint64_t> cells; uint64_t rec[16] = { 0 }; } g_errprof;
// --genotype FILE: a VCF record per SNP site of the index.  Like the profile, the host pipeline hands its batches' qualities over; after the
// last block the other GPUs' sums are added into the first GPU's, whose kernels make the calls and print the records piece by piece.
struct GtRun : TallyRun { bool gz = false; const char *sample = nullptr; std::vector<salt_gt_site_t> host_sums; } g_gt;
// --discover FILE: SNP candidates off the index's sites, in salt-idx's SNP-file format.  Like the genotypes, the host pipeline hands its
// batches' qualities over; after the last block the other GPUs' two arrays are added into the first GPU's, whose kernels flag, compact and
// print the candidates piece by piece.  The only tally whose default MAPQ floor is not 0.
struct DiscRun : TallyRun {
    bool gz = false, all = false; uint32_t min_baseq = 20, min_alt = 3, min_pct = 20; std::vector<uint64_t> host_alt; std::vector<uint32_t> host_diff;
    DiscRun() { min_mapq = 20; }
} g_disc;
// --stats FILE: the run's summary -- mapping counts, histograms of MAPQ, read length, GC, insert size and indel length, counts per contig.
// After the last block the GPUs' tables are fetched and summed on the host; salt_stats_text prints the file on both paths.
struct StatsRun : TallyRun { std::vector<uint64_t> cells, ct; } g_stats;
// --indels FILE: indel candidates as VCF.  Every GPU's index keeps a hash table of left-normalised allele keys and the tally's own
// difference array; after the last block the other GPUs' live slots and arrays are added into the first GPU's, whose kernels sort the
// alleles, apply the call rule and print the records piece by piece.  Like --discover its default MAPQ floor is 20.
struct IndelRun : TallyRun {
    bool gz = false; uint32_t min_alt = 3, min_pct = 20, log2_slots = 24; salt_indel_t *host_tab = nullptr; std::vector<uint32_t> host_diff;
    IndelRun() { min_mapq = 20; }
} g_indel;

// What differs between them where they run alike, in the order snp, depth, error profile, genotype, discover, stats, indels.  opt: --OPT FILE; stem: --STEM-min-mapq; mode:
// how the file is opened; does: what a libsalt_gpu without the symbols does not do (the --polish refusal); symbols: this libsalt_gpu has
// the device side; host_add: the twin over SAM lines (< 0: refused); uncount: the last align call's adds leave the device's table.
struct Tally {
    TallyRun *run; const char *opt, *stem, *mode, *does;
    bool (*symbols)(); int64_t (*host_add)(const char *sam, size_t n); int (*uncount)(salt_gpu_ws_t *ws);
};
const Tally TALLIES[7] = {
    { &g_snp, "snp-counts", "snp", "w", "counts",
      [] { return salt_gpu_index_snp_enable && salt_gpu_index_snp_sites && salt_gpu_index_snp_counts && salt_gpu_ws_snp_uncount; },
      [](const char *sam, size_t n) { return salt_snp_count_sam(g_snp.ix, sam, n, g_snp.min_mapq, g_snp.host_counts.data(), g_snp.n_sites); }, salt_gpu_ws_snp_uncount },
    { &g_depth, "depth", "depth", "wb", "marks the coverage",
      [] { return salt_gpu_index_depth_enable && salt_gpu_index_depth_fetch && salt_gpu_index_depth_add && salt_gpu_index_depth_text_begin && salt_gpu_index_depth_text_next && salt_gpu_ws_depth_uncount; },
      [](const char *sam, size_t n) { return salt_depth_add_sam(g_depth.ix, sam, n, g_depth.min_mapq, g_depth.host_diff.data(), g_depth.host_diff.size()); }, salt_gpu_ws_depth_uncount },
    { &g_errprof, "error-profile", "error-profile", "w", "makes the profile",
      [] { return salt_gpu_index_errprof_enable && salt_gpu_index_errprof_fetch && salt_gpu_ws_errprof_uncount && salt_gpu_ws_set_quals; },
      [](const char *sam, size_t n) { return salt_errprof_add_sam(g_errprof.ix, sam, n, g_errprof.min_mapq, g_errprof.cells.data(), g_errprof.cells.size(), g_errprof.rec); }, salt_gpu_ws_errprof_uncount },
    { &g_gt, "genotype", "genotype", "wb", "sums and calls the genotypes",
      [] { return salt_gpu_index_gt_enable && salt_gpu_index_gt_fetch && salt_gpu_index_gt_add && salt_gpu_index_gt_text_begin && salt_gpu_index_gt_text_next && salt_gpu_ws_gt_uncount && salt_gpu_ws_set_quals; },
      [](const char *sam, size_t n) { return salt_gt_add_sam(g_gt.ix, sam, n, g_gt.min_mapq, g_gt.host_sums.data(), g_gt.host_sums.size()); }, salt_gpu_ws_gt_uncount },
    { &g_disc, "discover", "discover", "wb", "counts and prints the candidates",
      [] { return salt_gpu_index_disc_enable && salt_gpu_index_disc_fetch && salt_gpu_index_disc_add && salt_gpu_index_disc_text_begin && salt_gpu_index_disc_text_next && salt_gpu_index_disc_text_seen &&
                  salt_gpu_ws_disc_uncount && salt_gpu_ws_set_quals; },
      [](const char *sam, size_t n) { return salt_disc_add_sam(g_disc.ix, sam, n, g_disc.min_mapq, g_disc.min_baseq, g_disc.host_alt.data(), g_disc.host_diff.data(), g_disc.host_alt.size()); }, salt_gpu_ws_disc_uncount },
    { &g_stats, "stats", "stats", "w", "makes the summary",
      [] { return salt_gpu_index_stats_enable && salt_gpu_index_stats_fetch && salt_gpu_ws_stats_uncount; },
      [](const char *sam, size_t n) { return salt_stats_add_sam(g_stats.ix, sam, n, g_stats.min_mapq, g_stats.cells.data(), g_stats.cells.size(), g_stats.ct.data(), g_stats.ct.size()); }, salt_gpu_ws_stats_uncount },
    { &g_indel, "indels", "indels", "wb", "tables and prints the indels",
      [] { return salt_gpu_index_indel_enable && salt_gpu_index_indel_stats && salt_gpu_index_indel_fetch && salt_gpu_index_indel_add && salt_gpu_index_indel_fetch_diff &&
                  salt_gpu_index_indel_add_diff && salt_gpu_index_indel_text_begin && salt_gpu_index_indel_text_next && salt_gpu_ws_indel_uncount; },
      [](const char *sam, size_t n) { return salt_indel_add_sam(g_indel.ix, g_indel.host_tab, sam, n, g_indel.min_mapq, g_indel.host_diff.data(), g_indel.host_diff.size() - 1); }, salt_gpu_ws_indel_uncount },
};

// the SAM lines of a block or batch that is about to be written, through every host twin that is on; false with the reason on stderr
bool host_twins_add(const char *sam, size_t n)
{
    for (const Tally &t : TALLIES) {
        if (!t.run->host()) continue;
        std::lock_guard<std::mutex> lk(t.run->mu);
        if (t.host_add(sam, n) < 0) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
    }
    return true;
}
// a block the text path aligned and will not write leaves the device's tables
void drop_block(salt_gpu_ws_t *ws)
{
    for (const Tally &t : TALLIES)
        if (t.run->on && t.run->device && t.uncount(ws)) fprintf(stderr, "[salt] %s\n", salt_gpu_last_error());
    if (g_trim.device && salt_gpu_ws_trim_uncount(ws)) fprintf(stderr, "[salt] %s\n", salt_gpu_last_error());      // (the host parser trims those reads again)
}

// SAM lines -> BAM records in `out`; false with the reason on stderr (a read name past the format's limit)
bool bam_of_sam(const char *sam, size_t n, std::string &out)
{
    int64_t w = SALT_BAM_E_CAP;
    for (size_t cap = 2 * n + 4096; w == SALT_BAM_E_CAP && cap <= SALT_BAM_BOUND(n) + 2 * n + 4096; cap *= 2) {
        out.resize(cap);
        w = salt_bam_from_sam(g_bam.ix, sam, n, reinterpret_cast<uint8_t *>(&out[0]), cap, nullptr);
    }
    if (w < 0) { fprintf(stderr, "[salt] %s\n", w == SALT_BAM_E_CAP ? "BAM: records larger than their bound" : salt_host_last_error()); return false; }
    out.resize((size_t)w);
    g_bam.host_records = true;
    return true;
}

// a batch of the host pipeline: its SAM pieces become BGZF blocks, cut over the whole batch and deflated by the worker's helper threads
bool bgzf_batch(std::vector<std::string> &pieces, Pool &pool)
{
    std::string all;
    size_t n = 0;
    if (g_bam.on) {                                          // every piece holds whole lines: records piece by piece, side by side
        std::vector<std::string> rec(pieces.size());
        std::atomic<bool> good{ true };
        pool.parallel([&](int t) { for (size_t i = (size_t)t; i < pieces.size(); i += (size_t)pool.n) if (!bam_of_sam(pieces[i].data(), pieces[i].size(), rec[i])) good = false; });
        if (!good) return false;
        pieces.swap(rec);
    }
    for (const std::string &p : pieces) n += p.size();
    all.reserve(n);
    for (const std::string &p : pieces) all += p;
    const size_t n_blocks = (n + BGZF_CUT - 1) / BGZF_CUT, n_threads = (size_t)pool.n;
    std::vector<std::string> out(n_threads);
    std::atomic<bool> ok{ true };
    pool.parallel([&](int t) {
        const size_t lo = n_blocks * (size_t)t / n_threads * BGZF_CUT, hi = std::min(n, n_blocks * ((size_t)t + 1) / n_threads * BGZF_CUT);
        if (lo < hi && !bgzf_deflate_host(all.data() + lo, hi - lo, out[(size_t)t])) ok = false;
    });
    size_t bytes = 0;
    for (const std::string &o : out) bytes += o.size();
    g_bgzf.text_bytes += n; g_bgzf.file_bytes += bytes; g_bgzf.host_blocks = true;
    pieces.swap(out);
    return ok;
}

// a block of the text path, before it is written: from the device it is BGZF already; otherwise it becomes BGZF here (zbuf: the worker's own)
bool bgzf_text_block(const char *&sam, uint64_t &sam_bytes, std::string &zbuf)
{
    std::string rec;
    if (g_bam.on && !g_bam.device) {
        if (!bam_of_sam(sam, (size_t)sam_bytes, rec)) return false;
        sam = rec.data(); sam_bytes = rec.size();
    }
    if (g_bgzf.device) g_bgzf.text_bytes += bgzf_text_bytes(sam, sam_bytes);
    else {
        zbuf.clear();
        if (!bgzf_deflate_host(sam, (size_t)sam_bytes, zbuf)) return false;
        g_bgzf.text_bytes += sam_bytes; g_bgzf.host_blocks = true;
        sam = zbuf.data(); sam_bytes = zbuf.size();
    }
    g_bgzf.file_bytes += sam_bytes;
    return true;
}

// after the last SAM block of a run that succeeded: the end-of-file block, and the line that says which compressor ran
void bgzf_finish()
{
    if (!g_bgzf.on) return;
    fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, stdout);
    fflush(stdout);
    g_bgzf.file_bytes += sizeof BGZF_EOF;
    const bool dev = g_bgzf.device, host = g_bgzf.host_blocks;
    fprintf(stderr, "[salt] BGZF output: %s deflate%s, %llu -> %llu bytes\n", dev ? "device" : "host", dev && host ? " (host deflate behind the hand-over)" : "",
            (unsigned long long)g_bgzf.text_bytes.load(), (unsigned long long)g_bgzf.file_bytes.load());
    if (g_bam.on) {
        const bool bd = g_bam.device, bh = g_bam.host_records;
        fprintf(stderr, "[salt] BAM output: %s records%s, %llu -> %llu bytes\n", bd ? "device" : "host", bd && bh ? " (host records behind the hand-over)" : "",
                (unsigned long long)g_bgzf.text_bytes.load(), (unsigned long long)g_bgzf.file_bytes.load());
    }
}

double now() { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + ts.tv_nsec * 1e-9; }

int usage()
{
    fprintf(stderr,
            "\nUsage:     salt [Options] <Index.prefix> <Read_mate1> [Read_mate2]\n\n"
            "Options:   -h, --help                   help\n"
            "           -t, --threads       <int>    host threads (SAM formatting)\n"
            "           -g, --group         <str>    read group id\n"
            "           -c, --xa_cigar               print cigar in XA fields [False]\n"
            "           -d, --md                     print tag NM and MD [False]\n"
            "           -r, --overlap       <int>    seed stride [seed length]\n"
            "           -v, --ref                    only seed on the primary reference\n"
            "           -s, --max_seed      <int>    max seed occ [50]\n"
            "           -m, --max_locate    <int>    max loci per strand [1000] (up to 262144)\n"
            "           -p, --pe                     paired end mode (two read files)\n"
            "           -a, --min_tlen      <int>    min template length [250]\n"
            "           -b, --max_tlen      <int>    max template length [550]\n"
            "               --gpus          <int>    GPUs to shard batches over [1]\n"
            "               --bgzf                   write the SAM stream as BGZF blocks (.sam.gz), deflated on the GPU [False]\n"
            "               --bam                    write BAM: binary records from the GPU inside BGZF blocks (implies --bgzf;\n"
            "                                        read names of up to 254 bytes) [False]\n"
            "               --polish[=lv|sw]         print the records `polish` (lv) or `polish -s` (sw) makes of the SAM lines, re-scored\n"
            "                                        on the GPU, no header; not with --bam [False]\n"
            "               --snp-counts    <file>   write, per SNP site of the index, how many reads show A, C, G, T there (counted on\n"
            "                                        the GPU; tab-separated, one line per site) [off]\n"
            "               --snp-min-mapq  <int>    --snp-counts: records with a smaller MAPQ do not count, 0 .. 255 [0]\n"
            "               --depth         <file>   write the coverage along the genome (made on the GPU): bedGraph, one line per run\n"
            "                                        of equal depth; a name ending in .gz is written as BGZF [off]\n"
            "               --depth-min-mapq <int>   --depth: records with a smaller MAPQ do not count, 0 .. 255 [0]\n"
            "               --depth-window  <int>    --depth: the mean depth of every window of <int> positions instead [per base]\n"
            "               --error-profile <file>   write how often a sequenced base disagrees with the genome, by cycle, base quality and\n"
            "                                        substitution, the index's SNP sites left out (counted on the GPU; tab-separated) [off]\n"
            "               --error-profile-min-mapq <int>  --error-profile: records with a smaller MAPQ do not count, 0 .. 255 [0]\n"
            "               --error-profile-full     --error-profile: also every non-zero cell (mate, cycle, quality, ref, read)\n"
            "               --stats <file>           write the run's summary: mapped, properly paired and per-contig counts, histograms of MAPQ,\n"
            "                                        read length, GC, insert size and indel length, summed on the GPU behind every block\n"
            "               --stats-min-mapq <int>   --stats: records with a smaller MAPQ are mapped but not counted, 0 .. 255 [0]\n"
            "               --indels        <file>   write the insertions and deletions the reads show as VCF 4.2 records, left-normalised\n"
            "                                        against the genome: anchor position, REF, ALT, depth and the observations per strand\n"
            "                                        (tabled, sorted, called and printed on the GPU); .gz is written as BGZF [off]\n"
            "               --indels-min-mapq <int>  --indels: records with a smaller MAPQ do not count, 0 .. 255 [20]\n"
            "               --indels-min-alt <int>   --indels: an allele is called from this many observations, 1 .. 4294967295 [3]\n"
            "               --indels-min-pct <int>   --indels: ... that are at least this share of the depth at the anchor, 0 .. 100 [20]\n"
            "               --indels-slots <int>     --indels: slots of the GPU's allele table, a power of two from 64 to 268435456, 16 bytes\n"
            "                                        each; alleles that find no slot are dropped and counted [16777216]\n"
            "               --trim-adapter  <seq>    trim the reads in front of the aligner (on the GPU, in the FASTQ block as it lies there):\n"
            "                                        cut a read where this 3' adapter starts, 1 to 64 letters of ACGT; the leftmost start whose\n"
            "                                        overlap with the adapter (no indels) has few enough mismatches; single end and mate 1 [off]\n"
            "               --trim-adapter2 <seq>    --trim-adapter: the adapter of mate 2 [the one of mate 1]\n"
            "               --trim-min-overlap <int> --trim-adapter: an overlap at the read's end counts from this many bases, 1 .. 64 [5]\n"
            "               --trim-error-pct <int>   --trim-adapter: mismatches allowed, in percent of the overlap, 0 .. 50 [10]\n"
            "               --trim-qual     <int>    cut the 3' end by base quality, the rule of bwa aln -q and cutadapt -q, 1 .. 93 [off]\n"
            "               --trim-front    <int>    remove this many bases from every read's 5' end, 0 .. 511 [0]\n"
            "               --trim-tail     <int>    remove this many bases from every read's 3' end, 0 .. 511 [0]\n"
            "                                        order: clips, quality, adapter; a read keeps at least one base, no read is dropped;\n"
            "                                        one line of counters on stderr\n"
            "               --trim-pair-overlap      paired end: find each pair's adapters from the mates' overlap, whatever the adapter is (on the\n"
            "                                        GPU): the largest insert length at which the mates agree, both cut there; between the\n"
            "                                        quality and the adapter step; mates of up to 512 bases; nothing is merged or corrected;\n"
            "                                        a second line of counters on stderr [off]\n"
            "               --trim-pair-min-overlap <int>  --trim-pair-overlap: the mates agree over at least this many bases, 1 .. 512 [20]\n"
            "               --trim-pair-error-pct <int>    --trim-pair-overlap: mismatches allowed, in percent of the overlap, 0 .. 50 [10]\n"
            "               --genotype      <file>   write a VCF 4.2 record per SNP site of the index: the genotype, allele depths and\n"
            "                                        likelihoods from the reads' bases and base qualities (summed, called and printed on\n"
            "                                        the GPU); a name ending in .gz is written as BGZF [off]\n"
            "               --genotype-min-mapq <int>  --genotype: records with a smaller MAPQ do not count, 0 .. 255 [0]\n"
            "               --genotype-sample <name>   --genotype: the sample column's name [sample]\n"
            "               --discover      <file>   write the SNP candidates OFF the index's sites: positions where the reads show a base\n"
            "                                        the index does not have there, in salt-idx's SNP-file format (contig, pos, alleles, ref;\n"
            "                                        then depth and counts), counted and printed on the GPU; .gz is written as BGZF [off]\n"
            "               --discover-min-mapq <int>  --discover: records with a smaller MAPQ do not count, 0 .. 255 [20: the only tally\n"
            "                                        whose default is not 0, because mismapped paralogs are what makes false SNPs]\n"
            "               --discover-min-baseq <int> --discover: bases with a smaller quality do not count, 0 .. 93 [20]\n"
            "               --discover-min-alt <int>   --discover: a base is called from this many observations, 1 .. 2097151 [3]\n"
            "               --discover-min-pct <int>   --discover: ... that are at least this share of the depth, 0 .. 100 [20]\n"
            "               --discover-all           --discover: also the index's sites without a called base: a whole SNP file\n"
            "           (-n -e -l -M -O -E -X are accepted and ignored like in the reference)\n\n");
    return 1;
}

// ---------------------------------------------------------------------------------------------
// Single end, plain 4-line FASTQ in a regular file: the text path.  FASTQ text goes to the GPU as it lies in the file, SAM text comes
// back (salt_gpu_align_se_text: parse, align and format are kernels), and the host only moves bytes:
//   every worker claims the next chunk of the file (pread into page-locked memory), cuts it at record boundaries -- a record starts
//   at a line that begins with '@' and whose next-but-one line begins with '+' (a quality line may begin with '@', but then the
//   line two further on is a sequence) --, calls the device, and writes its SAM block when the blocks before it have been written.
//   One writer at a time also for regular files: buffered writes to one file serialize on the inode anyway (one thread alone writes
//   10.6 GB/s into the page cache of the GPU box, eight threads with pwrite at their own offsets 9.5 GB/s between them), and the
//   blocks behind the one being written are read and aligned meanwhile.  Output order = input order, as the reference's puts loop
//   gives it (alnse.c:1433-1439).
// ---------------------------------------------------------------------------------------------
// ---- BGZF input (blocked gzip: every block is a gzip member of at most 64 KiB with its compressed size in a 'BC' extra field -- what
// bgzip and most sequencing pipelines write).  The reference reads any .gz through gzopen (query.c:103-112), one stream, one thread; a
// blocked file can be cut anywhere: the block table (compressed offset, uncompressed offset) is read from the headers and trailers
// without inflating, and the text path treats the UNCOMPRESSED byte range as its file -- a worker inflates the blocks its chunk touches
// into its page-locked buffer, a few at a time on helper threads.  Plain single-member gzip stays on the host pipeline.
struct Bgzf {
    std::vector<uint64_t> coff, uoff;                        // per block: offset in the file, offset in the uncompressed text; one entry past the end
    bool ok = false;
};
static bool bgzf_index(const char *fn, Bgzf &B)
{
    const int fd = open(fn, O_RDONLY);
    if (fd < 0) return false;
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { close(fd); return false; }
    const uint64_t size = (uint64_t)sb.st_size;
    uint64_t at = 0, u = 0;
    bool good = true;
    while (at < size) {
        unsigned char h[18 + 256];
        const ssize_t got = pread(fd, h, sizeof h, (off_t)at);
        if (got < 18 || h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) { good = false; break; }
        const uint32_t xlen = h[10] | (h[11] << 8);
        uint32_t bsize = 0;
        for (uint32_t p = 12; p + 4 <= 12 + xlen && p + 4 <= (uint32_t)got; ) {       // extra subfields: SI1 SI2 SLEN data
            const uint32_t slen = h[p + 2] | (h[p + 3] << 8);
            if (h[p] == 'B' && h[p + 1] == 'C' && slen == 2 && p + 6 <= (uint32_t)got) { bsize = (h[p + 4] | (h[p + 5] << 8)) + 1u; break; }
            p += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || at + bsize > size) { good = false; break; }
        unsigned char t[4];
        if (pread(fd, t, 4, (off_t)(at + bsize - 4)) != 4) { good = false; break; }
        const uint32_t isize = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
        if (isize > 65536) { good = false; break; }
        B.coff.push_back(at); B.uoff.push_back(u);
        at += bsize; u += isize;
    }
    close(fd);
    if (!good || B.coff.empty()) { B.coff.clear(); B.uoff.clear(); return false; }
    B.coff.push_back(at); B.uoff.push_back(u);
    B.ok = true;
    return true;
}
// inflates block b (bytes cbuf[0 .. csize) of the file) to exactly usize bytes at dst; false on a damaged block
static bool bgzf_inflate(const unsigned char *cbuf, size_t csize, char *dst, size_t usize)
{
    if (csize < 26) return false;
    const uint32_t xlen = cbuf[10] | (cbuf[11] << 8);
    const size_t hdr = 12 + (size_t)xlen;
    if (hdr + 8 > csize) return false;
    z_stream z; memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -15) != Z_OK) return false;
    z.next_in = const_cast<unsigned char *>(cbuf + hdr); z.avail_in = (uInt)(csize - hdr - 8);
    z.next_out = reinterpret_cast<unsigned char *>(dst); z.avail_out = (uInt)usize;
    const int rc = inflate(&z, Z_FINISH);
    bool ok = (rc == Z_STREAM_END || (usize == 0 && rc == Z_BUF_ERROR)) && z.total_out == usize;
    inflateEnd(&z);
    if (ok) {                                                // the member's CRC-32, as gzread checks it
        const unsigned char *t = cbuf + csize - 8;
        const uint32_t want = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
        ok = (uint32_t)crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef *>(dst), (uInt)usize) == want;
    }
    return ok;
}

// file bytes [off, off + n) into dst, in as many reads as it takes; returns the bytes read (fewer than n: an error, or the file ends before)
static uint64_t pread_full(int fd, void *dst, uint64_t n, uint64_t off)
{
    uint64_t got = 0;
    while (got < n) { const ssize_t r = pread(fd, (char *)dst + got, (size_t)(n - got), (off_t)(off + got)); if (r <= 0) break; got += (uint64_t)r; }
    return got;
}
// The ordered block writer and run state of a text path, single end and paired end: workers claim chunks (next_chunk), block k is written
// once block k - 1 has been, and a failure stops everyone.  A chunk the device parser refused (SALT_E_INVAL: a multi-line record, a blank
// line, an empty read -- things kseq.h reads, query.c:103-239): the blocks before it are written, then the host parser takes over at
// `resume` -- single end a byte offset (a record start: everything before it was strict 4-line FASTQ), paired end a chunk index.
// One locking rule: a flag that a waiter's predicate reads is stored with that waiter's mutex held, before the notify -- a waiter that has
// evaluated its predicate but not yet blocked cannot miss the notify.  The paired-end workers wait for the scanners' offsets (PeScan) on
// this mutex and condition variable too, so a failure or a fallback wakes them like everyone else.
struct TextRun {
    std::mutex mu; std::condition_variable cv;
    uint64_t written = 0; long reads_done = 0;
    std::atomic<bool> failed{ false }, fallback{ false }; uint64_t resume = 0; std::atomic<uint64_t> next_chunk{ 0 };
    std::atomic<double> t_read{ 0 }, t_gpu{ 0 }, t_write{ 0 }, t_last;     // t_last: when the last SAM byte so far was written
    explicit TextRun(double t0) : t_last(t0) {}
    void fail() { { std::lock_guard<std::mutex> lk(mu); failed = true; } cv.notify_all(); }
    void fail_gpu() { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); fail(); }
    // waits until block k may be written; false when the run failed or fell back instead (claim: a true answer is the fallback's election)
    bool wait_turn(uint64_t k, bool claim = false)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return failed || fallback || written == k; });
        const bool mine = !failed && !fallback;
        if (mine && claim) fallback = true;
        return mine;
    }
    // block k, whose turn it is: its bytes to stdout, then the next block's turn; false (and the run failed) when they cannot be written
    bool write_block(uint64_t k, const char *sam, uint64_t sam_bytes, long n_reads)
    {
        const double tw0 = now(); bool ok = true;
        for (uint64_t w = 0; w < sam_bytes && ok; ) { const ssize_t r = write(1, sam + w, sam_bytes - w); if (r <= 0) ok = false; else w += (uint64_t)r; }
        t_write = t_write + (now() - tw0);
        { const double tn = now(); double cur = t_last.load(); while (tn > cur && !t_last.compare_exchange_weak(cur, tn)) {} }
        if (!ok) { fprintf(stderr, "[salt] write error on the SAM stream\n"); fail(); return false; }
        { std::lock_guard<std::mutex> lk(mu); written = k + 1; reads_done += n_reads; fprintf(stderr, "%ld reads have been aligned!\n", reads_done); }
        cv.notify_all();
        return true;
    }
    // chunk k cannot go through the device parser: once the blocks before it are out, everyone stops and the host pipeline continues there.
    // True for the first claimant of a run that has not failed: it alone sets `resume` (read after the workers have been joined)
    bool claim_fallback(uint64_t k) { const bool won = wait_turn(k, true); cv.notify_all(); return won; }
};
// a refused chunk is the host parser's, unless what the device refused is the output (a read name no BAM record holds)
static bool parser_refused(int grc) { return grc == SALT_E_INVAL && !(g_bam.device && strncmp(salt_gpu_last_error(), "BAM:", 4) == 0); }

static const uint64_t TEXT_SLACK = 1u << 20;             // how far past a chunk's end a worker looks for the next record start (longest record it can cut)

// first record start at or after `from` in buf[0..n): a line start whose line begins with '@' and whose next-but-one line begins with '+'.
// `from` itself counts only when the byte before it is a newline (or it is the start of the file).  Returns n when there is none.
static uint64_t next_record_start(const char *buf, uint64_t n, uint64_t from, bool from_is_line_start)
{
    uint64_t p = from;
    if (!from_is_line_start) { const char *nl = (const char *)memchr(buf + p, '\n', n - p); if (!nl) return n; p = (uint64_t)(nl - buf) + 1; }
    while (p < n) {
        const char *n1 = (const char *)memchr(buf + p, '\n', n - p);
        if (!n1) return n;
        const uint64_t l1 = (uint64_t)(n1 - buf) + 1;
        if (buf[p] == '@' && l1 < n) {
            const char *n2 = (const char *)memchr(buf + l1, '\n', n - l1);
            if (!n2) return n;
            const uint64_t l2 = (uint64_t)(n2 - buf) + 1;
            if (l2 < n && buf[l2] == '+') return p;
            if (l2 >= n) return n;
        }
        p = l1;
    }
    return n;
}

// next_record_start over text that lies on the device: text bytes [base, base + n) stand where buf[0 .. n) stands there (add_nl: a newline
// counts as byte n - 1, the file's last record lacks its own).  The function looks forward only, so it is run on a window peeked from
// `from` on -- 64 KiB, then TEXT_SLACK, then everything -- and a window that ends before the text does is widened when it answers "none":
// the offset is the one the whole buffer would give.  Returns false when the peek fails.
static bool next_record_start_dev(salt_gpu_ws_t *ws, std::vector<char> &win, uint64_t base, uint64_t n, bool add_nl, uint64_t from, bool at_file_start, uint64_t *res)
{
    const uint64_t ctx = from ? 1 : 0;                        // the byte in front of `from`: is `from` a line start?
    const uint64_t widths[3] = { 1u << 16, TEXT_SLACK, n };
    for (int i = 0; i < 3; ++i) {
        const uint64_t w_lo = from - ctx, w_hi = std::min(n, from + widths[i]), wn = w_hi - w_lo;
        const bool nl_in = add_nl && w_hi == n;               // the window reaches the newline that is not in the text
        win.resize((size_t)wn + 1);
        if (salt_gpu_ws_text_peek(ws, base + w_lo, wn - (nl_in ? 1 : 0), win.data())) return false;
        if (nl_in) win[(size_t)wn - 1] = '\n';
        const uint64_t r = from < n ? next_record_start(win.data(), wn, ctx, ctx ? win[0] == '\n' : at_file_start) : wn;
        if (r < wn || w_hi == n) { *res = r < wn ? w_lo + r : n; return true; }
    }
    *res = n;
    return true;
}

// What the text path needs to know before the index is there: chunk size, workers, and -- from the first 64 KB of the file -- how many
// reads a chunk is expected to hold and how much SAM they turn into.  Workspaces are sized by that expectation (+ 30 %), not by the
// worst case of 32-byte records; a chunk that holds more reads (SALT_E_CAPACITY) has its worker re-create the workspace for the worst
// case and call again.
struct TextPlan {
    uint64_t chunk = 0, in_cap = 0, sam_cap = 0;
    int n_workers = 0, wpg = 0;
    uint32_t worst_reads = 0, max_reads = 0, head_read_len = 0;
    // page-locked buffers, allocated by a thread of their own while the index is loaded and attached
    std::vector<char *> in_buf, sam_buf;
    std::thread alloc; bool alloc_ok = true; double alloc_s = 0;
    bool pe = false; uint64_t pairs_per_chunk = 0;          // paired end: chunks are cut by record count (both files the same), about `chunk` bytes per file
    Bgzf bgzf;                                               // single end, blocked gzip input: its block table
    ~TextPlan();
};

static void text_plan(TextPlan &P, const char *fn_reads, int n_gpus, int n_threads, bool pe)
{
    P.pe = pe;
    { const char *e = getenv("SALT_CHUNK_MB"); int mb = e ? atoi(e) : 32; if (mb < 1) mb = 1; if (mb > 1024) mb = 1024; P.chunk = (uint64_t)mb << 20; }
    if (const char *e = getenv("SALT_CHUNK_BYTES")) { long v = atol(e); if (v >= 256) P.chunk = (uint64_t)v; }      // tests: many chunks on a small file
    // workers per GPU: each preads a chunk, calls the device and writes its block in turn.  The write stream is the narrow part (one
    // writer at a time); three to four workers keep it busy, more only lengthen the start-up (measured 2: 25.8, 3: 28.7, 4: 27.9,
    // 6: 24.2, 8: 23.8 Mreads/s on 16 M reads)
    P.wpg = n_threads / n_gpus >= 4 ? 4 : 2;
    if (const char *e = getenv("SALT_TEXT_WORKERS")) { int v = atoi(e); if (v >= 1 && v <= 32) P.wpg = v; }
    P.n_workers = n_gpus * P.wpg;
    P.worst_reads = (uint32_t)((P.chunk + TEXT_SLACK) / 32);
    P.max_reads = P.worst_reads;
    double sam_per_fq_byte = 1.5;                            // SAM bytes a FASTQ byte turns into, for the first sizing of the SAM buffers
    char head[65536];
    ssize_t got = -1;
    if (P.bgzf.ok) {                                         // the head of the TEXT: the first block, inflated
        const int fd = open(fn_reads, O_RDONLY);
        std::vector<unsigned char> cb((size_t)(P.bgzf.coff[1] - P.bgzf.coff[0]));
        const size_t us = (size_t)(P.bgzf.uoff[1] - P.bgzf.uoff[0]);
        if (fd >= 0 && pread(fd, cb.data(), cb.size(), 0) == (ssize_t)cb.size() && us <= sizeof head && bgzf_inflate(cb.data(), cb.size(), head, us)) got = (ssize_t)us;
        if (fd >= 0) close(fd);
    } else { const int fd = open(fn_reads, O_RDONLY); if (fd >= 0) { got = pread(fd, head, sizeof head, 0); close(fd); } }
    uint64_t lines = 0, last_rec_end = 0, line_start = 0, name_bytes = 0;
    for (ssize_t i = 0; i < got; ++i)
        if (head[i] == '\n') {
            const uint32_t len = (uint32_t)((uint64_t)i - line_start);
            if ((lines & 3) == 0) name_bytes += len;
            if ((lines & 3) == 1 && len > P.head_read_len) P.head_read_len = len;
            line_start = (uint64_t)i + 1;
            if ((++lines & 3) == 0) last_rec_end = (uint64_t)i + 1;
        }
    if (lines >= 4 && last_rec_end) {
        const double n_rec = (double)(lines / 4), rec_bytes = (double)last_rec_end / n_rec;
        const double est = (double)(P.chunk + TEXT_SLACK) / rec_bytes * 1.3 + 1024.0;
        if (est < (double)P.worst_reads) P.max_reads = (uint32_t)est;
        // a record: name, the fixed fields (~45 bytes), SEQ, QUAL, tags (NM MD XV XA: ~40 + alternative hits)
        sam_per_fq_byte = (name_bytes / n_rec + 2.0 * P.head_read_len + 160.0) / rec_bytes;
    }
    if (P.head_read_len > SALT_MAX_READ_LEN) P.head_read_len = 0;      // the call itself reports it
    P.in_cap = P.chunk + 2 * TEXT_SLACK + 64 + (P.bgzf.ok ? (3u << 16) : 0u);      // blocked input: whole 64 KiB blocks at both ends
    P.sam_cap = (uint64_t)((double)(P.chunk + TEXT_SLACK) * sam_per_fq_byte) + 4096;
    if (pe) {                                                // a chunk = pairs_per_chunk records of EACH file; both blocks share the input buffer
        const double rec_bytes = lines >= 4 && last_rec_end ? (double)last_rec_end / (double)(lines / 4) : 250.0;
        P.pairs_per_chunk = (uint64_t)((double)P.chunk / rec_bytes) + 1;
        P.max_reads = (uint32_t)(2 * P.pairs_per_chunk);
        P.worst_reads = P.max_reads;                         // exact: the record count is what defines a chunk
        P.in_cap = 2 * (uint64_t)((double)P.chunk * 1.5) + 2 * TEXT_SLACK + 64;
        P.sam_cap = 2 * (uint64_t)((double)P.chunk * (sam_per_fq_byte + 0.3)) + 4096;
    }
    P.in_buf.assign((size_t)P.n_workers, nullptr); P.sam_buf.assign((size_t)P.n_workers, nullptr);
    P.alloc = std::thread([&P]() {
        const double t = now();
        for (int w = 0; w < P.n_workers && P.alloc_ok; ++w) {
            if (w % P.wpg == 0) pin_to_device_node(w / P.wpg);    // worker w's buffers from its GPU's node
            if (salt_gpu_host_alloc(P.in_cap, (void **)&P.in_buf[(size_t)w]) || salt_gpu_host_alloc(P.sam_cap, (void **)&P.sam_buf[(size_t)w])) P.alloc_ok = false;
        }
        P.alloc_s = now() - t;
    });
}

TextPlan::~TextPlan()
{
    if (alloc.joinable()) alloc.join();
    for (char *b : in_buf) if (b) salt_gpu_host_free(b);
    for (char *b : sam_buf) if (b) salt_gpu_host_free(b);
}

// A workspace of the text path on `gix` for chunks of up to max_reads reads, with the run's output modes set.  text_reads non-zero (and a
// read length known from the file's head): the device buffers for chunks of text_bytes holding that many reads are reserved now, the SAM
// text landing in worker wk's page-locked buffer.  Returns the first error code; *ws is the caller's to destroy either way.
static int open_text_ws(salt_gpu_index_t *gix, uint32_t max_reads, salt_gpu_ws_t **ws, const salt_aln_opt_t *ao = nullptr, const TextPlan *P = nullptr, int wk = 0, uint64_t text_bytes = 0, uint32_t text_reads = 0)
{
    int rc = salt_gpu_ws_create(gix, max_reads, (uint64_t)max_reads * 160, ws);
    if (!rc && g_bgzf.device) rc = salt_gpu_ws_set_sam_bgzf(*ws, 1);
    if (!rc && g_bam.device) rc = salt_gpu_ws_set_sam_bam(*ws, 1);
    if (!rc && g_polish) rc = salt_gpu_ws_set_polish(*ws, g_polish);
    if (!rc && g_trim.device && g_trim.on) rc = salt_gpu_ws_set_trim(*ws, &g_trim.opt);
    if (!rc && g_trim.device && g_trim.pair_on) rc = salt_gpu_ws_set_trim_pair(*ws, &g_trim.pair_opt);
    if (!rc && text_reads && P->head_read_len) rc = salt_gpu_ws_reserve_text(*ws, ao, text_bytes, text_reads, P->head_read_len, P->sam_cap - 64, P->sam_buf[(size_t)wk], P->sam_cap);
    return rc;
}
// the contig table of the host index, for RNAME / POS on the device and for the polish handles
struct Contigs {
    std::vector<int64_t> off; std::vector<const char *> nm;
    explicit Contigs(const salt_index_t *ix) : off((size_t)salt_index_n_seqs(ix)), nm(off.size()) { for (size_t i = 0; i < off.size(); ++i) salt_index_seq(ix, (int)i, &off[i], nullptr, &nm[i]); }
    int32_t n() const { return (int32_t)off.size(); }
};
// what both text paths begin with: the contig table on every GPU, and the page-locked buffers there
static bool text_begin(const std::vector<salt_gpu_index_t *> &gix, const Contigs &C, TextPlan &P)
{
    fflush(stdout);
    bool ok = true;
    for (salt_gpu_index_t *g : gix) ok = ok && salt_gpu_index_set_contigs(g, C.n(), C.off.data(), C.nm.data()) == 0;
    if (ok && P.alloc.joinable()) P.alloc.join();
    if (!ok || !P.alloc_ok) fprintf(stderr, "[salt] %s\n", salt_gpu_last_error());
    return ok && P.alloc_ok;
}

// what the workers of a single-end run share besides its TextRun
struct SeText {
    const char *fn; int fd = -1; uint64_t file_size = 0, chunk = 0, n_chunks = 0;
    const Bgzf *bgzf = nullptr;                              // non-null: `file_size` and every offset are in the uncompressed text
    bool dev_inflate = false; int inflate_helpers = 0;
    const TextPlan &P; const std::vector<salt_gpu_index_t *> &gix; const salt_aln_opt_t &ao; const salt_text_opt_t to; const double t0;
};

// One worker of the single-end text path.  A turn of run(): load() chunk k's bytes, cut() them at record starts, align(), write in turn.
struct SeWorker {
    TextRun &R; const SeText &S; const int wk;
    SeWorker(TextRun &r, const SeText &s, int w) : R(r), S(s), wk(w) {}
    salt_gpu_ws_t *ws = nullptr; uint32_t ws_reads = 0;
    std::vector<unsigned char> cbuf;                              // blocked gzip input: the compressed bytes of a chunk's blocks
    std::vector<char> win; std::vector<uint32_t> zc, zu;          // ... inflated on the device: the windows peeked from its text, the chunk's block offsets
    std::string zbuf;                                             // --bgzf with the host compressor: this worker's blocks
    // where load() left the chunk's text: n bytes at `text` in the worker's buffer (blocked input inflates whole blocks: the chunk's bytes then
    // start inside the buffer), or in the workspace with byte 0 at dev_base (on_dev); add_nl: byte n - 1 is a newline the device's text lacks
    char *text = nullptr; uint64_t dev_base = 0, n = 0; bool on_dev = false, add_nl = false;
    salt_gpu_index_t *gix() const { return S.gix[(size_t)(wk / S.P.wpg)]; }
    bool load(uint64_t rd_lo, uint64_t rd_hi);
    bool cut(uint64_t lo, uint64_t hi, uint64_t rd_lo, uint64_t *beg, uint64_t *end);
    int align(uint64_t k, uint64_t beg, uint64_t end, const char **sam, uint64_t *sam_bytes, uint32_t *n_reads);
    void run();
};

// Text bytes [rd_lo, rd_hi) of the input, three ways: pread from a plain file; blocked gzip inflated by this worker and its helpers; blocked
// gzip inflated on the device.  The file's last record gets the newline it may lack.  False: reported, and the run failed.
bool SeWorker::load(uint64_t rd_lo, uint64_t rd_hi)
{
    char *const buf = S.P.in_buf[(size_t)wk];
    text = buf; dev_base = 0; n = rd_hi - rd_lo; on_dev = add_nl = false;
    if (!S.bgzf) {
        if (pread_full(S.fd, buf, n, rd_lo) != n) { fprintf(stderr, "[salt] short read on %s\n", S.fn); R.fail(); return false; }
    } else {
        // the blocks that hold text bytes [rd_lo, rd_hi): read as one piece, inflated side by side by this worker and its helpers
        const Bgzf &B = *S.bgzf;
        const size_t b0 = (size_t)(std::upper_bound(B.uoff.begin(), B.uoff.end(), rd_lo) - B.uoff.begin()) - 1;
        size_t b1 = (size_t)(std::lower_bound(B.uoff.begin(), B.uoff.end(), rd_hi) - B.uoff.begin());
        if (b1 >= B.uoff.size()) b1 = B.uoff.size() - 1;
        const uint64_t c0 = B.coff[b0], c1 = B.coff[b1], u0 = B.uoff[b0];
        bool ok = B.uoff[b1] - u0 <= S.P.in_cap - 64;
        // on the device: the compressed blocks go into the page-locked buffer as they are (blocks that deflate did not shrink can
        // outgrow it by their headers: such a chunk is inflated here)
        on_dev = S.dev_inflate && ok && c1 - c0 <= S.P.in_cap - 64 && c1 - c0 < 0xFFFFFFFFull && B.uoff[b1] - u0 < 0xFFFFFFFFull;
        if (on_dev) {
            ok = pread_full(S.fd, buf, c1 - c0, c0) == c1 - c0;
            zc.resize(b1 - b0 + 1); zu.resize(b1 - b0 + 1);
            for (size_t b = b0; b <= b1; ++b) { zc[b - b0] = (uint32_t)(B.coff[b] - c0); zu[b - b0] = (uint32_t)(B.uoff[b] - u0); }
            if (ok) {
                const int zrc = salt_gpu_ws_inflate_bgzf(ws, buf, c1 - c0, (uint32_t)(b1 - b0), zc.data(), zu.data());
                if (zrc) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); if (zrc != SALT_E_DATA) { R.fail(); return false; } ok = false; }
            }
            dev_base = rd_lo - u0;
        } else if (ok) {
            cbuf.resize((size_t)(c1 - c0));
            std::atomic<size_t> nb{ b0 }; std::atomic<bool> bad{ pread_full(S.fd, cbuf.data(), c1 - c0, c0) != c1 - c0 };
            auto work = [&]() {
                for (;;) {
                    const size_t b = nb.fetch_add(1);
                    if (b >= b1 || bad) break;
                    if (!bgzf_inflate(cbuf.data() + (B.coff[b] - c0), (size_t)(B.coff[b + 1] - B.coff[b]), buf + (B.uoff[b] - u0), (size_t)(B.uoff[b + 1] - B.uoff[b]))) bad = true;
                }
            };
            std::vector<std::thread> helpers;
            for (int h = 0; h < S.inflate_helpers; ++h) helpers.emplace_back(work);
            work();
            for (auto &h : helpers) h.join();
            ok = !bad;
        }
        if (!ok) { fprintf(stderr, "[salt] %s: damaged or oversized gzip block near text offset %llu\n", S.fn, (unsigned long long)rd_lo); R.fail(); return false; }
        text = buf + (rd_lo - u0);
    }
    if (rd_hi == S.file_size && n) {                              // a last record without its newline
        char last = on_dev ? '\n' : text[n - 1];
        if (on_dev && salt_gpu_ws_text_peek(ws, dev_base + n - 1, 1, &last)) { R.fail_gpu(); return false; }
        if (last != '\n') { if (on_dev) add_nl = true; else text[n] = '\n'; ++n; }
    }
    return true;
}
// The chunk's records are those that start in file bytes [lo, hi): *beg and *end are the record starts at or after the two (offsets in the
// loaded text, which has one byte of context in front and TEXT_SLACK behind), cut on the host's text or from windows of the device's.
bool SeWorker::cut(uint64_t lo, uint64_t hi, uint64_t rd_lo, uint64_t *beg, uint64_t *end)
{
    const uint64_t b0 = lo - rd_lo;                               // offset of file byte `lo` in the text
    *end = n;
    if (on_dev) {
        bool pk = next_record_start_dev(ws, win, dev_base, n, add_nl, b0, lo == 0, beg);
        if (pk && hi < S.file_size) pk = next_record_start_dev(ws, win, dev_base, n, add_nl, hi - rd_lo, false, end);
        if (!pk) { R.fail_gpu(); return false; }
    } else {
        *beg = next_record_start(text, n, b0, lo == 0 || text[b0 - 1] == '\n');
        if (hi < S.file_size) *end = next_record_start(text, n, hi - rd_lo, text[hi - rd_lo - 1] == '\n');
    }
    if (hi < S.file_size && *end == n) { fprintf(stderr, "[salt] a FASTQ record longer than %llu bytes near offset %llu\n", (unsigned long long)TEXT_SLACK, (unsigned long long)hi); R.fail(); return false; }
    *beg = std::min(*beg, *end);
    return true;
}
// Text [beg, end) through the device, into a SAM block that lies in the workspace's (or the worker's page-locked) buffer.  A chunk with more
// reads than the workspace was made for has it re-created once, for the worst case.  Returns the device call's code.
int SeWorker::align(uint64_t k, uint64_t beg, uint64_t end, const char **sam, uint64_t *sam_bytes, uint32_t *n_reads)
{
    if (end <= beg) return 0;
    // (on the device the range ends with the text's own newline, or with the one put behind the file's last record)
    auto call = [&]() {
        if (!on_dev) return salt_gpu_align_se_text(ws, &S.ao, &S.to, text + beg, end - beg, sam, sam_bytes, n_reads);
        const bool nl = add_nl && end == n;
        return salt_gpu_align_se_text_dev(ws, &S.ao, &S.to, dev_base + beg, end - beg - (nl ? 1 : 0), nl ? 1 : 0, sam, sam_bytes, n_reads);
    };
    int grc = call();
    if (grc == SALT_E_CAPACITY && ws_reads < S.P.worst_reads) {                         // shorter records than the file's head promised
        if (getenv("SALT_TEXT_TRACE")) fprintf(stderr, "[salt] worker %d: chunk %llu holds more than %u reads, workspace re-created for %u\n", wk, (unsigned long long)k, ws_reads, S.P.worst_reads);
        trim_collect(ws); salt_gpu_ws_destroy(ws); ws = nullptr; ws_reads = S.P.worst_reads;
        grc = open_text_ws(gix(), ws_reads, &ws);
        if (!grc && on_dev) grc = salt_gpu_ws_inflate_bgzf(ws, S.P.in_buf[(size_t)wk], zc.back(), (uint32_t)(zc.size() - 1), zc.data(), zu.data());      // the new workspace's text
        if (!grc) grc = call();
    }
    return grc;
}

void SeWorker::run()
{
    pin_to_device_node(wk / S.P.wpg);
    const bool trace = getenv("SALT_TEXT_TRACE") != nullptr;      // per-worker timeline on stderr
    const double tw_start = now(); int n_calls = 0; double t_first = 0, t_rest = 0;
    ws_reads = S.P.max_reads;
    if (open_text_ws(gix(), ws_reads, &ws, &S.ao, &S.P, wk, S.chunk + TEXT_SLACK, (uint32_t)(ws_reads / 1.3))) { R.fail_gpu(); salt_gpu_ws_destroy(ws); return; }
    const double t_setup = now() - tw_start;
    for (;;) {
        const uint64_t k = R.next_chunk.fetch_add(1);
        if (k >= S.n_chunks || R.failed || R.fallback) break;
        // bytes [lo - 1, hi + slack) of the file: one byte of context in front (is `lo` a line start?), slack behind (where does the last record end?)
        const uint64_t lo = k * S.chunk, hi = std::min(S.file_size, lo + S.chunk);
        const uint64_t rd_lo = lo ? lo - 1 : 0, rd_hi = std::min(S.file_size, hi + TEXT_SLACK);
        const double tr0 = now(); uint64_t beg = 0, end = 0;
        if (!load(rd_lo, rd_hi)) break;
        if (!on_dev) R.t_read = R.t_read + (now() - tr0);
        if (!cut(lo, hi, rd_lo, &beg, &end)) break;
        if (on_dev) R.t_read = R.t_read + (now() - tr0);          // (the windows peeked from the device's text count as reading)
        const char *sam = nullptr; uint64_t sam_bytes = 0; uint32_t n_reads = 0;
        const double tg0 = now();
        const int grc = align(k, beg, end, &sam, &sam_bytes, &n_reads);
        if (grc && !parser_refused(grc)) { R.fail_gpu(); break; }
        if (grc) {
            // not strict 4-line FASTQ in this chunk: when the blocks before it are out, the host parser continues from its first record
            const std::string why = salt_gpu_last_error();
            if (R.claim_fallback(k)) {
                R.resume = rd_lo + beg;
                fprintf(stderr, "[salt] %s: the host parser takes over at byte %llu of %s\n", why.c_str(), (unsigned long long)R.resume, S.fn);
            }
            break;
        }
        R.t_gpu = R.t_gpu + (now() - tg0);
        if (n_calls++ == 0) t_first = now() - tg0; else t_rest += now() - tg0;
        const char *const lines = sam; const uint64_t lines_bytes = sam_bytes;      // (SAM lines whenever --snp-counts counts on the host)
        if (g_bgzf.on && !bgzf_text_block(sam, sam_bytes, zbuf)) { fprintf(stderr, "[salt] no BGZF blocks for a block of the output\n"); R.fail(); break; }
        if (!R.wait_turn(k)) { drop_block(ws); break; }
        if (!host_twins_add(lines, (size_t)lines_bytes)) { R.fail(); break; }
        if (!R.write_block(k, sam, sam_bytes, n_reads)) break;
    }
    if (trace) fprintf(stderr, "[salt] worker %d: started %.3f s after the clock, setup %.3f s, first device call %.3f s, %d later calls %.4f s each, done at %.3f s\n", wk,
                       tw_start - S.t0, t_setup, t_first, n_calls - 1, n_calls > 1 ? t_rest / (n_calls - 1) : 0.0, now() - S.t0);
    trim_collect(ws);
    salt_gpu_ws_destroy(ws);
}

// returns 0 = done, 1 = failed, 2 = *resume_off is where the host pipeline has to take over (everything before it is written)
static int run_se_text(const char *fn_reads, const std::vector<salt_gpu_index_t *> &gix, const Contigs &contigs, TextPlan &P,
                       const salt_aln_opt_t &ao, const salt_sam_opt_t &so, double t0, uint64_t *resume_off)
{
    SeText S{ fn_reads, open(fn_reads, O_RDONLY), 0, P.chunk, 0, nullptr, false, 0, P, gix, ao, { so.print_xa_cigar, so.print_nm_md, so.rg_id }, t0 };
    if (S.fd < 0) { fprintf(stderr, "[query_open]: file %s open fail!\n", fn_reads); return 1; }
    struct stat sb; if (fstat(S.fd, &sb) != 0) { fprintf(stderr, "[salt] cannot stat %s\n", fn_reads); return 1; }
    S.file_size = (uint64_t)sb.st_size;
    if (P.bgzf.ok) { S.bgzf = &P.bgzf; S.file_size = P.bgzf.uoff.back(); }
    S.n_chunks = (S.file_size + S.chunk - 1) / S.chunk;
    if (!text_begin(gix, contigs, P)) return 1;
    // blocked gzip input: every worker inflates with a few helper threads (a block inflates at ~0.3 GB/s on one core; a worker's chunk must
    // not take longer to inflate than the device takes for the chunks of the other workers)
    S.dev_inflate = S.bgzf && salt_gpu_ws_inflate_bgzf && salt_gpu_ws_text_peek && salt_gpu_align_se_text_dev &&
                    getenv("SALT_INFLATE_DEVICE") && atoi(getenv("SALT_INFLATE_DEVICE")) && !(getenv("SALT_INFLATE_HOST") && atoi(getenv("SALT_INFLATE_HOST")));
    if (S.bgzf) fprintf(stderr, "[salt] BGZF input: %s inflate, %llu blocks\n", S.dev_inflate ? "device" : "host", (unsigned long long)(S.bgzf->coff.size() - 1));
    if (S.bgzf) { S.inflate_helpers = 5; if (const char *e = getenv("SALT_INFLATE_HELPERS")) { const int v = atoi(e); if (v >= 0 && v <= 64) S.inflate_helpers = v; } }
    TextRun R(t0);
    std::vector<std::thread> workers;
    for (int wk = 0; wk < P.n_workers; ++wk) workers.emplace_back([&R, &S, wk]() { SeWorker(R, S, wk).run(); });
    for (auto &w : workers) w.join();
    close(S.fd);
    if (!R.failed && R.fallback) { *resume_off = R.resume; return 2; }
    const double dt = R.t_last.load() - t0;                 // first chunk claimed .. last SAM byte written (releasing the workspaces is not alignment time)
    fprintf(stderr, "[alnse_core]: total %lf sec escaped\n", dt);
    fprintf(stderr, "[salt] text path: %d worker(s), chunk %llu MiB, blocks written in turn; seconds summed over workers: read %.3f device call %.3f write %.3f "
                    "(page-locked buffers: %.3f s, while the index was loading)\n", P.n_workers, (unsigned long long)(S.chunk >> 20), R.t_read.load(), R.t_gpu.load(), R.t_write.load(), P.alloc_s);
    fprintf(stderr, "[salt] %ld reads, %.3f Mreads/s end to end (FASTQ -> SAM, %d GPU(s))\n", R.reads_done, dt > 0 ? R.reads_done / dt / 1e6 : 0.0, (int)gix.size());
    return R.failed ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// Paired end, two plain 4-line FASTQ files: the same path with chunks cut by RECORD COUNT.  One scanner thread per file counts newlines
// (8 bytes per step) and publishes the byte offset of every pairs_per_chunk-th record; a worker takes chunk k of both files as soon
// as both offsets are there, calls salt_gpu_align_pe_text and writes its block in turn.
// ---------------------------------------------------------------------------------------------
struct PeScan {                                             // guarded by the run's mutex, announced on its condition variable
    std::vector<uint64_t> off[2];                           // off[f][k] = start of chunk k in file f; the last entry of a finished file = its size
    bool done[2] = { false, false }; uint64_t records[2] = { 0, 0 };
    bool bad = false;
};

static inline uint64_t count_nl8(uint64_t w)               // newlines among the 8 bytes of w
{
    const uint64_t x = w ^ 0x0A0A0A0A0A0A0A0Aull, m = 0x7F7F7F7F7F7F7F7Full;
    const uint64_t y = ~(((x & m) + m) | x | m);            // bit 7 of every byte that is zero in x
    return (uint64_t)__builtin_popcountll(y);
}

// The chunk boundaries of one file of a pair: chunk k starts where line 4 k pairs_per_chunk starts.  Counting lines is a pass over the
// whole file, and one thread counts ~4 GB/s -- 30 M mates/s of 150-base pairs, less than one GPU aligns.  So the file goes in segments of
// 32 MiB to PE_SCAN_THREADS threads: each counts its segment's newlines, learns how many lines lie in front of it once the segments before
// it are counted (a running sum kept under the scan's mutex), finds the chunk starts that fall inside its segment in the bytes it still
// holds, and publishes them after the segment before it has published its own.
static const int PE_SCAN_THREADS = 4;
static void pe_scan_file(const char *fn, int f, uint64_t pairs_per_chunk, PeScan &S, TextRun &R)
{
    const int fd = open(fn, O_RDONLY);
    const uint64_t lines_per_chunk = 4 * pairs_per_chunk;
    if (fd < 0) { { std::lock_guard<std::mutex> lk(R.mu); S.bad = true; S.done[f] = true; } R.cv.notify_all(); return; }
    struct stat st;
    const uint64_t size = fstat(fd, &st) == 0 ? (uint64_t)st.st_size : 0;
    { std::lock_guard<std::mutex> lk(R.mu); S.off[f].push_back(0); }
    R.cv.notify_all();
    uint64_t SEG = 32ull << 20;
    if (const char *e = getenv("SALT_PE_SCAN_SEG_BYTES")) { const long long v = atoll(e); if (v >= 64) SEG = (uint64_t)v; }      // tests: many segments in a small file
    const uint64_t n_seg = (size + SEG - 1) / SEG;
    std::mutex mu; std::condition_variable cv;               // the order among this file's segments
    std::vector<int64_t> cnt((size_t)n_seg, -1);             // newlines of a segment, once counted
    std::vector<uint64_t> before((size_t)n_seg + 1, 0);      // lines in front of a segment, known for segments < known
    uint64_t known = 0, published = 0;                       // segments whose `before` is known / whose boundaries are out
    std::atomic<uint64_t> next_seg{ 0 };
    std::atomic<bool> short_read{ false };
    char last_byte = '\n';
    auto work = [&]() {
        std::vector<char> buf((size_t)SEG);
        for (;;) {
            const uint64_t sg = next_seg.fetch_add(1);
            if (sg >= n_seg || R.failed) break;
            const uint64_t lo = sg * SEG, want = std::min<uint64_t>(SEG, size - lo);
            const uint64_t got = pread_full(fd, buf.data(), want, lo);
            if (got != want) short_read = true;               // (the file shrank under us: the workers' own reads will fail on it)
            uint64_t c = 0; size_t j = 0;
            for (; j + 8 <= (size_t)got; j += 8) { uint64_t w; memcpy(&w, buf.data() + j, 8); c += count_nl8(w); }
            for (; j < (size_t)got; ++j) c += buf[j] == '\n';
            uint64_t l0;
            {
                std::unique_lock<std::mutex> lk(mu);
                cnt[(size_t)sg] = (int64_t)c;
                while (known < n_seg && cnt[(size_t)known] >= 0) { before[(size_t)known + 1] = before[(size_t)known] + (uint64_t)cnt[(size_t)known]; ++known; }
                cv.notify_all();
                while (known <= sg && !R.failed) cv.wait_for(lk, std::chrono::milliseconds(50));      // (a failed run notifies nobody here)
                if (known <= sg) break;
                l0 = before[(size_t)sg];
                if (sg + 1 == n_seg && got) last_byte = buf[(size_t)got - 1];
            }
            // chunk starts inside this segment: the byte behind the newline that completes line m * lines_per_chunk, l0 < m * lpc <= l0 + c
            std::vector<uint64_t> mine;
            uint64_t nextb = (l0 / lines_per_chunk + 1) * lines_per_chunk, lines = l0;
            for (size_t i = 0; i < (size_t)got && nextb <= l0 + c; ) {
                const size_t piece = std::min<size_t>(4096, (size_t)got - i);
                uint64_t pc = 0; size_t q = 0;
                for (; q + 8 <= piece; q += 8) { uint64_t w; memcpy(&w, buf.data() + i + q, 8); pc += count_nl8(w); }
                for (; q < piece; ++q) pc += buf[i + q] == '\n';
                if (lines + pc < nextb) { lines += pc; i += piece; continue; }
                for (q = 0; q < piece; ++q)
                    if (buf[i + q] == '\n' && ++lines == nextb) { mine.push_back(lo + i + q + 1); nextb += lines_per_chunk; }
                i += piece;
            }
            {
                std::unique_lock<std::mutex> lk(mu);
                while (published != sg && !R.failed) cv.wait_for(lk, std::chrono::milliseconds(50));
                if (published != sg) break;
                if (!mine.empty()) {
                    { std::lock_guard<std::mutex> lk2(R.mu); for (uint64_t o : mine) if (o < size) S.off[f].push_back(o); }      // (a start at the very end is the file's end, added below)
                    R.cv.notify_all();
                }
                published = sg + 1;
                cv.notify_all();
            }
        }
    };
    std::vector<std::thread> th;
    const int nt = (int)std::min<uint64_t>((uint64_t)PE_SCAN_THREADS, std::max<uint64_t>(n_seg, 1));
    for (int t = 0; t < nt; ++t) th.emplace_back(work);
    for (auto &t : th) t.join();
    close(fd);
    uint64_t lines = known == n_seg ? before[(size_t)n_seg] : 0;
    if (size && last_byte != '\n') ++lines;                   // a last line without its newline
    {
        std::lock_guard<std::mutex> lk(R.mu);
        if (S.off[f].back() != size) S.off[f].push_back(size);
        S.records[f] = lines / 4; S.done[f] = true;
        if (lines % 4 || short_read || (R.failed && known != n_seg)) S.bad = true;
    }
    R.cv.notify_all();
}

// returns 0 = done, 1 = failed, 2 = the host pipeline has to take over at resume_off[0 / 1] of the two files (everything before is written):
// a chunk the device parser refused, a file whose line count is not a multiple of four (a trailing blank line is fine for kseq.h), or files
// with different numbers of chunks -- the host parser reads what the reference reads and reports what it cannot
static int run_pe_text(const char *fn1, const char *fn2, const std::vector<salt_gpu_index_t *> &gix, const Contigs &contigs, TextPlan &P,
                       const salt_aln_opt_t &ao, const salt_sam_opt_t &so, const salt_pe_opt_t &po, double t0, uint64_t resume_off[2])
{
    const int fd[2] = { open(fn1, O_RDONLY), open(fn2, O_RDONLY) };
    if (fd[0] < 0 || fd[1] < 0) { fprintf(stderr, "[query_open]: file %s open fail!\n", fd[0] < 0 ? fn1 : fn2); return 1; }
    if (!text_begin(gix, contigs, P)) return 1;
    const salt_text_opt_t to = { so.print_xa_cigar, so.print_nm_md, so.rg_id };
    PeScan S; TextRun R(t0);
    auto fall_back = [&](uint64_t k, const std::string &why) {
        if (R.claim_fallback(k)) { R.resume = k; fprintf(stderr, "[salt] %s: the host parser takes over at pair chunk %llu\n", why.c_str(), (unsigned long long)k); }
    };
    std::thread scan1(pe_scan_file, fn1, 0, P.pairs_per_chunk, std::ref(S), std::ref(R)), scan2(pe_scan_file, fn2, 1, P.pairs_per_chunk, std::ref(S), std::ref(R));
    std::vector<std::thread> workers;
    for (int wk = 0; wk < P.n_workers; ++wk)
        workers.emplace_back([&, wk]() {
            salt_gpu_ws_t *ws = nullptr; char *buf = P.in_buf[(size_t)wk]; std::string zbuf;
            pin_to_device_node(wk / P.wpg);
            if (open_text_ws(gix[(size_t)(wk / P.wpg)], P.max_reads + 64, &ws, &ao, &P, wk, P.in_cap, P.max_reads)) { R.fail_gpu(); salt_gpu_ws_destroy(ws); return; }
            for (;;) {
                const uint64_t k = R.next_chunk.fetch_add(1);
                uint64_t lo[2], hi[2]; bool end = false, odd = false;
                {   // chunk k of both files: its start and end offsets (or the news that there is no chunk k)
                    std::unique_lock<std::mutex> lk(R.mu);
                    R.cv.wait(lk, [&] { return R.failed || R.fallback || ((S.off[0].size() > k + 1 || S.done[0]) && (S.off[1].size() > k + 1 || S.done[1])); });
                    if (R.failed || R.fallback) break;
                    if (S.bad) odd = true;
                    else if (S.off[0].size() <= k + 1 || S.off[1].size() <= k + 1) {
                        // one file has no chunk k: fine if neither has (both finished with the same number of chunks), else the files differ
                        if ((S.off[0].size() > k + 1) != (S.off[1].size() > k + 1)) { S.bad = true; odd = true; }
                        else end = true;
                    } else for (int f = 0; f < 2; ++f) { lo[f] = S.off[f][k]; hi[f] = S.off[f][k + 1]; }
                }
                if (end) break;
                if (odd) { fall_back(k, "the read files are not two equally long runs of 4-line records"); break; }
                const uint64_t n1 = hi[0] - lo[0], n2 = hi[1] - lo[1], b2 = (n1 + 64) & ~63ull;
                if (b2 + n2 + 2 > P.in_cap) { fprintf(stderr, "[salt] a chunk of %llu pairs is larger than its buffer (records much longer than the file's first ones)\n", (unsigned long long)P.pairs_per_chunk); R.fail(); break; }
                const double tr0 = now();
                if (pread_full(fd[0], buf, n1, lo[0]) != n1 || pread_full(fd[1], buf + b2, n2, lo[1]) != n2) { fprintf(stderr, "[salt] short read on the FASTQ files\n"); R.fail(); break; }
                uint64_t m1 = n1, m2 = n2;
                if (m1 && buf[m1 - 1] != '\n') buf[m1++] = '\n';                              // a last record without its newline
                if (m2 && buf[b2 + m2 - 1] != '\n') buf[b2 + m2++] = '\n';
                R.t_read = R.t_read + (now() - tr0);
                const char *sam = nullptr; uint64_t sam_bytes = 0; uint32_t n_pairs = 0;
                const double tg0 = now();
                const int grc = salt_gpu_align_pe_text(ws, &ao, &po, &to, buf, m1, buf + b2, m2, &sam, &sam_bytes, &n_pairs);
                if (grc && !parser_refused(grc)) { R.fail_gpu(); break; }
                if (grc) { fall_back(k, salt_gpu_last_error()); break; }
                R.t_gpu = R.t_gpu + (now() - tg0);
                const char *const lines = sam; const uint64_t lines_bytes = sam_bytes;
                if (g_bgzf.on && !bgzf_text_block(sam, sam_bytes, zbuf)) { fprintf(stderr, "[salt] no BGZF blocks for a block of the output\n"); R.fail(); break; }
                if (!R.wait_turn(k)) { drop_block(ws); break; }
                if (!host_twins_add(lines, (size_t)lines_bytes)) { R.fail(); break; }
                if (!R.write_block(k, sam, sam_bytes, 2 * (long)n_pairs)) break;
            }
            trim_collect(ws);
            salt_gpu_ws_destroy(ws);
        });
    for (auto &w : workers) w.join();
    scan1.join(); scan2.join();
    close(fd[0]); close(fd[1]);
    if (!R.failed && R.fallback) {
        for (int f = 0; f < 2; ++f) resume_off[f] = S.off[f].size() > R.resume ? S.off[f][R.resume] : (S.off[f].empty() ? 0 : S.off[f].back());
        return 2;
    }
    if (!R.failed && (S.bad || S.records[0] != S.records[1])) {
        fprintf(stderr, "[salt] the two read files hold different numbers of reads (%llu / %llu) or broken records\n", (unsigned long long)S.records[0], (unsigned long long)S.records[1]);
        return 1;
    }
    const long pairs_done = R.reads_done / 2;
    const double dt = R.t_last.load() - t0;
    fprintf(stderr, "[alnpe_core]: total %lf sec escaped\n", dt);
    fprintf(stderr, "[salt] text path (paired end): %d worker(s), %llu pairs per chunk, blocks written in turn; seconds summed over workers: read %.3f device call %.3f write %.3f "
                    "(page-locked buffers: %.3f s, while the index was loading)\n", P.n_workers, (unsigned long long)P.pairs_per_chunk, R.t_read.load(), R.t_gpu.load(), R.t_write.load(), P.alloc_s);
    fprintf(stderr, "[salt] %ld pairs, %.3f M mates/s end to end (FASTQ -> SAM, %d GPU(s))\n", pairs_done, dt > 0 ? 2.0 * pairs_done / dt / 1e6 : 0.0, (int)gix.size());
    return R.failed ? 1 : 0;
}

// pair i of a batch and its mate batch = reads 2i, 2i + 1 of iseq / ioff
static void interleave_mates(const Batch &b, const Batch &m, std::vector<uint8_t> &iseq, std::vector<uint32_t> &ioff)
{
    const size_t n = (size_t)b.n();
    ioff.assign(2 * n + 1, 0);
    iseq.resize(b.seqs.size() + m.seqs.size());
    for (size_t i = 0; i < n; ++i) {
        const uint32_t l0 = b.offs[i + 1] - b.offs[i], l1 = m.offs[i + 1] - m.offs[i];
        memcpy(iseq.data() + ioff[2 * i], b.seqs.data() + b.offs[i], l0); ioff[2 * i + 1] = ioff[2 * i] + l0;
        memcpy(iseq.data() + ioff[2 * i + 1], m.seqs.data() + m.offs[i], l1); ioff[2 * i + 2] = ioff[2 * i + 1] + l1;
    }
}
// the quality bytes of a parsed batch in the layout of the bases handed to the device: read i's at offs[i], mates interleaved as interleave_mates does
static void batch_quals(const Batch &b, const Batch *m, std::vector<uint8_t> &q)
{
    const size_t n = (size_t)b.n();
    q.resize(b.seqs.size() + (m ? m->seqs.size() : 0));
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t l0 = b.offs[i + 1] - b.offs[i];
        memcpy(q.data() + at, b.raw.data() + b.qual[i], l0); at += l0;
        if (!m) continue;
        const uint32_t l1 = m->offs[i + 1] - m->offs[i];
        memcpy(q.data() + at, m->raw.data() + m->qual[i], l1); at += l1;
    }
}
struct Opts {
    int n_threads = 1, n_gpus = 1, overlap = -1, pe = 0;
    salt_aln_opt_t ao{}; salt_sam_opt_t so{};
    salt_pe_opt_t po = { 250, 550 };                                       // aln.c:43-44
    std::string cmd; const char *prefix = nullptr, *fn_reads = nullptr, *fn_mates = nullptr;
};

// the command line into o (and g_bgzf, g_bam, g_polish); returns -1 to go on, else the exit code
static int parse_options(int argc, char **argv, Opts &o)
{
    o.ao.max_seed = 50; o.ao.max_locate = 1000; o.ao.max_hits = 5;       // aln.c:46-47, aln.h:133
    for (int i = 0; i < argc; ++i) { if (i) o.cmd += " "; o.cmd += argv[i]; }
    static const struct option lo[] = {
        { "threads", 1, 0, 't' }, { "num", 1, 0, 'n' }, { "help", 0, 0, 'h' }, { "pe", 0, 0, 'p' }, { "min_tlen", 1, 0, 'a' },
        { "max_tlen", 1, 0, 'b' }, { "group", 1, 0, 'g' }, { "sw", 0, 0, 'e' }, { "max_locate", 1, 0, 'm' }, { "max_seed", 1, 0, 's' },
        { "read_length", 1, 0, 'l' }, { "overlap", 1, 0, 'r' }, { "xa_cigar", 0, 0, 'c' }, { "md", 0, 0, 'd' }, { "ref", 0, 0, 'v' },
        { "mismatch", 1, 0, 'M' }, { "gapop", 1, 0, 'O' }, { "gapex", 1, 0, 'E' }, { "extend", 1, 0, 'X' }, { "gpus", 1, 0, 1000 }, { "bgzf", 0, 0, 1001 }, { "bam", 0, 0, 1002 }, { "polish", 2, 0, 1003 },
        { "snp-counts", 1, 0, 1004 }, { "snp-min-mapq", 1, 0, 1005 }, { "depth", 1, 0, 1006 }, { "depth-min-mapq", 1, 0, 1007 }, { "depth-window", 1, 0, 1008 },
        { "error-profile", 1, 0, 1009 }, { "error-profile-min-mapq", 1, 0, 1010 }, { "error-profile-full", 0, 0, 1011 },
        { "genotype", 1, 0, 1012 }, { "genotype-min-mapq", 1, 0, 1013 }, { "genotype-sample", 1, 0, 1014 },
        { "discover", 1, 0, 1015 }, { "discover-min-mapq", 1, 0, 1016 }, { "discover-min-baseq", 1, 0, 1017 }, { "discover-min-alt", 1, 0, 1018 }, { "discover-min-pct", 1, 0, 1019 },
        { "discover-all", 0, 0, 1020 }, { "stats", 1, 0, 1021 }, { "stats-min-mapq", 1, 0, 1022 },
        { "indels", 1, 0, 1023 }, { "indels-min-mapq", 1, 0, 1024 }, { "indels-min-alt", 1, 0, 1025 }, { "indels-min-pct", 1, 0, 1026 }, { "indels-slots", 1, 0, 1027 },
        { "trim-adapter", 1, 0, 1028 }, { "trim-adapter2", 1, 0, 1029 }, { "trim-qual", 1, 0, 1030 }, { "trim-front", 1, 0, 1031 }, { "trim-tail", 1, 0, 1032 },
        { "trim-min-overlap", 1, 0, 1033 }, { "trim-error-pct", 1, 0, 1034 },
        { "trim-pair-overlap", 0, 0, 1035 }, { "trim-pair-min-overlap", 1, 0, 1036 }, { "trim-pair-error-pct", 1, 0, 1037 }, { 0, 0, 0, 0 } };
    for (int c; (c = getopt_long(argc, argv, "t:n:hpa:b:g:em:s:l:cdr:vM:O:E:X:", lo, nullptr)) >= 0; ) {
        switch (c) {
        case 't': o.n_threads = atoi(optarg); break;
        case 'g': o.so.rg_id = optarg; break;
        case 's': o.ao.max_seed = (uint32_t)atoi(optarg); break;
        case 'm': o.ao.max_locate = (uint32_t)atoi(optarg); break;
        case 'c': o.so.print_xa_cigar = 1; break;
        case 'd': o.so.print_nm_md = 1; break;
        case 'v': o.ao.seed_only_ref = 1; break;
        case 'r': o.overlap = atoi(optarg); break;
        case 'p': o.pe = 1; break;
        case 'a': o.po.min_tlen = (uint32_t)atoi(optarg); break;
        case 'b': o.po.max_tlen = (uint32_t)atoi(optarg); break;
        case 1000: o.n_gpus = atoi(optarg); break;
        case 1001: g_bgzf.on = true; break;
        case 1002: g_bam.on = true; g_bgzf.on = true; break;
        case 1003:
            if (!optarg || strcmp(optarg, "lv") == 0) g_polish = 1;
            else if (strcmp(optarg, "sw") == 0) g_polish = 2;
            else { fprintf(stderr, "[opt_parse]: --polish=%s: the re-scoring is lv (Landau-Vishkin, the default) or sw (Smith-Waterman)\n", optarg); return 1; }
            break;
        case 1004: g_snp.on = true; g_snp.fn = optarg; break;
        case 1005: case 1007: case 1010: case 1013: case 1016: case 1022: case 1024: {
            const Tally &t = TALLIES[c == 1005 ? 0 : c == 1007 ? 1 : c == 1010 ? 2 : c == 1013 ? 3 : c == 1016 ? 4 : c == 1022 ? 5 : 6];
            char *end = nullptr; const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || v < 0 || v > 255) { fprintf(stderr, "[opt_parse]: --%s-min-mapq %s: a MAPQ is a number from 0 to 255\n", t.stem, optarg); return 1; }
            t.run->min_mapq = (uint32_t)v;
            break;
        }
        case 1006: g_depth.on = true; g_depth.fn = optarg; break;
        case 1008: {
            char *end = nullptr; errno = 0; const long long v = strtoll(optarg, &end, 10);
            if (end == optarg || *end || errno || v < 1 || v > 0xFFFFFFFFll) { fprintf(stderr, "[opt_parse]: --depth-window %s: a window is a number of positions from 1 to 4294967295\n", optarg); return 1; }
            g_depth.window = (uint32_t)v;
            break;
        }
        case 1009: g_errprof.on = true; g_errprof.fn = optarg; break;
        case 1011: g_errprof.full = true; break;
        case 1012: g_gt.on = true; g_gt.fn = optarg; break;
        case 1014:
            if (!*optarg || strpbrk(optarg, "\t\n\r")) { fprintf(stderr, "[opt_parse]: --genotype-sample: a sample name is not empty and holds no tab or line end\n"); return 1; }
            g_gt.sample = optarg;
            break;
        case 1015: g_disc.on = true; g_disc.fn = optarg; break;
        case 1017: case 1018: case 1019: {
            const char *name = c == 1017 ? "baseq" : c == 1018 ? "alt" : "pct";
            const long lo = c == 1018 ? 1 : 0, hi = c == 1017 ? 93 : c == 1018 ? 2097151 : 100;
            char *end = nullptr; errno = 0; const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || errno || v < lo || v > hi) { fprintf(stderr, "[opt_parse]: --discover-min-%s %s: a number from %ld to %ld\n", name, optarg, lo, hi); return 1; }
            (c == 1017 ? g_disc.min_baseq : c == 1018 ? g_disc.min_alt : g_disc.min_pct) = (uint32_t)v;
            break;
        }
        case 1020: g_disc.all = true; break;
        case 1021: g_stats.on = true; g_stats.fn = optarg; break;
        case 1023: g_indel.on = true; g_indel.fn = optarg; break;
        case 1025: case 1026: {
            const long long lo = c == 1025 ? 1 : 0, hi = c == 1025 ? 0xFFFFFFFFll : 100;
            char *end = nullptr; errno = 0; const long long v = strtoll(optarg, &end, 10);
            if (end == optarg || *end || errno || v < lo || v > hi) { fprintf(stderr, "[opt_parse]: --indels-min-%s %s: a number from %lld to %lld\n", c == 1025 ? "alt" : "pct", optarg, lo, hi); return 1; }
            (c == 1025 ? g_indel.min_alt : g_indel.min_pct) = (uint32_t)v;
            break;
        }
        case 1027: {
            char *end = nullptr; errno = 0; const long long v = strtoll(optarg, &end, 10);
            uint32_t lg = 0;
            while (lg < 63 && (1ll << lg) < v) ++lg;
            if (end == optarg || *end || errno || v < 64 || v > (1ll << 28) || (1ll << lg) != v) { fprintf(stderr, "[opt_parse]: --indels-slots %s: a power of two from 64 to 268435456\n", optarg); return 1; }
            g_indel.log2_slots = lg;
            break;
        }
        case 1028: case 1029: {
            const char *name = c == 1028 ? "adapter" : "adapter2";
            const size_t n = strlen(optarg);
            if (n < 1 || n > 64 || strspn(optarg, "ACGTacgt") != n) { fprintf(stderr, "[opt_parse]: --trim-%s %s: 1 to 64 letters of ACGT\n", name, optarg); return 1; }
            if (c == 1028) { g_trim.opt.adapter = optarg; g_trim.opt.adapter_len = (uint32_t)n; } else { g_trim.opt.adapter2 = optarg; g_trim.opt.adapter2_len = (uint32_t)n; }
            break;
        }
        case 1030: case 1031: case 1032: case 1033: case 1034: {
            static const struct { const char *name; long lo, hi; } F[5] = { { "qual", 1, 93 }, { "front", 0, 511 }, { "tail", 0, 511 }, { "min-overlap", 1, 64 }, { "error-pct", 0, 50 } };
            char *end = nullptr; errno = 0; const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || errno || v < F[c - 1030].lo || v > F[c - 1030].hi) { fprintf(stderr, "[opt_parse]: --trim-%s %s: a number from %ld to %ld\n", F[c - 1030].name, optarg, F[c - 1030].lo, F[c - 1030].hi); return 1; }
            (c == 1030 ? g_trim.opt.qual : c == 1031 ? g_trim.opt.front : c == 1032 ? g_trim.opt.tail : c == 1033 ? g_trim.opt.min_overlap : g_trim.opt.error_pct) = (uint32_t)v;
            if (c == 1033) g_trim.has_overlap = true;
            if (c == 1034) g_trim.has_error = true;
            break;
        }
        case 1035: g_trim.pair_on = true; break;
        case 1036: case 1037: {
            const char *name = c == 1036 ? "min-overlap" : "error-pct"; const long lo = c == 1036 ? 1 : 0, hi = c == 1036 ? 512 : 50;
            char *end = nullptr; errno = 0; const long v = strtol(optarg, &end, 10);
            if (end == optarg || *end || errno || v < lo || v > hi) { fprintf(stderr, "[opt_parse]: --trim-pair-%s %s: a number from %ld to %ld\n", name, optarg, lo, hi); return 1; }
            if (c == 1036) { g_trim.pair_opt.min_overlap = (uint32_t)v; g_trim.has_pair_overlap = true; } else { g_trim.pair_opt.error_pct = (uint32_t)v; g_trim.has_pair_error = true; }
            break;
        }
        case 'h': return usage();
        case '?': fprintf(stderr, "[ERROR]: no arg %c\n", optopt); return 1;
        default: break;
        }
    }
    if (g_polish && g_bam.on) { fprintf(stderr, "[opt_parse]: --polish and --bam cannot be combined: polished records are written as text only (--polish --bgzf compresses them)\n"); return 1; }
    if (g_trim.opt.adapter2 && !g_trim.opt.adapter) { fprintf(stderr, "[opt_parse]: --trim-adapter2 needs --trim-adapter (the adapter of mate 1; without --trim-adapter2 mate 2 is searched with it too)\n"); return 1; }
    if ((g_trim.has_overlap || g_trim.has_error) && !g_trim.opt.adapter) { fprintf(stderr, "[opt_parse]: --trim-%s belongs to the adapter search: give --trim-adapter (1 to 64 letters of ACGT)\n", g_trim.has_overlap ? "min-overlap" : "error-pct"); return 1; }
    if (g_trim.opt.adapter) { if (!g_trim.has_overlap) g_trim.opt.min_overlap = 5; if (!g_trim.has_error) g_trim.opt.error_pct = 10; }
    if ((g_trim.has_pair_overlap || g_trim.has_pair_error) && !g_trim.pair_on) { fprintf(stderr, "[opt_parse]: --trim-pair-%s belongs to the search for the mates' overlap: give --trim-pair-overlap\n", g_trim.has_pair_overlap ? "min-overlap" : "error-pct"); return 1; }
    if (g_trim.pair_on && !o.pe) { fprintf(stderr, "[opt_parse]: --trim-pair-overlap needs the mates: paired end (-p) and a second read file\n"); return 1; }
    if (g_trim.pair_on) { if (!g_trim.has_pair_overlap) g_trim.pair_opt.min_overlap = 20; if (!g_trim.has_pair_error) g_trim.pair_opt.error_pct = 10; }
    g_trim.on = g_trim.opt.adapter || g_trim.opt.qual || g_trim.opt.front || g_trim.opt.tail;
    g_trim.device = g_trim.any() && salt_gpu_ws_set_trim != nullptr && salt_gpu_ws_trim_counts != nullptr && salt_gpu_ws_trim_uncount != nullptr &&
                    (!g_trim.pair_on || (salt_gpu_ws_set_trim_pair != nullptr && salt_gpu_ws_trim_pair_counts != nullptr)) && !(getenv("SALT_TRIM_HOST") && atoi(getenv("SALT_TRIM_HOST")));
    if (optind + 2 + o.pe > argc) { fprintf(stderr, "[opt_parse]: index prefix and read file can't be omited!\n"); return 1; }
    if (o.n_threads < 1) o.n_threads = 1;
    if (o.n_gpus < 1) o.n_gpus = 1;
    o.prefix = argv[optind]; o.fn_reads = argv[optind + 1]; o.fn_mates = o.pe ? argv[optind + 2] : nullptr;
    // the device compressor, unless this libsalt_gpu has none or SALT_BGZF_HOST=1 asks for zlib (A/B runs, tests)
    g_bgzf.device = g_bgzf.on && salt_gpu_ws_set_sam_bgzf != nullptr && !(getenv("SALT_BGZF_HOST") && atoi(getenv("SALT_BGZF_HOST")));
    // the device's record kernels, unless this libsalt_gpu has none or SALT_BAM_HOST=1 asks for the host encoder; records made on the host
    // out of the device's SAM text are deflated there too
    g_bam.device = g_bam.on && salt_gpu_ws_set_sam_bam != nullptr && !(getenv("SALT_BAM_HOST") && atoi(getenv("SALT_BAM_HOST")));
    if (g_bam.on && !g_bam.device) g_bgzf.device = false;
    for (const Tally &t : TALLIES) {
        TallyRun &r = *t.run;
        if (!r.on) continue;
        r.device = t.symbols();
        // made on the host: from SAM lines, so the blocks reach the host as SAM lines and become records and BGZF blocks there
        if (!r.device && g_polish) { fprintf(stderr, "[opt_parse]: --%s with --polish needs a libsalt_gpu that %s on the device: this one does not, and no SAM lines exist under --polish\n", t.opt, t.does); return 1; }
        if (!r.device) g_bgzf.device = g_bam.device = false;
        if (!(r.fp = fopen(r.fn, t.mode))) { fprintf(stderr, "[opt_parse]: --%s: cannot open %s for writing: %s\n", t.opt, r.fn, strerror(errno)); return 1; }
    }
    const size_t l = g_depth.on ? strlen(g_depth.fn) : 0;
    g_depth.gz = l > 3 && strcmp(g_depth.fn + l - 3, ".gz") == 0;
    const size_t lg = g_gt.on ? strlen(g_gt.fn) : 0;
    g_gt.gz = lg > 3 && strcmp(g_gt.fn + lg - 3, ".gz") == 0;
    const size_t ld = g_disc.on ? strlen(g_disc.fn) : 0;
    g_disc.gz = ld > 3 && strcmp(g_disc.fn + ld - 3, ".gz") == 0;
    const size_t li = g_indel.on ? strlen(g_indel.fn) : 0;
    g_indel.gz = li > 3 && strcmp(g_indel.fn + li - 3, ".gz") == 0;
    return -1;
}

// aln_samhead (sam.c:56-84)
static bool print_header(const salt_index_t *ix, const Opts &o)
{
    if (g_polish) return true;                              // `polish` prints no header
    std::vector<char> hb(16 << 20);
    int w = salt_sam_header(ix, &o.so, hb.data(), hb.size());
    if (w < 0) { fprintf(stderr, "[salt] SAM header too large\n"); return false; }
    time_t tt = time(nullptr); struct tm *tmv = localtime(&tt);
    std::vector<char> pg(o.cmd.size() + 128);
    const int wp = snprintf(pg.data(), pg.size(), "@PG\tID:snpaln\tPN:snpaln\tCL:\"%s\"\tDS:%d-%d-%d\tVN:0.1beta\n", o.cmd.c_str(), tmv->tm_year + 1900, tmv->tm_mon + 1, tmv->tm_mday);
    if (!g_bgzf.on) { fwrite(hb.data(), 1, (size_t)w, stdout); fwrite(pg.data(), 1, (size_t)wp, stdout); return true; }
    std::string text(hb.data(), (size_t)w), z;
    text.append(pg.data(), (size_t)wp);
    if (g_bam.on) {                                          // the same text inside the BAM header, then the reference list of the same contig table
        std::string bh(text.size() + (size_t)w + 64 + 16 * (size_t)salt_index_n_seqs(ix), '\0');
        const int64_t wb = salt_bam_header(ix, text.data(), text.size(), reinterpret_cast<uint8_t *>(&bh[0]), bh.size());
        if (wb < 0) { fprintf(stderr, "[salt] BAM header too large\n"); return false; }
        bh.resize((size_t)wb);
        text.swap(bh);
    }
    if (!bgzf_deflate_host(text.data(), text.size(), z)) { fprintf(stderr, "[salt] zlib failed on the SAM header\n"); return false; }
    fwrite(z.data(), 1, z.size(), stdout);
    g_bgzf.text_bytes += text.size(); g_bgzf.file_bytes += z.size();
    return true;
}

// N3: -b 0 = infer the insert-size window from the first batch (N_SEQS / 2 pairs), the mates aligned as single-end reads
// (salt_isize_infer; the reference prints "infer isize func haven't been implemented" here, alnpe.c:586-589)
static bool infer_isize(Opts &o, const salt_index_t *ix, salt_gpu_index_t *gix)
{
    gzFile g1 = gzopen(o.fn_reads, "r"), g2 = gzopen(o.fn_mates, "r");
    if (!g1 || !g2) { fprintf(stderr, "[query_open]: file %s open fail!\n", g1 ? o.fn_mates : o.fn_reads); return false; }
    RawReader r1(g1, !sniff_four_line(o.fn_reads)), r2(g2, !sniff_four_line(o.fn_mates));
    Batch b1, b2; Pool pool(o.n_threads < 16 ? o.n_threads : 16);
    const int got = r1.take(b1.raw, N_SEQS / 2, b1.rec);
    if (got == 0 || r2.take(b2.raw, got, b2.rec) != got) { fprintf(stderr, "[salt] the two read files hold different numbers of reads\n"); return false; }
    parse_batch_pe(b1, b2, pool, false);
    std::vector<uint8_t> iseq; std::vector<uint32_t> ioff;
    interleave_mates(b1, b2, iseq, ioff);
    gzclose(g1); gzclose(g2);
    salt_gpu_ws_t *w0 = nullptr;
    std::vector<salt_result_t> r((size_t)2 * got);
    if (salt_gpu_ws_create(gix, (uint32_t)(2 * got), (uint64_t)iseq.size() + 64, &w0) ||
        salt_gpu_align_se(w0, &o.ao, (uint32_t)(2 * got), iseq.data(), ioff.data(), r.data())) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    salt_gpu_ws_destroy(w0);
    uint32_t used = 0;
    if (salt_isize_infer(ix, (uint32_t)got, ioff.data(), r.data(), &o.po.min_tlen, &o.po.max_tlen, &used)) {
        fprintf(stderr, "[alnpe_core]: cannot infer the insert size: %u usable pairs in the first batch (25 needed); give -a / -b\n", used);
        return false;
    }
    fprintf(stderr, "[alnpe_core]: insert size window [%u, %u] inferred from %u pairs\n", o.po.min_tlen, o.po.max_tlen, used);
    return true;
}

// The host pipeline: reader -> per-GPU workers -> ordered writer (the calling thread), over the whole input or -- header_out -- over what the
// text path left from resume[0 / 1] on, its header and blocks being out already.  t0: the start of the program's clock.  Returns the exit code.
static int run_host_pipeline(const Opts &o, const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix, const Contigs &contigs, bool header_out, const uint64_t resume[2], double t0)
{
    const int n_gpus = o.n_gpus, n_threads = o.n_threads; const bool pe = o.pe != 0;
    // workers per GPU: each takes a batch through parse -> device -> format, so several batches overlap on the host
    const int WPG = n_threads / n_gpus >= 32 ? 4 : n_threads / n_gpus >= 12 ? 3 : 2;
    std::vector<salt_gpu_ws_t *> ws((size_t)n_gpus * WPG, nullptr);
    for (int i = 0; i < n_gpus * WPG; ++i)
        if (salt_gpu_ws_create(gix[(size_t)(i / WPG)], N_SEQS, (uint64_t)N_SEQS * SALT_MAX_READ_LEN, &ws[(size_t)i])) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return 1; }
    fprintf(stderr, "%lf sec escaped.\n", now() - t0);
    t0 = now();
    gzFile fp = gzopen(o.fn_reads, "r");
    if (!fp) { fprintf(stderr, "[query_open]: file %s open fail!\n", o.fn_reads); return 1; }
    gzbuffer(fp, 1 << 20);
    gzFile fp2 = nullptr;
    if (pe) {
        fp2 = gzopen(o.fn_mates, "r");
        if (!fp2) { fprintf(stderr, "[query_open]: file %s open fail!\n", o.fn_mates); return 1; }
        gzbuffer(fp2, 1 << 20);
    }
    if (header_out) {                                     // the text path wrote everything up to these offsets (plain files: a seek)
        fflush(stdout);
        if (gzseek(fp, (z_off_t)resume[0], SEEK_SET) < 0 || (pe && gzseek(fp2, (z_off_t)resume[1], SEEK_SET) < 0)) { fprintf(stderr, "[salt] cannot seek in the read files\n"); return 1; }
    } else if (!print_header(ix, o)) return 1;
    std::mutex mu; std::condition_variable cv;
    std::deque<std::unique_ptr<Batch>> todo;          // read, not yet aligned
    std::deque<std::unique_ptr<Batch>> done;          // aligned + formatted, any order
    bool eof = false; long n_tot = 0; std::atomic<bool> failed{ false };
    const size_t max_inflight = (size_t)n_gpus * WPG * 2 + 1; size_t inflight = 0;
    // the flag is stored with `mu` held: a waiter that has evaluated its predicate but not yet blocked cannot miss the notify
    auto set_failed = [&]() { { std::lock_guard<std::mutex> lk(mu); failed = true; } cv.notify_all(); };
    std::atomic<double> t_parse{ 0 }, t_gpu{ 0 }, t_fmt{ 0 };
    double t_write = 0, t_read = 0;
    std::thread reader([&]() {
        // (after a hand-over from the text path the head of the file says nothing about what follows: kseq's general reader)
        const bool general = header_out || g_trim.instead_of_text_path;
        RawReader rr(fp, general || !sniff_four_line(o.fn_reads));
        std::unique_ptr<RawReader> rr2(pe ? new RawReader(fp2, general || !sniff_four_line(o.fn_mates)) : nullptr);
        const int per_batch = pe ? N_SEQS / 2 : N_SEQS;    // pairs per batch: N_SEQS mates (query_read_multiPairedSeqs, query.c:252-268)
        long seq_no = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return inflight < max_inflight || failed; }); if (failed) break; }
            auto b = std::make_unique<Batch>();
            b->seq_no = seq_no;
            b->raw.reserve((size_t)N_SEQS * 260);
            double tr0 = now();
            const int got = rr.take(b->raw, per_batch, b->rec);
            if (pe && got) {
                b->mate = std::make_unique<Batch>();
                b->mate->raw.reserve((size_t)per_batch * 260);
                if (rr2->take(b->mate->raw, got, b->mate->rec) != got) { fprintf(stderr, "[salt] the two read files hold different numbers of reads\n"); set_failed(); }
            }
            if (got == 0 || failed) b.reset();
            t_read += now() - tr0;
            std::unique_lock<std::mutex> lk(mu);
            if (!b) { eof = true; cv.notify_all(); break; }
            ++seq_no; ++inflight;
            todo.push_back(std::move(b));
            cv.notify_all();
        }
    });
    std::vector<std::thread> workers;
    const int fmt_threads = n_threads / (n_gpus * WPG) > 0 ? n_threads / (n_gpus * WPG) : 1;
    for (int g = 0; g < n_gpus * WPG; ++g)
        workers.emplace_back([&, g]() {
            pin_to_device_node(g / WPG);                      // before the pool: its threads inherit the node
            Pool pool(fmt_threads);
            // --polish: this worker's polish handle (its own copy of the 2-bit genome and the sorted contig table)
            std::unique_ptr<salt_gpu_polish_t, void (*)(salt_gpu_polish_t *)> gp(nullptr, salt_gpu_polish_close ? salt_gpu_polish_close : +[](salt_gpu_polish_t *) {});
            if (g_polish) {
                uint64_t l_pac = 0; const uint8_t *pac = salt_index_pac(ix, &l_pac);
                salt_gpu_polish_t *h = nullptr;
                if (salt_gpu_polish_open(g / WPG, pac, l_pac, &h) || (gp.reset(h), salt_gpu_polish_set_contigs(h, contigs.n(), contigs.off.data(), contigs.nm.data()))) {
                    fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); set_failed(); return;
                }
            }
            for (;;) {
                std::unique_ptr<Batch> b;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return !todo.empty() || eof || failed; });
                    if (failed || (todo.empty() && eof)) break;
                    b = std::move(todo.front()); todo.pop_front();
                }
                double tp0 = now();
                if (pe && !b->rec.empty()) parse_batch_pe(*b, *b->mate, pool); else parse_batch(b->raw, *b, pool);
                std::vector<uint8_t> iseq; std::vector<uint32_t> ioff;
                if (pe && b->n()) {                              // interleave the mates: pair i = reads 2i, 2i+1
                    Batch &m = *b->mate;
                    if (m.n() != b->n()) { fprintf(stderr, "[salt] the two read files hold different numbers of reads\n"); set_failed(); break; }
                    interleave_mates(*b, m, iseq, ioff);
                }
                t_parse = t_parse + (now() - tp0);
                if (b->n() == 0) { std::unique_lock<std::mutex> lk(mu); done.push_back(std::move(b)); cv.notify_all(); continue; }
                b->res.resize((size_t)b->n() * (pe ? 2 : 1));
                double tg0 = now();
                std::vector<uint8_t> iqual;                      // --error-profile, --genotype or --discover on the device: the batch's qualities, parallel to the bases
                if ((g_errprof.on && g_errprof.device) || (g_gt.on && g_gt.device) || (g_disc.on && g_disc.device)) {
                    batch_quals(*b, pe ? b->mate.get() : nullptr, iqual);
                    if (salt_gpu_ws_set_quals(ws[(size_t)g], iqual.data(), 0)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); set_failed(); break; }
                }
                int grc = pe ? salt_gpu_align_pe(ws[(size_t)g], &o.ao, &o.po, (uint32_t)b->n(), iseq.data(), ioff.data(), b->res.data())
                             : salt_gpu_align_se(ws[(size_t)g], &o.ao, (uint32_t)b->n(), b->seqs.data(), b->offs.data(), b->res.data());
                t_gpu = t_gpu + (now() - tg0);
                if (grc) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); set_failed(); break; }
                double tf0 = now();
                if (pe) format_batch_pe(ix, &o.so, &o.po, *b, pool); else format_batch(ix, &o.so, *b, pool);
                if (g_snp.host() || g_depth.host() || g_errprof.host() || g_gt.host() || g_disc.host() || g_stats.host() || g_indel.host()) {
                    bool good = true;
                    for (const std::string &piece : b->sam) good = good && host_twins_add(piece.data(), piece.size());
                    if (!good) { set_failed(); break; }
                }
                if (g_polish && !polish_batch(gp.get(), pe, *b)) { set_failed(); break; }
                if (g_bgzf.on && !bgzf_batch(b->sam, pool)) { fprintf(stderr, "[salt] no BGZF blocks for a block of the output\n"); set_failed(); break; }
                t_fmt = t_fmt + (now() - tf0);
                std::unique_lock<std::mutex> lk(mu);
                done.push_back(std::move(b));
                cv.notify_all();
            }
        });
    long next = 0;
    for (;;) {
        std::unique_ptr<Batch> b;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] {
                if (failed) return true;
                for (auto &d : done) if (d->seq_no == next) return true;
                return eof && inflight == 0;
            });
            if (failed) break;
            for (auto it = done.begin(); it != done.end(); ++it) if ((*it)->seq_no == next) { b = std::move(*it); done.erase(it); break; }
            if (!b) break;                                   // eof and nothing in flight
        }
        double tw0 = now();
        for (const std::string &piece : b->sam) fwrite(piece.data(), 1, piece.size(), stdout);
        t_write += now() - tw0;
        n_tot += b->n() * (pe ? 2 : 1); ++next;
        fprintf(stderr, "%ld reads have been aligned!\n", n_tot);
        { std::unique_lock<std::mutex> lk(mu); --inflight; cv.notify_all(); }
    }
    reader.join();
    for (auto &w : workers) w.join();
    if (!failed) bgzf_finish();
    fflush(stdout);
    double dt = now() - t0;
    fprintf(stderr, "[alnse_core]: total %lf sec escaped\n", dt);
    fprintf(stderr, "[salt] host phases (s, summed over workers): read %.3f parse %.3f gpu-call %.3f format %.3f write %.3f\n", t_read, t_parse.load(), t_gpu.load(), t_fmt.load(), t_write);
    fprintf(stderr, "[salt] %ld reads, %.3f Mreads/s end to end (FASTQ -> SAM, %d GPU(s), %d host thread(s))\n", n_tot, dt > 0 ? n_tot / dt / 1e6 : 0.0, n_gpus, n_threads);
    gzclose(fp);
    if (fp2) gzclose(fp2);
    for (int i = 0; i < n_gpus * WPG; ++i) salt_gpu_ws_destroy(ws[(size_t)i]);
    return failed ? 1 : 0;
}

// --snp-counts, before the first block: the sites of the index; counting on on every GPU's index, or the host's table
static bool snp_begin(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_snp.on) return true;
    g_snp.ix = ix;
    const int64_t n = salt_snp_sites(ix, nullptr, 0);
    if (n < 0) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
    g_snp.n_sites = (uint64_t)n;
    if (!g_snp.device) { g_snp.host_counts.assign((size_t)n * 4, 0u); return true; }
    for (salt_gpu_index_t *g : gix) {
        uint32_t n_dev = 0;
        if (salt_gpu_index_snp_enable(g, 1, g_snp.min_mapq) || salt_gpu_index_snp_sites(g, &n_dev, nullptr, 0)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
        if (n_dev != g_snp.n_sites) { fprintf(stderr, "[salt] --snp-counts: the device's site table has %u sites, the index %llu\n", n_dev, (unsigned long long)g_snp.n_sites); return false; }
    }
    return true;
}

// --snp-counts, after the last block of a run that succeeded: every GPU's counts summed in 64 bits, one line per site in genome order
static bool snp_finish(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_snp.on) return true;
    const size_t n = (size_t)g_snp.n_sites;
    std::vector<uint64_t> sum(n * 4, 0);
    if (g_snp.device) {
        std::vector<uint32_t> c(n * 4);
        for (salt_gpu_index_t *g : gix) {
            if (salt_gpu_index_snp_counts(g, c.data(), c.size(), 0)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
            for (size_t i = 0; i < c.size(); ++i) sum[i] += c[i];
        }
    } else for (size_t i = 0; i < sum.size(); ++i) sum[i] = g_snp.host_counts[i];
    std::vector<uint32_t> pos(n);
    salt_snp_sites(ix, pos.data(), n);
    const salt_host_index_t *hv = salt_index_host_view(ix);
    uint64_t l_pac = 0; const uint8_t *pac = salt_index_pac(ix, &l_pac);
    FILE *f = g_snp.fp;
    fprintf(f, "#contig\tpos\tref\talleles\tA\tC\tG\tT\n");
    int32_t c = 0; const int32_t n_seqs = salt_index_n_seqs(ix);
    int64_t c_off = 0; int32_t c_len = 0; const char *c_name = "*";
    if (n_seqs > 0) salt_index_seq(ix, 0, &c_off, &c_len, &c_name);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t g = pos[i];
        while (c + 1 < n_seqs && (int64_t)g >= c_off + c_len) salt_index_seq(ix, ++c, &c_off, &c_len, &c_name);
        const uint32_t mask = (hv->ref[g >> 3] >> (4 * (g & 7u))) & 15u;
        char alleles[5]; int na = 0;
        for (int b = 0; b < 4; ++b) if (mask & (1u << b)) alleles[na++] = "ACGT"[b];
        alleles[na] = 0;
        const char ref = g < l_pac ? "ACGT"[(pac[g >> 2] >> ((~g & 3u) << 1)) & 3u] : 'N';
        fprintf(f, "%s\t%lld\t%c\t%s\t%llu\t%llu\t%llu\t%llu\n", c_name, (long long)((int64_t)g - c_off + 1), ref, alleles,
                (unsigned long long)sum[4 * i], (unsigned long long)sum[4 * i + 1], (unsigned long long)sum[4 * i + 2], (unsigned long long)sum[4 * i + 3]);
    }
    const bool ok = !ferror(f) && fclose(f) == 0;
    g_snp.fp = nullptr;
    if (!ok) { fprintf(stderr, "[salt] --snp-counts: write error on %s\n", g_snp.fn); return false; }
    fprintf(stderr, "[salt] SNP counts: %llu sites, %s, MAPQ >= %u -> %s\n", (unsigned long long)g_snp.n_sites, g_snp.device ? "counted on the device" : "counted on the host from the SAM lines",
            g_snp.min_mapq, g_snp.fn);
    return true;
}

// --error-profile, before the first block: the profile on on every GPU's index, or the host's tables
static bool errprof_begin(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_errprof.on) return true;
    g_errprof.ix = ix;
    g_errprof.cells.assign(ERRPROF_CELLS, 0);
    if (!g_errprof.device) return true;
    for (salt_gpu_index_t *g : gix)
        if (salt_gpu_index_errprof_enable(g, 1, g_errprof.min_mapq)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    return true;
}

// --error-profile, after the last block of a run that succeeded: every GPU's tables are fetched and summed on the host, and the file is printed
static bool errprof_finish(const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_errprof.on) return true;
    if (g_errprof.device) {
        std::vector<uint64_t> one(ERRPROF_CELLS);
        for (salt_gpu_index_t *g : gix) {
            uint64_t rec[16];
            if (salt_gpu_index_errprof_fetch(g, one.data(), one.size(), rec, 0)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
            for (size_t i = 0; i < one.size(); ++i) g_errprof.cells[i] += one[i];
            for (int i = 0; i < 16; ++i) g_errprof.rec[i] += rec[i];
        }
    }
    const int64_t need = salt_errprof_text(g_errprof.cells.data(), g_errprof.rec, g_errprof.min_mapq, g_errprof.full ? 1 : 0, nullptr, 0);
    std::string text(need > 0 ? (size_t)need : 0, '\0');
    if (need < 0 || salt_errprof_text(g_errprof.cells.data(), g_errprof.rec, g_errprof.min_mapq, g_errprof.full ? 1 : 0, &text[0], (uint64_t)need) != need) {
        fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false;
    }
    FILE *f = g_errprof.fp;
    bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    ok = !ferror(f) && fclose(f) == 0 && ok;
    g_errprof.fp = nullptr;
    if (!ok) { fprintf(stderr, "[salt] --error-profile: write error on %s\n", g_errprof.fn); return false; }
    uint64_t bases = 0;
    for (uint64_t v : g_errprof.cells) bases += v;
    fprintf(stderr, "[salt] error profile: %llu records, %llu bases, %s, MAPQ >= %u -> %s (%llu bytes)\n", (unsigned long long)(g_errprof.rec[4] + g_errprof.rec[12]),
            (unsigned long long)bases, g_errprof.device ? "counted on the device" : "counted on the host from the SAM lines", g_errprof.min_mapq, g_errprof.fn,
            (unsigned long long)text.size());
    return true;
}

// --stats, before the first block: the contig table (the tally's per-contig counts need it on the host pipeline too) and the tally on on
// every GPU's index, or the host's tables
static bool stats_begin(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix, const Contigs &C)
{
    if (!g_stats.on) return true;
    g_stats.ix = ix;
    g_stats.cells.assign(STATS_CELLS, 0);
    g_stats.ct.assign((size_t)salt_index_n_seqs(ix) * 8, 0);
    if (!g_stats.device) return true;
    for (salt_gpu_index_t *g : gix)
        if (salt_gpu_index_set_contigs(g, C.n(), C.off.data(), C.nm.data()) || salt_gpu_index_stats_enable(g, 1, g_stats.min_mapq)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    return true;
}

// --stats, after the last block of a run that succeeded: every GPU's tables are fetched and summed on the host, and the file is printed
static bool stats_finish(const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_stats.on) return true;
    if (g_stats.device) {
        std::vector<uint64_t> one(g_stats.cells.size()), one_ct(g_stats.ct.size());
        for (salt_gpu_index_t *g : gix) {
            if (salt_gpu_index_stats_fetch(g, one.data(), one.size(), one_ct.data(), one_ct.size(), 0)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
            for (size_t i = 0; i < one.size(); ++i) g_stats.cells[i] += one[i];
            for (size_t i = 0; i < one_ct.size(); ++i) g_stats.ct[i] += one_ct[i];
        }
    }
    auto text_of = [&](char *out, uint64_t cap) { return salt_stats_text(g_stats.ix, g_stats.cells.data(), g_stats.cells.size(), g_stats.ct.data(), g_stats.ct.size(), g_stats.min_mapq, out, cap); };
    const int64_t need = text_of(nullptr, 0);
    std::string text(need > 0 ? (size_t)need : 0, '\0');
    if (need < 0 || text_of(&text[0], (uint64_t)need) != need) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
    FILE *f = g_stats.fp;
    bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    ok = !ferror(f) && fclose(f) == 0 && ok;
    g_stats.fp = nullptr;
    if (!ok) { fprintf(stderr, "[salt] --stats: write error on %s\n", g_stats.fn); return false; }
    fprintf(stderr, "[salt] stats: %llu records seen, %llu counted, %s, MAPQ >= %u -> %s (%llu bytes)\n", (unsigned long long)(g_stats.cells[0] + g_stats.cells[16]),
            (unsigned long long)(g_stats.cells[4] + g_stats.cells[20]), g_stats.device ? "counted on the device" : "counted on the host from the SAM lines", g_stats.min_mapq, g_stats.fn,
            (unsigned long long)text.size());
    return true;
}

// --depth, before the first block: marking on on every GPU's index, or the host's array
static bool depth_begin(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_depth.on) return true;
    g_depth.ix = ix;
    if (!g_depth.device) { g_depth.host_diff.assign((size_t)salt_index_host_view(ix)->ref_len + 1, 0u); return true; }
    for (salt_gpu_index_t *g : gix)
        if (salt_gpu_index_depth_enable(g, 1, g_depth.min_mapq)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    return true;
}

// --depth, after the last block of a run that succeeded: the arrays of the other GPUs are added into the first one's, in chunks through a
// page-locked buffer, and its text kernels print the file piece by piece; on the host the twin prints it.  A .gz file ends with the BGZF
// end-of-file block.
static bool depth_finish(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix, const Contigs &C)
{
    if (!g_depth.on) return true;
    FILE *f = g_depth.fp;
    uint64_t text_bytes = 0, file_bytes = 0;
    bool ok = true;
    if (g_depth.device) {
        const uint64_t words = (uint64_t)salt_index_host_view(ix)->ref_len + 1, chunk = std::min<uint64_t>(words, 16u << 20);
        auto gpu_fail = [&]() { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; };
        if (gix.size() > 1) {
            uint32_t *buf = nullptr;
            if (salt_gpu_host_alloc(chunk * 4, (void **)&buf)) return gpu_fail();
            for (size_t k = 1; k < gix.size() && ok; ++k)
                for (uint64_t at = 0; at < words && ok; at += chunk) {
                    const uint64_t n = std::min(chunk, words - at);
                    ok = salt_gpu_index_depth_fetch(gix[k], at, n, buf) == 0 && salt_gpu_index_depth_add(gix[0], at, n, buf) == 0;
                }
            if (!ok) gpu_fail();
            salt_gpu_host_free(buf);
            if (!ok) return false;
        }
        salt_depth_text_opt_t to; to.window = g_depth.window; to.tile_positions = 0; to.bgzf = g_depth.gz ? 1 : 0;
        if (salt_gpu_index_depth_enable(gix[0], 0, g_depth.min_mapq) || salt_gpu_index_set_contigs(gix[0], C.n(), C.off.data(), C.nm.data()) ||
            salt_gpu_index_depth_text_begin(gix[0], &to)) return gpu_fail();
        for (;;) {
            const char *data = nullptr; uint64_t n = 0;
            if (salt_gpu_index_depth_text_next(gix[0], &data, &n)) return gpu_fail();
            if (n == 0) break;
            ok = ok && fwrite(data, 1, (size_t)n, f) == n;
            file_bytes += n; text_bytes += g_depth.gz ? bgzf_text_bytes(data, n) : n;
        }
    } else {
        const int64_t need = salt_depth_text(ix, g_depth.host_diff.data(), g_depth.host_diff.size(), g_depth.window, nullptr, 0);
        std::string text(need > 0 ? (size_t)need : 0, '\0'), z;
        if (need < 0 || salt_depth_text(ix, g_depth.host_diff.data(), g_depth.host_diff.size(), g_depth.window, &text[0], (uint64_t)need) != need) {
            fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false;
        }
        if (g_depth.gz && !bgzf_deflate_host(text.data(), text.size(), z)) { fprintf(stderr, "[salt] --depth: no BGZF blocks for the text\n"); return false; }
        const std::string &out = g_depth.gz ? z : text;
        ok = fwrite(out.data(), 1, out.size(), f) == out.size();
        text_bytes = text.size(); file_bytes = out.size();
    }
    if (g_depth.gz) { ok = ok && fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, f) == sizeof BGZF_EOF; file_bytes += sizeof BGZF_EOF; }
    ok = !ferror(f) && fclose(f) == 0 && ok;
    g_depth.fp = nullptr;
    if (!ok) { fprintf(stderr, "[salt] --depth: write error on %s\n", g_depth.fn); return false; }
    char what[64];
    if (g_depth.window) snprintf(what, sizeof what, "windows of %u", g_depth.window); else snprintf(what, sizeof what, "per base");
    fprintf(stderr, "[salt] depth: %s, %s, MAPQ >= %u, %llu bytes of text -> %s (%llu bytes)\n", what,
            g_depth.device ? "marked and printed on the device" : "summed on the host from the SAM lines", g_depth.min_mapq, (unsigned long long)text_bytes, g_depth.fn,
            (unsigned long long)file_bytes);
    return true;
}

// --genotype, before the first block: the sums on on every GPU's index, or the host's table
static bool gt_begin(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_gt.on) return true;
    g_gt.ix = ix;
    const int64_t n = salt_snp_sites(ix, nullptr, 0);
    if (n < 0) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
    if (!g_gt.device) { g_gt.host_sums.assign((size_t)n, salt_gt_site_t{}); return true; }
    for (salt_gpu_index_t *g : gix)
        if (salt_gpu_index_gt_enable(g, 1, g_gt.min_mapq)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    return true;
}

// --genotype, after the last block of a run that succeeded: the header (salt_gt_header; through the host's BGZF encoder for a .gz file), then
// the records: the sums of the other GPUs are added into the first one's, in chunks through a page-locked buffer, and its kernels make the
// calls and print the records piece by piece; on the host the twin's printer does.  A .gz file ends with the BGZF end-of-file block.
static bool gt_finish(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix, const Contigs &C)
{
    if (!g_gt.on) return true;
    FILE *f = g_gt.fp;
    uint64_t text_bytes = 0, file_bytes = 0;
    const uint64_t n_sites = (uint64_t)salt_snp_sites(ix, nullptr, 0);
    const int64_t hn = salt_gt_header(ix, g_gt.sample, nullptr, 0);
    std::string head(hn > 0 ? (size_t)hn : 0, '\0'), z;
    if (hn < 0 || salt_gt_header(ix, g_gt.sample, &head[0], (uint64_t)hn) != hn) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
    if (g_gt.gz && !bgzf_deflate_host(head.data(), head.size(), z)) { fprintf(stderr, "[salt] --genotype: no BGZF blocks for the header\n"); return false; }
    bool ok = fwrite((g_gt.gz ? z : head).data(), 1, (g_gt.gz ? z : head).size(), f) == (g_gt.gz ? z : head).size();
    text_bytes += head.size(); file_bytes += (g_gt.gz ? z : head).size();
    if (g_gt.device) {
        const uint64_t chunk = std::min<uint64_t>(n_sites, 1u << 17);             // 16 MiB of sums at a time
        auto gpu_fail = [&]() { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; };
        if (gix.size() > 1 && n_sites) {
            salt_gt_site_t *buf = nullptr;
            if (salt_gpu_host_alloc(chunk * sizeof(salt_gt_site_t), (void **)&buf)) return gpu_fail();
            for (size_t k = 1; k < gix.size() && ok; ++k)
                for (uint64_t at = 0; at < n_sites && ok; at += chunk) {
                    const uint64_t n = std::min(chunk, n_sites - at);
                    ok = salt_gpu_index_gt_fetch(gix[k], at, n, buf) == 0 && salt_gpu_index_gt_add(gix[0], at, n, buf) == 0;
                }
            if (!ok) gpu_fail();
            salt_gpu_host_free(buf);
            if (!ok) return false;
        }
        salt_gt_text_opt_t to; to.tile_sites = 0; to.bgzf = g_gt.gz ? 1 : 0;
        if (salt_gpu_index_gt_enable(gix[0], 0, g_gt.min_mapq) || salt_gpu_index_set_contigs(gix[0], C.n(), C.off.data(), C.nm.data()) ||
            salt_gpu_index_gt_text_begin(gix[0], &to)) return gpu_fail();
        for (;;) {
            const char *data = nullptr; uint64_t n = 0;
            if (salt_gpu_index_gt_text_next(gix[0], &data, &n)) return gpu_fail();
            if (n == 0) break;
            ok = ok && fwrite(data, 1, (size_t)n, f) == n;
            file_bytes += n; text_bytes += g_gt.gz ? bgzf_text_bytes(data, n) : n;
        }
    } else {
        const int64_t need = salt_gt_text(ix, g_gt.host_sums.data(), 0, n_sites, nullptr, 0);
        std::string text(need > 0 ? (size_t)need : 0, '\0');
        if (need < 0 || salt_gt_text(ix, g_gt.host_sums.data(), 0, n_sites, &text[0], (uint64_t)need) != need) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
        z.clear();
        if (g_gt.gz && !text.empty() && !bgzf_deflate_host(text.data(), text.size(), z)) { fprintf(stderr, "[salt] --genotype: no BGZF blocks for the records\n"); return false; }
        const std::string &out = g_gt.gz ? z : text;
        ok = ok && fwrite(out.data(), 1, out.size(), f) == out.size();
        text_bytes += text.size(); file_bytes += out.size();
    }
    if (g_gt.gz) { ok = ok && fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, f) == sizeof BGZF_EOF; file_bytes += sizeof BGZF_EOF; }
    ok = !ferror(f) && fclose(f) == 0 && ok;
    g_gt.fp = nullptr;
    if (!ok) { fprintf(stderr, "[salt] --genotype: write error on %s\n", g_gt.fn); return false; }
    fprintf(stderr, "[salt] genotypes: %llu sites, %s, MAPQ >= %u, %llu bytes of text -> %s (%llu bytes)\n", (unsigned long long)n_sites,
            g_gt.device ? "summed, called and printed on the device" : "summed on the host from the SAM lines", g_gt.min_mapq, (unsigned long long)text_bytes, g_gt.fn,
            (unsigned long long)file_bytes);
    return true;
}

// --discover, before the first block: the arrays on on every GPU's index, or the host's arrays
static bool disc_begin(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix)
{
    if (!g_disc.on) return true;
    g_disc.ix = ix;
    const size_t ref_len = salt_index_host_view(ix)->ref_len;
    if (!g_disc.device) { g_disc.host_alt.assign(ref_len, 0ull); g_disc.host_diff.assign(ref_len + 1, 0u); return true; }
    for (salt_gpu_index_t *g : gix)
        if (salt_gpu_index_disc_enable(g, 1, g_disc.min_mapq, g_disc.min_baseq)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    return true;
}

// --discover, after the last block of a run that succeeded: both arrays of the other GPUs are added into the first one's, in chunks through
// a page-locked buffer, and its kernels flag, compact and print the candidates piece by piece; on the host the twin's printer does.  A .gz
// file ends with the BGZF end-of-file block.  salt-idx lays the i-th group of lines over the i-th contig whatever its name: a contig without
// a line shifts those behind it, which is said on stderr.
static bool disc_finish(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix, const Contigs &C)
{
    if (!g_disc.on) return true;
    FILE *f = g_disc.fp;
    uint64_t text_bytes = 0, file_bytes = 0;
    bool ok = true;
    const uint64_t ref_len = salt_index_host_view(ix)->ref_len;
    std::vector<uint8_t> seen((size_t)C.n() + 1, 0);
    if (g_disc.device) {
        const uint64_t chunk = std::min<uint64_t>(ref_len + 1, 4u << 20);              // 32 MiB of alt at a time
        auto gpu_fail = [&]() { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; };
        if (gix.size() > 1) {
            void *buf = nullptr;
            if (salt_gpu_host_alloc(chunk * 8, &buf)) return gpu_fail();
            for (size_t k = 1; k < gix.size() && ok; ++k)
                for (int which = SALT_DISC_ALT; which <= SALT_DISC_DIFF && ok; ++which) {
                    const uint64_t words = ref_len + (which == SALT_DISC_DIFF ? 1 : 0);
                    for (uint64_t at = 0; at < words && ok; at += chunk) {
                        const uint64_t n = std::min(chunk, words - at);
                        ok = salt_gpu_index_disc_fetch(gix[k], which, at, n, buf) == 0 && salt_gpu_index_disc_add(gix[0], which, at, n, buf) == 0;
                    }
                }
            if (!ok) gpu_fail();
            salt_gpu_host_free(buf);
            if (!ok) return false;
        }
        salt_disc_text_opt_t to; to.min_alt = g_disc.min_alt; to.min_pct = g_disc.min_pct; to.all_sites = g_disc.all ? 1 : 0; to.tile_positions = 0; to.bgzf = g_disc.gz ? 1 : 0;
        if (salt_gpu_index_disc_enable(gix[0], 0, g_disc.min_mapq, g_disc.min_baseq) || salt_gpu_index_set_contigs(gix[0], C.n(), C.off.data(), C.nm.data()) ||
            salt_gpu_index_disc_text_begin(gix[0], &to)) return gpu_fail();
        for (;;) {
            const char *data = nullptr; uint64_t n = 0;
            if (salt_gpu_index_disc_text_next(gix[0], &data, &n)) return gpu_fail();
            if (n == 0) break;
            ok = ok && fwrite(data, 1, (size_t)n, f) == n;
            file_bytes += n; text_bytes += g_disc.gz ? bgzf_text_bytes(data, n) : n;
        }
        if (salt_gpu_index_disc_text_seen(gix[0], seen.data(), seen.size())) return gpu_fail();
    } else {
        const int64_t need = salt_disc_text(ix, g_disc.host_alt.data(), g_disc.host_diff.data(), ref_len, g_disc.min_alt, g_disc.min_pct, g_disc.all, nullptr, 0, nullptr);
        std::string text(need > 0 ? (size_t)need : 0, '\0'), z;
        if (need < 0 || salt_disc_text(ix, g_disc.host_alt.data(), g_disc.host_diff.data(), ref_len, g_disc.min_alt, g_disc.min_pct, g_disc.all, &text[0], (uint64_t)need, seen.data()) != need) {
            fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false;
        }
        if (g_disc.gz && !text.empty() && !bgzf_deflate_host(text.data(), text.size(), z)) { fprintf(stderr, "[salt] --discover: no BGZF blocks for the text\n"); return false; }
        const std::string &out = g_disc.gz ? z : text;
        ok = fwrite(out.data(), 1, out.size(), f) == out.size();
        text_bytes = text.size(); file_bytes = out.size();
    }
    if (g_disc.gz) { ok = ok && fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, f) == sizeof BGZF_EOF; file_bytes += sizeof BGZF_EOF; }
    ok = !ferror(f) && fclose(f) == 0 && ok;
    g_disc.fp = nullptr;
    if (!ok) { fprintf(stderr, "[salt] --discover: write error on %s\n", g_disc.fn); return false; }
    fprintf(stderr, "[salt] discover: %s, MAPQ >= %u, base quality >= %u, min_alt %u, min_pct %u%s, %llu bytes of text -> %s (%llu bytes)\n",
            g_disc.device ? "counted and printed on the device" : "counted on the host from the SAM lines", g_disc.min_mapq, g_disc.min_baseq, g_disc.min_alt, g_disc.min_pct,
            g_disc.all ? ", all sites" : "", (unsigned long long)text_bytes, g_disc.fn, (unsigned long long)file_bytes);
    int n_without = 0, first_without = -1;
    for (int c = 0; c < C.n(); ++c) if (!seen[(size_t)c]) { if (first_without < 0) first_without = c; ++n_without; }
    if (n_without) {
        int64_t off = 0; int32_t len = 0; const char *name = "?";
        salt_index_seq(ix, first_without, &off, &len, &name);
        fprintf(stderr, "[salt] discover: %d of %d contigs have no line in %s, the first is %s: salt-idx lays the i-th group of lines over the i-th contig whatever its name, "
                        "so the groups behind it would shift\n", n_without, C.n(), g_disc.fn, name);
    }
    return true;
}

// --indels, before the first block: the contig table (an allele stays inside its contig) and the tally on on every GPU's index, or the host's map
static bool indel_begin(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix, const Contigs &C)
{
    if (!g_indel.on) return true;
    g_indel.ix = ix;
    if (!g_indel.device) { g_indel.host_tab = salt_indel_new(); g_indel.host_diff.assign((size_t)salt_index_host_view(ix)->ref_len + 1, 0u); return true; }
    for (salt_gpu_index_t *g : gix)
        if (salt_gpu_index_set_contigs(g, C.n(), C.off.data(), C.nm.data()) || salt_gpu_index_indel_enable(g, 1, g_indel.min_mapq, g_indel.log2_slots)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; }
    return true;
}

// --indels, after the last block of a run that succeeded: the other GPUs' live slots (through the insert kernel) and difference arrays are
// added into the first one's, whose kernels sort the alleles, apply the call rule and print the records piece by piece; on the host the
// twin's printer does.  The header carries the dropped events; a .gz file ends with the BGZF end-of-file block.
static bool indel_finish(const salt_index_t *ix, const std::vector<salt_gpu_index_t *> &gix, const Contigs &C)
{
    if (!g_indel.on) return true;
    FILE *f = g_indel.fp;
    uint64_t text_bytes = 0, file_bytes = 0, stat[4] = { 0, 0, 0, 0 };
    bool ok = true;
    const uint64_t ref_len = salt_index_host_view(ix)->ref_len;
    auto gpu_fail = [&]() { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return false; };
    auto emit = [&](const std::string &text) {                         // text that was made on the host: the header, the host path's records
        std::string z;
        if (g_indel.gz && !text.empty() && !bgzf_deflate_host(text.data(), text.size(), z)) { fprintf(stderr, "[salt] --indels: no BGZF blocks for the text\n"); return false; }
        const std::string &out = g_indel.gz ? z : text;
        ok = ok && fwrite(out.data(), 1, out.size(), f) == out.size();
        text_bytes += text.size(); file_bytes += out.size();
        return true;
    };
    auto header = [&]() {
        const int64_t need = salt_indel_header(ix, g_indel.min_mapq, g_indel.min_alt, g_indel.min_pct, stat[1], nullptr, 0);
        std::string h(need > 0 ? (size_t)need : 0, '\0');
        if (need < 0 || salt_indel_header(ix, g_indel.min_mapq, g_indel.min_alt, g_indel.min_pct, stat[1], &h[0], (uint64_t)need) != need) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
        return emit(h);
    };
    if (g_indel.device) {
        // GPU 0's counters after the merge hold its own events and the others' tabled ones (tabled or dropped again on GPU 0); the others'
        // dropped, long and unanchored are added on the host
        uint64_t extra[4] = { 0, 0, 0, 0 };
        if (gix.size() > 1) {
            const uint64_t chunk = std::min<uint64_t>(ref_len + 1, 8u << 20);
            std::vector<uint32_t> words((size_t)chunk);
            std::vector<uint64_t> pairs;
            for (size_t k = 1; k < gix.size(); ++k) {
                uint64_t one[4], n = 0;
                if (salt_gpu_index_indel_stats(gix[k], one) || salt_gpu_index_indel_fetch(gix[k], 0, nullptr, &n)) return gpu_fail();
                pairs.resize((size_t)n * 2);
                if (n && (salt_gpu_index_indel_fetch(gix[k], n, pairs.data(), &n) || salt_gpu_index_indel_add(gix[0], pairs.data(), n))) return gpu_fail();
                for (int i = 1; i < 4; ++i) extra[i] += one[i];
                for (uint64_t at = 0; at < ref_len + 1; at += chunk) {
                    const uint64_t m = std::min(chunk, ref_len + 1 - at);
                    if (salt_gpu_index_indel_fetch_diff(gix[k], at, m, words.data()) || salt_gpu_index_indel_add_diff(gix[0], at, m, words.data())) return gpu_fail();
                }
            }
        }
        if (salt_gpu_index_indel_enable(gix[0], 0, g_indel.min_mapq, 0) || salt_gpu_index_indel_stats(gix[0], stat)) return gpu_fail();
        for (int i = 1; i < 4; ++i) stat[i] += extra[i];
        if (!header()) return false;
        salt_indel_text_opt_t to; to.min_alt = g_indel.min_alt; to.min_pct = g_indel.min_pct; to.tile_positions = 0; to.bgzf = g_indel.gz ? 1 : 0;
        if (salt_gpu_index_set_contigs(gix[0], C.n(), C.off.data(), C.nm.data()) || salt_gpu_index_indel_text_begin(gix[0], &to)) return gpu_fail();
        for (;;) {
            const char *data = nullptr; uint64_t n = 0;
            if (salt_gpu_index_indel_text_next(gix[0], &data, &n)) return gpu_fail();
            if (n == 0) break;
            ok = ok && fwrite(data, 1, (size_t)n, f) == n;
            file_bytes += n; text_bytes += g_indel.gz ? bgzf_text_bytes(data, n) : n;
        }
    } else {
        salt_indel_stats(g_indel.host_tab, stat);
        if (!header()) return false;
        const int64_t n = salt_indel_entries(g_indel.host_tab, nullptr, 0);
        std::vector<uint64_t> pairs(n > 0 ? (size_t)n * 2 : 0);
        if (n < 0 || salt_indel_entries(g_indel.host_tab, pairs.data(), (uint64_t)n) != n) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false; }
        const int64_t need = salt_indel_text(ix, pairs.data(), (uint64_t)n, g_indel.host_diff.data(), ref_len, g_indel.min_alt, g_indel.min_pct, nullptr, 0);
        std::string text(need > 0 ? (size_t)need : 0, '\0');
        if (need < 0 || salt_indel_text(ix, pairs.data(), (uint64_t)n, g_indel.host_diff.data(), ref_len, g_indel.min_alt, g_indel.min_pct, &text[0], (uint64_t)need) != need) {
            fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return false;
        }
        if (!emit(text)) return false;
        salt_indel_free(g_indel.host_tab); g_indel.host_tab = nullptr;
    }
    if (g_indel.gz) { ok = ok && fwrite(BGZF_EOF, 1, sizeof BGZF_EOF, f) == sizeof BGZF_EOF; file_bytes += sizeof BGZF_EOF; }
    ok = !ferror(f) && fclose(f) == 0 && ok;
    g_indel.fp = nullptr;
    if (!ok) { fprintf(stderr, "[salt] --indels: write error on %s\n", g_indel.fn); return false; }
    fprintf(stderr, "[salt] indels: %s, MAPQ >= %u, min_alt %u, min_pct %u, %llu slots, tabled %llu, dropped %llu, long %llu, unanchored %llu, %llu bytes of text -> %s (%llu bytes)\n",
            g_indel.device ? "tabled and printed on the device" : "tabled on the host from the SAM lines", g_indel.min_mapq, g_indel.min_alt, g_indel.min_pct,
            (unsigned long long)(g_indel.device ? 1ull << g_indel.log2_slots : 0ull), (unsigned long long)stat[0], (unsigned long long)stat[1], (unsigned long long)stat[2], (unsigned long long)stat[3],
            (unsigned long long)text_bytes, g_indel.fn, (unsigned long long)file_bytes);
    if (stat[1]) fprintf(stderr, "[salt] indels: WARNING: %llu events found no slot within %u of their home slot and are not in %s: the table of %llu slots is too full, raise --indels-slots\n",
                         (unsigned long long)stat[1], 128u, g_indel.fn, (unsigned long long)(1ull << g_indel.log2_slots));
    return true;
}

} // namespace

// options; choice of path (TextPlan); index load and attach; header; text path; host pipeline
int main(int argc, char **argv)
{
    Opts o;
    if (const int stop = parse_options(argc, argv, o); stop >= 0) return stop;
    const int n_gpus = o.n_gpus; const bool pe = o.pe != 0;
    // Single end + a plain (not gzipped) strict 4-line FASTQ in a regular file: the text path -- parse, align and format on the device
    // (run_se_text).  Everything else (paired end, gzip, pipes, multi-line records) goes through the host pipeline below.
    // SALT_HOST_PIPELINE=1 forces the latter.  Decided before the index is loaded: the text path's page-locked buffers are allocated
    // by a thread of their own meanwhile.
    TextPlan plan; bool text_path = false;
    if (!(getenv("SALT_HOST_PIPELINE") && atoi(getenv("SALT_HOST_PIPELINE")))) {
        auto plain4 = [](const char *fn) {
            struct stat sb; unsigned char magic[2] = { 0, 0 };
            bool plain = stat(fn, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0;
            if (plain) { FILE *f = fopen(fn, "rb"); plain = f && fread(magic, 1, 2, f) == 2 && !(magic[0] == 0x1f && magic[1] == 0x8b); if (f) fclose(f); }
            return plain && sniff_four_line(fn);
        };
        text_path = plain4(o.fn_reads) && (!pe || plain4(o.fn_mates));
        // single end, blocked gzip (BGZF) whose text starts as strict 4-line FASTQ: the text path over the uncompressed byte range
        if (!text_path && !pe && bgzf_index(o.fn_reads, plan.bgzf) && sniff_four_line(o.fn_reads)) text_path = true;
        else if (!text_path) plan.bgzf = Bgzf();
        if (text_path && g_trim.any() && !g_trim.device) {   // no k_fq_trim (or no k_fq_trim_pair) in this libsalt_gpu: the host parser trims, so the host pipeline reads
            fprintf(stderr, "[salt] trim: this libsalt_gpu does not trim on the device: the whole run goes through the host pipeline\n");
            text_path = false; plan.bgzf = Bgzf(); g_trim.instead_of_text_path = true;
        }
        if (text_path) text_plan(plan, o.fn_reads, n_gpus, o.n_threads, pe);
    }
    const double t0 = now();
    fprintf(stderr, "[alnse_core]:  Reload index...\n");
    salt_index_t *ix = salt_index_load(o.prefix, 0);
    if (!ix) { fprintf(stderr, "[salt] %s\n", salt_host_last_error()); return 1; }
    o.ao.l_seed = salt_index_seed_len(ix);
    g_bam.ix = ix;
    o.ao.l_overlap = o.overlap > 0 ? o.overlap : o.ao.l_seed;              // aln.c:223
    std::vector<int> devs; for (int i = 0; i < n_gpus; ++i) devs.push_back(i);
    std::vector<salt_gpu_index_t *> gix((size_t)n_gpus, nullptr);
    if (salt_gpu_index_attach(salt_index_host_view(ix), 0, &gix[0])) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return 1; }
    if (salt_gpu_index_replicate(gix[0], devs.data(), n_gpus, gix.data())) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return 1; }
    if (g_polish && (!salt_gpu_ws_set_polish || !salt_gpu_polish_open || !salt_gpu_polish_close || !salt_gpu_polish_set_contigs || !salt_gpu_polish_text)) {
        fprintf(stderr, "[salt] --polish: this libsalt_gpu has no polish stage\n"); return 1;
    }
    if (pe || g_polish) {                                 // the singleton rescue aligns against the 2-bit genome (alnpe.c:327-393); --polish re-scores against it
        uint64_t l_pac = 0; const uint8_t *pac = salt_index_pac(ix, &l_pac);
        for (int i = 0; i < n_gpus; ++i)
            if (salt_gpu_index_set_pac(gix[(size_t)i], pac, l_pac)) { fprintf(stderr, "[salt] %s\n", salt_gpu_last_error()); return 1; }
    }
    const Contigs contigs(ix);
    auto leave = [&](int rc) { if (rc == 0) trim_report(); for (int i = n_gpus - 1; i >= 0; --i) salt_gpu_index_detach(gix[(size_t)i]); salt_index_free(ix); return rc; };
    if (pe && o.po.max_tlen == 0 && !infer_isize(o, ix, gix[0])) return 1;
    if (!snp_begin(ix, gix) || !depth_begin(ix, gix) || !errprof_begin(ix, gix) || !gt_begin(ix, gix) || !disc_begin(ix, gix) || !stats_begin(ix, gix, contigs) || !indel_begin(ix, gix, contigs)) return 1;                          // (behind infer_isize: its single-end pass over the first batch is not the run's)
    bool header_out = false; uint64_t resume[2] = { 0, 0 };      // set when the text path hands the rest of the input to the host pipeline
    if (text_path) {
        fprintf(stderr, "%lf sec escaped.\n", now() - t0);
        if (!print_header(ix, o)) return 1;
        const int rc = pe ? run_pe_text(o.fn_reads, o.fn_mates, gix, contigs, plan, o.ao, o.so, o.po, now(), resume)
                          : run_se_text(o.fn_reads, gix, contigs, plan, o.ao, o.so, now(), &resume[0]);
        if (rc != 2) { if (rc == 0) bgzf_finish(); return leave(rc == 0 && !(snp_finish(ix, gix) && depth_finish(ix, gix, contigs) && errprof_finish(gix) && gt_finish(ix, gix, contigs) && disc_finish(ix, gix, contigs) && stats_finish(gix) && indel_finish(ix, gix, contigs)) ? 1 : rc); }
        header_out = true;
    }
    const int rc = run_host_pipeline(o, ix, gix, contigs, header_out, resume, t0);
    return leave(rc == 0 && !(snp_finish(ix, gix) && depth_finish(ix, gix, contigs) && errprof_finish(gix) && gt_finish(ix, gix, contigs) && disc_finish(ix, gix, contigs) && stats_finish(gix) && indel_finish(ix, gix, contigs)) ? 1 : rc);
}
