// tools/genotype_model.cc -- the host twin of the genotype sums and its printer (salt_gt_add_sam / salt_gt_text / salt_gt_header of
// salt_amd/host/salt_host.cc) as a stand-alone program, so that it can run under AddressSanitizer + UBSan (tests/test_genotype_model.py
// builds it together with salt_host.cc).
//
//   genotype_model <index prefix> <min_mapq> <file.sam | file.sam.gz>...
//
// Per file: the text whole, then the same text in pieces cut at line ends (a run counts block by block), then line by line with every
// line handed over WITHOUT its newline -- buffers that end exactly where the text ends, which is where a parser that looks one byte too
// far is caught.  All three must give the same sums.  The records are printed whole and site by site into buffers of exactly their size;
// both must give the same bytes.  Prints per file
//   <file> records <n> events <sum of n> fnv <hash of the sums> text <bytes> tfnv <hash of the records>
// and at the end the site count and the header's hash.  Then lines that are no SAM record: each must be refused with a message, and
// nothing of them added.  Exit 0, or 1 with the reason.
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/salt_host.h"

static bool slurp(const char *fn, std::string &out)
{
    gzFile f = gzopen(fn, "rb");                                       // (reads plain files as they are)
    if (!f) return false;
    char buf[1 << 16]; int n;
    while ((n = gzread(f, buf, sizeof buf)) > 0) out.append(buf, (size_t)n);
    gzclose(f);
    return n == 0;
}

static uint64_t fnv_bytes(const void *p, size_t n, uint64_t h = 1469598103934665603ull)
{
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: genotype_model <index prefix> <min_mapq> <file.sam[.gz]>...\n"); return 1; }
    salt_index_t *ix = salt_index_load(argv[1], 1);
    if (!ix) { fprintf(stderr, "%s\n", salt_host_last_error()); return 1; }
    const uint32_t min_mapq = (uint32_t)atoi(argv[2]);
    const int64_t n_sites = salt_snp_sites(ix, nullptr, 0);
    for (int a = 3; a < argc; ++a) {
        std::string sam;
        if (!slurp(argv[a], sam)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
        std::vector<salt_gt_site_t> whole((size_t)n_sites), pieces(whole), lines(whole);      // exactly n_sites: one more written is an overflow
        const int64_t n_rec = salt_gt_add_sam(ix, sam.data(), sam.size(), min_mapq, whole.data(), (uint64_t)n_sites);
        if (n_rec < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
        int64_t n_pieces = 0, n_lines = 0;
        for (size_t at = 0; at < sam.size(); ) {                       // pieces of about 4 KiB, each a heap buffer of its own size
            size_t end = at + 4096 < sam.size() ? at + 4096 : sam.size();
            while (end < sam.size() && sam[end - 1] != '\n') ++end;
            const std::vector<char> piece(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_gt_add_sam(ix, piece.data(), piece.size(), min_mapq, pieces.data(), (uint64_t)n_sites);
            if (r < 0) { fprintf(stderr, "%s (piece at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_pieces += r; at = end;
        }
        for (size_t at = 0; at < sam.size(); ) {                       // one line a call, without its newline
            const char *nl = (const char *)memchr(sam.data() + at, '\n', sam.size() - at);
            const size_t end = nl ? (size_t)(nl - sam.data()) : sam.size();
            const std::vector<char> line(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_gt_add_sam(ix, line.data(), line.size(), min_mapq, lines.data(), (uint64_t)n_sites);
            if (r < 0) { fprintf(stderr, "%s (line at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_lines += r; at = end + 1;
        }
        const size_t bytes = whole.size() * sizeof(salt_gt_site_t);
        if (memcmp(pieces.data(), whole.data(), bytes) || memcmp(lines.data(), whole.data(), bytes) || n_pieces != n_rec || n_lines != n_rec) {
            fprintf(stderr, "%s: the pieces do not add up to the whole\n", argv[a]); return 1;
        }
        // the records: whole into a buffer of exactly their size, then site by site, each into a buffer of its own size
        const int64_t need = salt_gt_text(ix, whole.data(), 0, (uint64_t)n_sites, nullptr, 0);
        if (need < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
        std::vector<char> text((size_t)need), by_site;
        if (salt_gt_text(ix, whole.data(), 0, (uint64_t)n_sites, text.data(), (uint64_t)need) != need) { fprintf(stderr, "the text changed its size\n"); return 1; }
        for (int64_t s = 0; s < n_sites; ++s) {
            const int64_t one = salt_gt_text(ix, &whole[(size_t)s], (uint64_t)s, 1, nullptr, 0);
            if (one <= 0) { fprintf(stderr, "site %lld has no record\n", (long long)s); return 1; }
            std::vector<char> rec((size_t)one), cut((size_t)one - 1, 'x');
            if (salt_gt_text(ix, &whole[(size_t)s], (uint64_t)s, 1, rec.data(), (uint64_t)one) != one) { fprintf(stderr, "a record changed its size\n"); return 1; }
            if (salt_gt_text(ix, &whole[(size_t)s], (uint64_t)s, 1, cut.data(), (uint64_t)one - 1) != one || memcmp(cut.data(), rec.data(), (size_t)one - 1)) {   // cap below the size
                fprintf(stderr, "cap not respected\n"); return 1;
            }
            by_site.insert(by_site.end(), rec.begin(), rec.end());
        }
        if (by_site != text) { fprintf(stderr, "%s: the records site by site are not the whole text\n", argv[a]); return 1; }
        uint64_t events = 0;
        for (const salt_gt_site_t &s : whole) for (int b = 0; b < 4; ++b) events += s.b[b].n;
        printf("%s records %lld events %llu fnv %llu text %lld tfnv %llu\n", argv[a], (long long)n_rec, (unsigned long long)events,
               (unsigned long long)fnv_bytes(whole.data(), bytes), (long long)need, (unsigned long long)fnv_bytes(text.data(), text.size()));
    }
    const int64_t hn = salt_gt_header(ix, "NA12878", nullptr, 0);
    std::vector<char> head((size_t)(hn > 0 ? hn : 0));
    if (hn <= 0 || salt_gt_header(ix, "NA12878", head.data(), (uint64_t)hn) != hn) { fprintf(stderr, "no header\n"); return 1; }
    printf("sites %lld header %lld hfnv %llu\n", (long long)n_sites, (long long)hn, (unsigned long long)fnv_bytes(head.data(), head.size()));
    // what is no record of this program is refused, and nothing is added from the line; a line whose CIGAR or QUAL is bad behind good M columns too
    static const char *const bad[] = { "x", "r\t0", "r\t0\tlambdaA\t1\t9\t", "r\t0\tlambdaA\t1\t9\t4M\t*\t0\t0\tACG\tIII", "r\t0\tlambdaA\t1\t9\tM\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t9\t4\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t0\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t9\t2I3S\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\t*\t1\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t70000\tlambdaA\t1\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t300\t4M\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t9\t999999999M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t9\t4M\t*\t0\t0\tACGT\tIII", "r\t0\tlambdaA\t1\t9\t4M\t*\t0\t0\tACGT\tIIIII" };
    std::vector<salt_gt_site_t> none((size_t)n_sites);
    for (const char *b : bad) {
        const std::vector<char> line(b, b + strlen(b));
        if (salt_gt_add_sam(ix, line.data(), line.size(), 0, none.data(), (uint64_t)n_sites) >= 0) { fprintf(stderr, "accepted: %s\n", b); return 1; }
        if (strncmp(salt_host_last_error(), "genotype: ", 10) != 0) { fprintf(stderr, "no message for: %s\n", b); return 1; }
    }
    // long M runs over many sites, then a CIGAR that outgrows SEQ: refused whole
    {
        std::string seq(600, 'A'), line = "r\t0\tlambdaA\t1\t9\t500M200M\t*\t0\t0\t" + seq + "\t" + std::string(600, 'I');
        if (salt_gt_add_sam(ix, line.data(), line.size(), 0, none.data(), (uint64_t)n_sites) >= 0) { fprintf(stderr, "accepted a CIGAR longer than SEQ\n"); return 1; }
    }
    if (salt_gt_add_sam(ix, nullptr, 0, 0, none.data(), (uint64_t)n_sites) != 0) { fprintf(stderr, "an empty text is no error\n"); return 1; }
    if (salt_gt_add_sam(ix, "x", 1, 0, none.data(), (uint64_t)n_sites + 1) >= 0) { fprintf(stderr, "a table of another size was accepted\n"); return 1; }
    if (salt_gt_text(ix, none.data(), (uint64_t)n_sites, 1, nullptr, 0) >= 0 || salt_gt_text(ix, none.data(), 1, (uint64_t)n_sites, nullptr, 0) >= 0) {
        fprintf(stderr, "a range beyond the sites was accepted\n"); return 1;
    }
    for (const salt_gt_site_t &s : none) for (int b = 0; b < 4; ++b) if (s.b[b].n | s.b[b].sm | s.b[b].sx | s.b[b].sh) { fprintf(stderr, "a refused line was added\n"); return 1; }
    printf("refused %zu\n", sizeof bad / sizeof bad[0] + 1);
    salt_index_free(ix);
    return 0;
}
