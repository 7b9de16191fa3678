// tools/snp_counts_model.cc -- the host twin of the SNP-site counts (salt_snp_sites / salt_snp_count_sam of salt_amd/host/salt_host.cc) as a
// stand-alone program, so that it can run under AddressSanitizer + UBSan (tests/test_snp_counts_model.py builds it together with salt_host.cc).
//
//   snp_counts_model <index prefix> <min_mapq> <file.sam | file.sam.gz>...
//
// Per file: the text whole, then the same text in pieces cut at line ends (a run counts block by block), then line by line with every
// line also handed over WITHOUT its newline and the file's last byte dropped -- buffers that end exactly where the text ends, which is
// where a parser that looks one byte too far is caught.  All three must give the same table.  Prints per file
//   <file> records <n> bases <sum> sites_hit <n> max <deepest site> fnv <hash of the table>
// and at the end the site count.  Then lines that are no SAM record: each must be refused with a message.  Exit 0, or 1 with the reason.
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

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: snp_counts_model <index prefix> <min_mapq> <file.sam[.gz]>...\n"); return 1; }
    salt_index_t *ix = salt_index_load(argv[1], 1);
    if (!ix) { fprintf(stderr, "%s\n", salt_host_last_error()); return 1; }
    const uint32_t min_mapq = (uint32_t)atoi(argv[2]);
    const int64_t n_sites = salt_snp_sites(ix, nullptr, 0);
    std::vector<uint32_t> pos((size_t)n_sites);                        // exactly n_sites entries: one more written is an overflow
    if (salt_snp_sites(ix, pos.data(), (uint64_t)n_sites) != n_sites) { fprintf(stderr, "site count changed\n"); return 1; }
    for (size_t i = 1; i < pos.size(); ++i) if (pos[i] <= pos[i - 1]) { fprintf(stderr, "sites not ascending\n"); return 1; }
    std::vector<uint32_t> few(3, 0xDEADBEEFu);                          // cap below n_sites: only cap entries are written
    salt_snp_sites(ix, few.data(), 2);
    if (n_sites >= 2 && (few[0] != pos[0] || few[1] != pos[1] || few[2] != 0xDEADBEEFu)) { fprintf(stderr, "cap not respected\n"); return 1; }
    for (int a = 3; a < argc; ++a) {
        std::string sam;
        if (!slurp(argv[a], sam)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
        std::vector<uint32_t> whole((size_t)n_sites * 4, 0), pieces(whole), lines(whole);
        const int64_t n_rec = salt_snp_count_sam(ix, sam.data(), sam.size(), min_mapq, whole.data(), (uint64_t)n_sites);
        if (n_rec < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
        int64_t n_pieces = 0, n_lines = 0;
        for (size_t at = 0; at < sam.size(); ) {                       // pieces of about 4 KiB, each a heap buffer of its own size
            size_t end = at + 4096 < sam.size() ? at + 4096 : sam.size();
            while (end < sam.size() && sam[end - 1] != '\n') ++end;
            const std::vector<char> piece(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_snp_count_sam(ix, piece.data(), piece.size(), min_mapq, pieces.data(), (uint64_t)n_sites);
            if (r < 0) { fprintf(stderr, "%s (piece at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_pieces += r; at = end;
        }
        for (size_t at = 0; at < sam.size(); ) {                       // one line a call, without its newline
            const char *nl = (const char *)memchr(sam.data() + at, '\n', sam.size() - at);
            const size_t end = nl ? (size_t)(nl - sam.data()) : sam.size();
            const std::vector<char> line(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_snp_count_sam(ix, line.data(), line.size(), min_mapq, lines.data(), (uint64_t)n_sites);
            if (r < 0) { fprintf(stderr, "%s (line at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_lines += r; at = end + 1;
        }
        if (pieces != whole || lines != whole || n_pieces != n_rec || n_lines != n_rec) { fprintf(stderr, "%s: the pieces do not add up to the whole\n", argv[a]); return 1; }
        uint64_t bases = 0, hit = 0, deepest = 0, fnv = 1469598103934665603ull;
        for (int64_t s = 0; s < n_sites; ++s) {
            uint64_t here = 0;
            for (int b = 0; b < 4; ++b) { const uint32_t c = whole[(size_t)s * 4 + (size_t)b]; here += c; fnv = (fnv ^ c) * 1099511628211ull; }
            bases += here; hit += here != 0; if (here > deepest) deepest = here;
        }
        printf("%s records %lld bases %llu sites_hit %llu max %llu fnv %llu\n", argv[a], (long long)n_rec, (unsigned long long)bases, (unsigned long long)hit,
               (unsigned long long)deepest, (unsigned long long)fnv);
    }
    printf("sites %lld\n", (long long)n_sites);
    // what is no record of this program is refused, and nothing is counted from the line
    static const char *const bad[] = { "x", "r\t0", "r\t0\tlambdaA\t1\t9\t", "r\t0\tlambdaA\t1\t9\t4M\t*\t0\t0\tACG\tIII", "r\t0\tlambdaA\t1\t9\tM\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t9\t4\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t0\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t9\t2I3S\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\t*\t1\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t70000\tlambdaA\t1\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t300\t4M\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t9\t999999999M\t*\t0\t0\tACGT\tIIII" };
    std::vector<uint32_t> none((size_t)n_sites * 4, 0);
    for (const char *b : bad) {
        const std::vector<char> line(b, b + strlen(b));
        if (salt_snp_count_sam(ix, line.data(), line.size(), 0, none.data(), (uint64_t)n_sites) >= 0) { fprintf(stderr, "accepted: %s\n", b); return 1; }
        if (strncmp(salt_host_last_error(), "snp counts: ", 12) != 0) { fprintf(stderr, "no message for: %s\n", b); return 1; }
    }
    if (salt_snp_count_sam(ix, nullptr, 0, 0, none.data(), (uint64_t)n_sites) != 0) { fprintf(stderr, "an empty text is no error\n"); return 1; }
    if (salt_snp_count_sam(ix, "x", 1, 0, none.data(), (uint64_t)n_sites + 1) >= 0) { fprintf(stderr, "a table of another size was accepted\n"); return 1; }
    for (uint32_t c : none) if (c) { fprintf(stderr, "a refused line was counted\n"); return 1; }
    printf("refused %zu\n", sizeof bad / sizeof bad[0]);
    salt_index_free(ix);
    return 0;
}
