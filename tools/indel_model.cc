// tools/indel_model.cc -- the host twin of the indel table and its printer (salt_indel_add_sam / salt_indel_entries / salt_indel_text /
// salt_indel_header of salt_amd/host/salt_host.cc) as a stand-alone program, so that it can run under AddressSanitizer + UBSan
// (tests/test_indel_model.py builds it together with salt_host.cc).
//
//   indel_model <index prefix> <min_mapq> <file.sam | file.sam.gz>...
//
// Per file: the text whole, then the same text in pieces cut at line ends (a run counts block by block), then line by line with every
// line handed over WITHOUT its newline -- buffers that end exactly where the text ends.  All three must give the same entries, counters
// and difference array, which has exactly ref_len + 1 words; the entries go into a buffer of exactly their size.  Every text (min_alt /
// min_pct 1 / 0, 2 / 10 and the defaults) and the header go into a buffer of exactly their size, and into one a byte shorter.  Prints per
// file
//   <file> records <n> stats <tabled> <dropped> <long> <unanchored> entries <n> efnv <hash of the pairs> dfnv <hash of diff>
//   then per text: text <bytes> tfnv <hash>; then: header <bytes> hfnv <hash>
// Then lines that are no SAM record: each must be refused with a message, and nothing of them added.  Exit 0, or 1 with the reason.
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

struct Table {
    salt_indel_t *t; std::vector<uint32_t> diff;                       // exactly ref_len + 1 words: one more written is an overflow
    explicit Table(size_t n) : t(salt_indel_new()), diff(n + 1) {}
    Table(const Table &) = delete;
    ~Table() { salt_indel_free(t); }
    std::vector<uint64_t> entries() const
    {
        const int64_t n = salt_indel_entries(t, nullptr, 0);
        std::vector<uint64_t> e((size_t)n * 2);                        // exactly the pairs
        if (salt_indel_entries(t, e.data(), (uint64_t)n) != n) abort();
        return e;
    }
    std::vector<uint64_t> stats() const { std::vector<uint64_t> s(4); salt_indel_stats(t, s.data()); return s; }
    bool same(const Table &o) const { return entries() == o.entries() && stats() == o.stats() && diff == o.diff; }
};

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: indel_model <index prefix> <min_mapq> <file.sam[.gz]>...\n"); return 1; }
    salt_index_t *ix = salt_index_load(argv[1], 1);
    if (!ix) { fprintf(stderr, "%s\n", salt_host_last_error()); return 1; }
    const uint32_t min_mapq = (uint32_t)atoi(argv[2]);
    const uint64_t n_pos = salt_index_host_view(ix)->ref_len;
    const int n_seqs = salt_index_n_seqs(ix);
    for (int a = 3; a < argc; ++a) {
        std::string sam;
        if (!slurp(argv[a], sam)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
        Table whole((size_t)n_pos), pieces((size_t)n_pos), lines((size_t)n_pos);
        const int64_t n_rec = salt_indel_add_sam(ix, whole.t, sam.data(), sam.size(), min_mapq, whole.diff.data(), n_pos);
        if (n_rec < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
        int64_t n_pieces = 0, n_lines = 0;
        for (size_t at = 0; at < sam.size(); ) {                       // pieces of about 4 KiB, each a heap buffer of its own size
            size_t end = at + 4096 < sam.size() ? at + 4096 : sam.size();
            while (end < sam.size() && sam[end - 1] != '\n') ++end;
            const std::vector<char> piece(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_indel_add_sam(ix, pieces.t, piece.data(), piece.size(), min_mapq, pieces.diff.data(), n_pos);
            if (r < 0) { fprintf(stderr, "%s (piece at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_pieces += r; at = end;
        }
        for (size_t at = 0; at < sam.size(); ) {                       // one line a call, without its newline
            const char *nl = (const char *)memchr(sam.data() + at, '\n', sam.size() - at);
            const size_t end = nl ? (size_t)(nl - sam.data()) : sam.size();
            const std::vector<char> line(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_indel_add_sam(ix, lines.t, line.data(), line.size(), min_mapq, lines.diff.data(), n_pos);
            if (r < 0) { fprintf(stderr, "%s (line at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_lines += r; at = end + 1;
        }
        if (!pieces.same(whole) || !lines.same(whole) || n_pieces != n_rec || n_lines != n_rec) { fprintf(stderr, "%s: the pieces do not add up to the whole\n", argv[a]); return 1; }
        const std::vector<uint64_t> e = whole.entries(), st = whole.stats();
        printf("%s records %lld stats %llu %llu %llu %llu entries %zu efnv %llu dfnv %llu", argv[a], (long long)n_rec, (unsigned long long)st[0], (unsigned long long)st[1],
               (unsigned long long)st[2], (unsigned long long)st[3], e.size() / 2, (unsigned long long)fnv_bytes(e.data(), e.size() * 8),
               (unsigned long long)fnv_bytes(whole.diff.data(), whole.diff.size() * 4));
        static const uint32_t rules[3][2] = { { 1, 0 }, { 2, 10 }, { 3, 20 } };
        for (const auto &rule : rules) {
            const int64_t need = salt_indel_text(ix, e.data(), e.size() / 2, whole.diff.data(), n_pos, rule[0], rule[1], nullptr, 0);
            if (need < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
            std::vector<char> text((size_t)need), cut((size_t)(need > 0 ? need - 1 : 0), 'x');
            if (salt_indel_text(ix, e.data(), e.size() / 2, whole.diff.data(), n_pos, rule[0], rule[1], text.data(), (uint64_t)need) != need) { fprintf(stderr, "the text changed its size\n"); return 1; }
            if (salt_indel_text(ix, e.data(), e.size() / 2, whole.diff.data(), n_pos, rule[0], rule[1], cut.data(), cut.size()) != need || (!cut.empty() && memcmp(cut.data(), text.data(), cut.size()))) {
                fprintf(stderr, "cap not respected\n"); return 1;
            }
            printf(" text %lld tfnv %llu", (long long)need, (unsigned long long)fnv_bytes(text.data(), text.size()));
        }
        const int64_t hn = salt_indel_header(ix, min_mapq, 3, 20, st[1], nullptr, 0);
        std::vector<char> head((size_t)(hn > 0 ? hn : 0)), hcut((size_t)(hn > 0 ? hn - 1 : 0));
        if (hn <= 0 || salt_indel_header(ix, min_mapq, 3, 20, st[1], head.data(), (uint64_t)hn) != hn || salt_indel_header(ix, min_mapq, 3, 20, st[1], hcut.data(), hcut.size()) != hn) {
            fprintf(stderr, "the header changed its size\n"); return 1;
        }
        printf(" header %lld hfnv %llu\n", (long long)hn, (unsigned long long)fnv_bytes(head.data(), head.size()));
    }
    // what is no record of this program is refused, and nothing is added from the line; a line whose CIGAR is bad behind a good indel too
    static const char *const bad[] = { "x", "r\t0", "r\t0\tlambdaA\t1\t99\t", "r\t0\tlambdaA\t1\t99\t4M\t*\t0\t0\tACG\tIII", "r\t0\tlambdaA\t1\t99\tM\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t99\t4\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t0\t99\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t99\t2I3S\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\t*\t1\t99\t4M\t*\t0\t0\tACGT\tIIII", "r\t70000\tlambdaA\t1\t99\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t300\t4M\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t99\t999999999M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t100\t99\t2M1I1M2D1M\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t100\t99\t2M1D2M1N1M\t*\t0\t0\tACGTA\tIIIII", "r\t0\tlambdaA\t100\t99\t2M1I2M1I\t*\t0\t0\tACGTA\tIIIII" };
    Table none((size_t)n_pos);
    for (const char *b : bad) {
        const std::vector<char> line(b, b + strlen(b));
        if (salt_indel_add_sam(ix, none.t, line.data(), line.size(), 0, none.diff.data(), n_pos) >= 0) { fprintf(stderr, "accepted: %s\n", b); return 1; }
        if (strncmp(salt_host_last_error(), "indels: ", 8) != 0) { fprintf(stderr, "no message for: %s\n", b); return 1; }
    }
    if (salt_indel_add_sam(ix, none.t, nullptr, 0, 0, none.diff.data(), n_pos) != 0) { fprintf(stderr, "an empty text is no error\n"); return 1; }
    if (salt_indel_add_sam(ix, none.t, "x", 1, 0, none.diff.data(), n_pos + 1) >= 0) { fprintf(stderr, "an array of another size was accepted\n"); return 1; }
    const uint64_t one[2] = { 1ull << 63 | 5ull << 31 | 1ull << 30 | 1ull << 24, 3 }, two[4] = { one[0], 3, one[0], 3 };
    if (salt_indel_text(ix, one, 1, none.diff.data(), n_pos, 0, 20, nullptr, 0) >= 0 || salt_indel_text(ix, one, 1, none.diff.data(), n_pos, 3, 101, nullptr, 0) >= 0 ||
        salt_indel_text(ix, two, 2, none.diff.data(), n_pos, 3, 20, nullptr, 0) >= 0 || salt_indel_text(ix, one, 1, none.diff.data(), n_pos, 3, 20, nullptr, 0) <= 0) {
        fprintf(stderr, "a call rule outside its range or pairs out of order were accepted\n"); return 1;
    }
    if (!none.same(Table((size_t)n_pos))) { fprintf(stderr, "a refused line was added\n"); return 1; }
    {   // the genome's edges, each line a heap buffer of its own size: a deletion that ends on the last contig's last base is tabled and its
        // REF is printed up to the genome's last letter; a record that reaches past the genome's end is cut in diff
        int64_t off = 0; int32_t len = 0; const char *name = nullptr;
        salt_index_seq(ix, n_seqs - 1, &off, &len, &name);
        const std::string l1 = std::string("r\t16\t") + name + "\t" + std::to_string(len - 72) + "\t99\t8M63D2M\t*\t0\t0\t" + std::string(10, 'G') + "\t*";
        const std::string l2 = std::string("r\t0\t") + name + "\t" + std::to_string(len - 4) + "\t99\t3M2I35M\t*\t0\t0\t" + std::string(40, 'G') + "\t*";
        for (const std::string &l : { l1, l2 }) {
            const std::vector<char> line(l.begin(), l.end());
            if (salt_indel_add_sam(ix, none.t, line.data(), line.size(), 0, none.diff.data(), n_pos) != 1) { fprintf(stderr, "%s\n", salt_host_last_error()); return 1; }
        }
        const std::vector<uint64_t> e = none.entries(), st = none.stats();
        if (none.diff[(size_t)n_pos] != 0xFFFFFFFEu || st[0] != 2 || e.size() != 4) { fprintf(stderr, "the records at the genome's end: tabled %llu\n", (unsigned long long)st[0]); return 1; }
        const int64_t need = salt_indel_text(ix, e.data(), 2, none.diff.data(), n_pos, 1, 0, nullptr, 0);
        std::vector<char> text((size_t)(need > 0 ? need : 0));
        if (need <= 0 || salt_indel_text(ix, e.data(), 2, none.diff.data(), n_pos, 1, 0, text.data(), (uint64_t)need) != need) { fprintf(stderr, "the text at the genome's end\n"); return 1; }
    }
    printf("refused %zu\n", sizeof bad / sizeof bad[0]);
    salt_index_free(ix);
    return 0;
}
