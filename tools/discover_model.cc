// tools/discover_model.cc -- the host twin of the SNP candidate arrays and its printer (salt_disc_add_sam / salt_disc_text of
// salt_amd/host/salt_host.cc) as a stand-alone program, so that it can run under AddressSanitizer + UBSan (tests/test_discover_model.py
// builds it together with salt_host.cc).
//
//   discover_model <index prefix> <min_mapq> <min_baseq> <file.sam | file.sam.gz>...
//
// Per file: the text whole, then the same text in pieces cut at line ends (a run counts block by block), then line by line with every
// line handed over WITHOUT its newline -- buffers that end exactly where the text ends.  All three must give the same arrays, which have
// exactly ref_len and ref_len + 1 words.  Every text (min_alt / min_pct 1 / 0, 2 / 10 and the defaults, with and without all) goes into a
// buffer of exactly its size, and into one a byte shorter.  Prints per file
//   <file> records <n> events <sum of the fields> afnv <hash of alt> dfnv <hash of diff> then per text: text <bytes> tfnv <hash>
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

struct Arrays {
    std::vector<uint64_t> alt; std::vector<uint32_t> diff;             // exactly ref_len and ref_len + 1: one more written is an overflow
    explicit Arrays(size_t n) : alt(n), diff(n + 1) {}
    bool operator==(const Arrays &o) const { return alt == o.alt && diff == o.diff; }
};

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: discover_model <index prefix> <min_mapq> <min_baseq> <file.sam[.gz]>...\n"); return 1; }
    salt_index_t *ix = salt_index_load(argv[1], 1);
    if (!ix) { fprintf(stderr, "%s\n", salt_host_last_error()); return 1; }
    const uint32_t min_mapq = (uint32_t)atoi(argv[2]), min_baseq = (uint32_t)atoi(argv[3]);
    const uint64_t n_pos = salt_index_host_view(ix)->ref_len;
    const int n_seqs = salt_index_n_seqs(ix);
    for (int a = 4; a < argc; ++a) {
        std::string sam;
        if (!slurp(argv[a], sam)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
        Arrays whole((size_t)n_pos), pieces((size_t)n_pos), lines((size_t)n_pos);
        const int64_t n_rec = salt_disc_add_sam(ix, sam.data(), sam.size(), min_mapq, min_baseq, whole.alt.data(), whole.diff.data(), n_pos);
        if (n_rec < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
        int64_t n_pieces = 0, n_lines = 0;
        for (size_t at = 0; at < sam.size(); ) {                       // pieces of about 4 KiB, each a heap buffer of its own size
            size_t end = at + 4096 < sam.size() ? at + 4096 : sam.size();
            while (end < sam.size() && sam[end - 1] != '\n') ++end;
            const std::vector<char> piece(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_disc_add_sam(ix, piece.data(), piece.size(), min_mapq, min_baseq, pieces.alt.data(), pieces.diff.data(), n_pos);
            if (r < 0) { fprintf(stderr, "%s (piece at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_pieces += r; at = end;
        }
        for (size_t at = 0; at < sam.size(); ) {                       // one line a call, without its newline
            const char *nl = (const char *)memchr(sam.data() + at, '\n', sam.size() - at);
            const size_t end = nl ? (size_t)(nl - sam.data()) : sam.size();
            const std::vector<char> line(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_disc_add_sam(ix, line.data(), line.size(), min_mapq, min_baseq, lines.alt.data(), lines.diff.data(), n_pos);
            if (r < 0) { fprintf(stderr, "%s (line at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_lines += r; at = end + 1;
        }
        if (!(pieces == whole) || !(lines == whole) || n_pieces != n_rec || n_lines != n_rec) { fprintf(stderr, "%s: the pieces do not add up to the whole\n", argv[a]); return 1; }
        uint64_t events = 0;
        for (uint64_t w : whole.alt) events += (w & SALT_DISC_FIELD_MAX) + ((w >> 21) & SALT_DISC_FIELD_MAX) + ((w >> 42) & SALT_DISC_FIELD_MAX);
        printf("%s records %lld events %llu afnv %llu dfnv %llu", argv[a], (long long)n_rec, (unsigned long long)events,
               (unsigned long long)fnv_bytes(whole.alt.data(), whole.alt.size() * 8), (unsigned long long)fnv_bytes(whole.diff.data(), whole.diff.size() * 4));
        static const uint32_t rules[3][2] = { { 1, 0 }, { 2, 10 }, { 3, 20 } };
        for (const auto &rule : rules)
            for (int all = 0; all < 2; ++all) {
                const int64_t need = salt_disc_text(ix, whole.alt.data(), whole.diff.data(), n_pos, rule[0], rule[1], all, nullptr, 0, nullptr);
                if (need < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
                std::vector<char> text((size_t)need), cut((size_t)(need > 0 ? need - 1 : 0), 'x');
                std::vector<uint8_t> seen((size_t)n_seqs);             // exactly a byte a sequence
                if (salt_disc_text(ix, whole.alt.data(), whole.diff.data(), n_pos, rule[0], rule[1], all, text.data(), (uint64_t)need, seen.data()) != need) { fprintf(stderr, "the text changed its size\n"); return 1; }
                if (salt_disc_text(ix, whole.alt.data(), whole.diff.data(), n_pos, rule[0], rule[1], all, cut.data(), cut.size(), nullptr) != need || (!cut.empty() && memcmp(cut.data(), text.data(), cut.size()))) {
                    fprintf(stderr, "cap not respected\n"); return 1;
                }
                printf(" text %lld tfnv %llu", (long long)need, (unsigned long long)fnv_bytes(text.data(), text.size()));
            }
        printf("\n");
    }
    // what is no record of this program is refused, and nothing is added from the line; a line whose CIGAR or QUAL is bad behind good M columns too
    static const char *const bad[] = { "x", "r\t0", "r\t0\tlambdaA\t1\t99\t", "r\t0\tlambdaA\t1\t99\t4M\t*\t0\t0\tACG\tIII", "r\t0\tlambdaA\t1\t99\tM\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t99\t4\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t0\t99\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t99\t2I3S\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\t*\t1\t99\t4M\t*\t0\t0\tACGT\tIIII", "r\t70000\tlambdaA\t1\t99\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t300\t4M\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t99\t999999999M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t99\t4M\t*\t0\t0\tACGT\tIII", "r\t0\tlambdaA\t1\t99\t4M\t*\t0\t0\tACGT\tIIIII" };
    Arrays none((size_t)n_pos);
    for (const char *b : bad) {
        const std::vector<char> line(b, b + strlen(b));
        if (salt_disc_add_sam(ix, line.data(), line.size(), 0, 0, none.alt.data(), none.diff.data(), n_pos) >= 0) { fprintf(stderr, "accepted: %s\n", b); return 1; }
        if (strncmp(salt_host_last_error(), "discover: ", 10) != 0) { fprintf(stderr, "no message for: %s\n", b); return 1; }
    }
    {   // long M runs, then a CIGAR that outgrows SEQ: refused whole
        std::string seq(600, 'T'), line = "r\t0\tlambdaA\t1\t99\t500M200M\t*\t0\t0\t" + seq + "\t" + std::string(600, 'I');
        if (salt_disc_add_sam(ix, line.data(), line.size(), 0, 0, none.alt.data(), none.diff.data(), n_pos) >= 0) { fprintf(stderr, "accepted a CIGAR longer than SEQ\n"); return 1; }
    }
    if (salt_disc_add_sam(ix, nullptr, 0, 0, 0, none.alt.data(), none.diff.data(), n_pos) != 0) { fprintf(stderr, "an empty text is no error\n"); return 1; }
    if (salt_disc_add_sam(ix, "x", 1, 0, 0, none.alt.data(), none.diff.data(), n_pos + 1) >= 0) { fprintf(stderr, "arrays of another size were accepted\n"); return 1; }
    if (salt_disc_text(ix, none.alt.data(), none.diff.data(), n_pos, 0, 20, 0, nullptr, 0, nullptr) >= 0 || salt_disc_text(ix, none.alt.data(), none.diff.data(), n_pos, 3, 101, 0, nullptr, 0, nullptr) >= 0) {
        fprintf(stderr, "a call rule outside its range was accepted\n"); return 1;
    }
    if (!(none == Arrays((size_t)n_pos))) { fprintf(stderr, "a refused line was added\n"); return 1; }
    {   // a record that reaches past the genome's end is cut: the last position and diff[ref_len] are the last words written
        int64_t off = 0; int32_t len = 0; const char *name = nullptr;
        salt_index_seq(ix, n_seqs - 1, &off, &len, &name);
        const std::string line = std::string("r\t16\t") + name + "\t" + std::to_string(len - 4) + "\t99\t40M\t*\t0\t0\t" + std::string(40, 'G') + "\t" + std::string(40, '5');
        if (salt_disc_add_sam(ix, line.data(), line.size(), 0, 0, none.alt.data(), none.diff.data(), n_pos) != 1 || none.diff[(size_t)n_pos] != 0xFFFFFFFFu || none.diff[(size_t)n_pos - 5] != 1u) {
            fprintf(stderr, "a record past the genome's end was not cut\n"); return 1;
        }
    }
    printf("refused %zu\n", sizeof bad / sizeof bad[0] + 1);
    salt_index_free(ix);
    return 0;
}
