// tools/depth_model.cc -- the host twins of the coverage (salt_depth_add_sam / salt_depth_text of salt_amd/host/salt_host.cc) as a stand-alone
// program, so that they can run under AddressSanitizer + UBSan (tests/test_depth_model.py builds it together with salt_host.cc).
//
//   depth_model <index prefix> <min_mapq> <file.sam | file.sam.gz>...
//
// Per file: the text whole, then the same text in pieces cut at line ends (a run adds block by block), then line by line with every line
// handed over WITHOUT its newline -- buffers that end exactly where the text ends, which is where a parser that looks one byte too far is
// caught.  All three must give the same array.  Then the array's texts, per base and for several windows, each into a buffer of exactly
// its size; a buffer one byte short must be left alone beyond its end.  Prints per file
//   <file> records <n> sum <checksum of the array> base <bytes> <checksum> w<W> <bytes> <checksum> ...
// Then lines that are no SAM record: each must be refused with a message and add nothing.  Exit 0, or 1 with the reason.
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

// sum of (i + 1) * byte i, mod 2^64: a position-weighted checksum a test can form with array arithmetic
static uint64_t wsum(const void *p, size_t n)
{
    uint64_t h = 0;
    for (size_t i = 0; i < n; ++i) h += (uint64_t)(i + 1) * ((const uint8_t *)p)[i];
    return h;
}

static const uint32_t WINDOWS[] = { 0, 1, 7, 64, 1000, 48502, 100000 };

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: depth_model <index prefix> <min_mapq> <file.sam[.gz]>...\n"); return 1; }
    salt_index_t *ix = salt_index_load(argv[1], 1);
    if (!ix) { fprintf(stderr, "%s\n", salt_host_last_error()); return 1; }
    const uint32_t min_mapq = (uint32_t)atoi(argv[2]);
    const uint64_t n_words = (uint64_t)salt_index_host_view(ix)->ref_len + 1;
    for (int a = 3; a < argc; ++a) {
        std::string sam;
        if (!slurp(argv[a], sam)) { fprintf(stderr, "cannot read %s\n", argv[a]); return 1; }
        std::vector<uint32_t> whole((size_t)n_words, 0), pieces(whole), lines(whole);      // exactly ref_len + 1 words: one more written is an overflow
        const int64_t n_rec = salt_depth_add_sam(ix, sam.data(), sam.size(), min_mapq, whole.data(), n_words);
        if (n_rec < 0) { fprintf(stderr, "%s: %s\n", argv[a], salt_host_last_error()); return 1; }
        int64_t n_pieces = 0, n_lines = 0;
        for (size_t at = 0; at < sam.size(); ) {                       // pieces of about 4 KiB, each a heap buffer of its own size
            size_t end = at + 4096 < sam.size() ? at + 4096 : sam.size();
            while (end < sam.size() && sam[end - 1] != '\n') ++end;
            const std::vector<char> piece(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_depth_add_sam(ix, piece.data(), piece.size(), min_mapq, pieces.data(), n_words);
            if (r < 0) { fprintf(stderr, "%s (piece at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_pieces += r; at = end;
        }
        for (size_t at = 0; at < sam.size(); ) {                       // one line a call, without its newline
            const char *nl = (const char *)memchr(sam.data() + at, '\n', sam.size() - at);
            const size_t end = nl ? (size_t)(nl - sam.data()) : sam.size();
            const std::vector<char> line(sam.begin() + (long)at, sam.begin() + (long)end);
            const int64_t r = salt_depth_add_sam(ix, line.data(), line.size(), min_mapq, lines.data(), n_words);
            if (r < 0) { fprintf(stderr, "%s (line at %zu): %s\n", argv[a], at, salt_host_last_error()); return 1; }
            n_lines += r; at = end + 1;
        }
        if (pieces != whole || lines != whole || n_pieces != n_rec || n_lines != n_rec) { fprintf(stderr, "%s: the pieces do not add up to the whole\n", argv[a]); return 1; }
        printf("%s records %lld sum %llu", argv[a], (long long)n_rec, (unsigned long long)wsum(whole.data(), whole.size() * 4));
        for (uint32_t w : WINDOWS) {
            const int64_t need = salt_depth_text(ix, whole.data(), n_words, w, nullptr, 0);
            if (need <= 0) { fprintf(stderr, "%s: no text: %s\n", argv[a], salt_host_last_error()); return 1; }
            std::vector<char> text((size_t)need);                      // exactly the text's size
            if (salt_depth_text(ix, whole.data(), n_words, w, text.data(), (uint64_t)need) != need) { fprintf(stderr, "%s: the text's size changed\n", argv[a]); return 1; }
            std::vector<char> shorter((size_t)need - 1);               // one byte short: the size comes back, the buffer holds the text's front
            if (salt_depth_text(ix, whole.data(), n_words, w, shorter.data(), (uint64_t)need - 1) != need || memcmp(shorter.data(), text.data(), shorter.size()) != 0) {
                fprintf(stderr, "%s: a short buffer was not filled with the text's front\n", argv[a]); return 1;
            }
            if (w) printf(" w%u %lld %llu", w, (long long)need, (unsigned long long)wsum(text.data(), text.size()));
            else printf(" base %lld %llu", (long long)need, (unsigned long long)wsum(text.data(), text.size()));
        }
        printf("\n");
    }
    // what is no record of this program is refused, and nothing of the line is added
    static const char *const bad[] = { "x", "r\t0", "r\t0\tlambdaA\t1\t9\t", "r\t0\tlambdaA\t1\t9\t4M\t*\t0\t0\tACG\tIII", "r\t0\tlambdaA\t1\t9\tM\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t9\t4\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t0\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t9\t2I3S\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\t*\t1\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t70000\tlambdaA\t1\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t300\t4M\t*\t0\t0\tACGT\tIIII",
                                       "r\t0\tlambdaA\t1\t9\t999999999M\t*\t0\t0\tACGT\tIIII", "r\t0\tlambdaA\t1\t9\t2M1D3M\t*\t0\t0\tACGT\tIIII" };
    std::vector<uint32_t> none((size_t)n_words, 0);
    for (const char *b : bad) {
        const std::vector<char> line(b, b + strlen(b));
        if (salt_depth_add_sam(ix, line.data(), line.size(), 0, none.data(), n_words) >= 0) { fprintf(stderr, "accepted: %s\n", b); return 1; }
        if (strncmp(salt_host_last_error(), "depth: ", 7) != 0) { fprintf(stderr, "no message for: %s\n", b); return 1; }
    }
    if (salt_depth_add_sam(ix, nullptr, 0, 0, none.data(), n_words) != 0) { fprintf(stderr, "an empty text is no error\n"); return 1; }
    if (salt_depth_add_sam(ix, "x", 1, 0, none.data(), n_words - 1) >= 0) { fprintf(stderr, "an array of another size was accepted\n"); return 1; }
    if (salt_depth_text(ix, none.data(), n_words + 1, 0, nullptr, 0) >= 0) { fprintf(stderr, "a text of an array of another size was made\n"); return 1; }
    for (uint32_t c : none) if (c) { fprintf(stderr, "a refused line was added\n"); return 1; }
    // a record whose M run ends beyond the genome: cut at ref_len, the last word of the array takes the -1
    {
        char line[512];
        const int n = snprintf(line, sizeof line, "r\t0\tlambdaB_div2pct\t48463\t30\t100M\t*\t0\t0\t%0100d\t%0100d", 0, 0);
        const std::vector<char> l(line, line + n);
        if (n_words == 97005 && (salt_depth_add_sam(ix, l.data(), l.size(), 0, none.data(), n_words) != 1 || none[96964] != 1u || none[97004] != 0xFFFFFFFFu)) {
            fprintf(stderr, "a run over the genome's end was not cut there\n"); return 1;
        }
    }
    printf("refused %zu\n", sizeof bad / sizeof bad[0]);
    salt_index_free(ix);
    return 0;
}
