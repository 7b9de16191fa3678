// tools/trim_pair_model.cc -- the pair form of the trimming rule (trim_pair_span of salt_amd/csrc/salt_trim_rule.h, the header k_fq_trim_pair
// and salt_trim_pair_span compile) run on the host over cases read from a file:  trim_pair_model cases.tsv > spans.txt.  It is where the
// pair rule's bounds are proven: tests/test_trim_pair_model.py builds it with AddressSanitizer and UBSan and compares its spans with the
// Python statement of the rule (tests/trim_pair_check.py); salt never runs it.
//   g++ -O2 -std=c++17 -o trim_pair_model tools/trim_pair_model.cc
// A case is one line of thirteen TAB-separated fields:
//   adapter  adapter2  qual  front  tail  min_overlap  error_pct  pair_min_overlap  pair_error_pct  seq1  quality1  seq2  quality2
// ('-' for no adapter; both pair fields 0: the pair rule off; sequences and qualities as hexadecimal bytes, so that any byte can stand in
// them).  Output: "b1 e1 b2 e2" per case, then the sixteen counters on one line and the eight pair counters on the next.  Exit 2 with the
// reason on stderr for a line that is no case or options the rule refuses.
#include "../salt_amd/csrc/salt_trim_rule.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

// the bytes of a hexadecimal field in an allocation of exactly their number: a read past either end is the sanitizer's to see
static bool unhex(const std::string &h, std::unique_ptr<uint8_t[]> &out, size_t &n)
{
    if (h.size() % 2) return false;
    n = h.size() / 2;
    out.reset(new uint8_t[n]);
    for (size_t i = 0; i < n; ++i) {
        unsigned v = 0;
        for (size_t k = 2 * i; k < 2 * i + 2; ++k) {
            const char c = h[k];
            const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
            if (d < 0) return false;
            v = v * 16 + (unsigned)d;
        }
        out[i] = (uint8_t)v;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: trim_pair_model cases.tsv\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string text;
    { char buf[1 << 16]; size_t r; while ((r = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, r); }
    fclose(f);
    uint64_t counts[2 * salt::TRIM_N_COUNTS] = {}, pair_counts[salt::TRIM_PAIR_N_COUNTS] = {};
    size_t line_no = 0;
    for (size_t at = 0; at < text.size(); ++line_no) {
        size_t e = text.find('\n', at);
        if (e == std::string::npos) e = text.size();
        std::vector<std::string> fld;
        for (size_t p = at; p <= e;) {
            size_t t = text.find('\t', p);
            if (t == std::string::npos || t > e) t = e;
            fld.emplace_back(text, p, t - p);
            p = t + 1;
        }
        at = e + 1;
        if (fld.size() != 13) { fprintf(stderr, "line %zu: %zu fields, a case has 13\n", line_no, fld.size()); return 2; }
        const bool has1 = fld[0] != "-", has2 = fld[1] != "-";
        uint32_t num[7];
        for (int k = 0; k < 7; ++k) num[k] = (uint32_t)strtoul(fld[2 + k].c_str(), nullptr, 10);
        salt::TrimRule rule; salt::TrimPairRule pair;
        const char *what = salt::trim_rule_make(has1 ? fld[0].data() : nullptr, (uint32_t)fld[0].size(), has2 ? fld[1].data() : nullptr, (uint32_t)fld[1].size(),
                                                num[1], num[2], num[0], num[3], num[4], &rule);
        if (!what) what = salt::trim_pair_rule_make(num[5], num[6], &pair);
        if (what) { fprintf(stderr, "line %zu: %s\n", line_no, what); return 2; }
        std::unique_ptr<uint8_t[]> seq[2], qual[2];
        size_t n_seq[2] = { 0, 0 }, n_qual[2] = { 0, 0 };
        bool ok = true;
        for (int m = 0; m < 2; ++m) ok = ok && unhex(fld[9 + 2 * m], seq[m], n_seq[m]) && unhex(fld[10 + 2 * m], qual[m], n_qual[m]) && n_seq[m] && n_seq[m] == n_qual[m];
        if (!ok) { fprintf(stderr, "line %zu: a sequence or quality is not what a case holds\n", line_no); return 2; }
        uint32_t span[4] = { 0, 0, 0, 0 };
        salt::trim_pair_span(rule, pair, seq[0].get(), qual[0].get(), (uint32_t)n_seq[0], seq[1].get(), qual[1].get(), (uint32_t)n_seq[1], span, counts, pair_counts);
        printf("%u %u %u %u\n", span[0], span[1], span[2], span[3]);
    }
    for (unsigned k = 0; k < 2 * salt::TRIM_N_COUNTS; ++k) printf("%llu%c", (unsigned long long)counts[k], k + 1 < 2 * salt::TRIM_N_COUNTS ? ' ' : '\n');
    for (unsigned k = 0; k < salt::TRIM_PAIR_N_COUNTS; ++k) printf("%llu%c", (unsigned long long)pair_counts[k], k + 1 < salt::TRIM_PAIR_N_COUNTS ? ' ' : '\n');
    return 0;
}
