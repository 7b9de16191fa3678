// tools/trim_model.cc -- the trimming rule (salt_amd/csrc/salt_trim_rule.h, the header k_fq_trim and salt_trim_span compile) run on the host
// over cases read from a file:  trim_model cases.tsv > spans.txt.  It is where the rule's bounds are proven: tests/test_trim_model.py builds
// it with AddressSanitizer and UBSan and compares its spans with the Python statement of the rule (tests/trim_check.py); salt never runs it.
//   g++ -O2 -std=c++17 -o trim_model tools/trim_model.cc
// A case is one line of ten TAB-separated fields:  mate  adapter  adapter2  qual  front  tail  min_overlap  error_pct  seq  quality
// ('-' for no adapter; seq and quality as hexadecimal bytes, so that any byte can stand in either).  Output: "beg end" per case, then the
// sixteen counters on one line.  Exit 2 with the reason on stderr for a line that is no case or options the rule refuses.
#include "../salt_amd/csrc/salt_trim_rule.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static bool unhex(const std::string &h, std::vector<uint8_t> &out)
{
    if (h.size() % 2) return false;
    out.clear();
    for (size_t i = 0; i < h.size(); i += 2) {
        unsigned v = 0;
        for (size_t k = i; k < i + 2; ++k) {
            const char c = h[k];
            const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
            if (d < 0) return false;
            v = v * 16 + (unsigned)d;
        }
        out.push_back((uint8_t)v);
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: trim_model cases.tsv\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string text;
    { char buf[1 << 16]; size_t r; while ((r = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, r); }
    fclose(f);
    uint64_t counts[2 * salt::TRIM_N_COUNTS] = {};
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
        if (fld.size() != 10) { fprintf(stderr, "line %zu: %zu fields, a case has 10\n", line_no, fld.size()); return 2; }
        const unsigned long mate = strtoul(fld[0].c_str(), nullptr, 10);
        const bool has1 = fld[1] != "-", has2 = fld[2] != "-";
        uint32_t num[5];
        for (int k = 0; k < 5; ++k) num[k] = (uint32_t)strtoul(fld[3 + k].c_str(), nullptr, 10);
        salt::TrimRule rule;
        if (const char *what = salt::trim_rule_make(has1 ? fld[1].data() : nullptr, (uint32_t)fld[1].size(), has2 ? fld[2].data() : nullptr, (uint32_t)fld[2].size(),
                                                    num[1], num[2], num[0], num[3], num[4], &rule)) {
            fprintf(stderr, "line %zu: %s\n", line_no, what);
            return 2;
        }
        // the read and its qualities in allocations of exactly their sizes: a read past either end is the sanitizer's to see
        std::vector<uint8_t> seq, qual;
        if (mate > 1 || !unhex(fld[8], seq) || !unhex(fld[9], qual) || seq.empty() || seq.size() != qual.size()) {
            fprintf(stderr, "line %zu: mate, sequence or quality is not what a case holds\n", line_no);
            return 2;
        }
        uint32_t beg = 0, end = 0;
        salt::trim_span(rule, (uint32_t)mate, seq.data(), qual.data(), (uint32_t)seq.size(), &beg, &end, counts + salt::TRIM_N_COUNTS * mate);
        printf("%u %u\n", beg, end);
    }
    for (unsigned k = 0; k < 2 * salt::TRIM_N_COUNTS; ++k) printf("%llu%c", (unsigned long long)counts[k], k + 1 < 2 * salt::TRIM_N_COUNTS ? ' ' : '\n');
    return 0;
}
