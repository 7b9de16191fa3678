// tools/vcf_model.cc -- the host twin of the device's VCF parser (salt_vcf_snps, salt_amd/host/salt_idx.cc, which compiles the kernel's own
// per-line function salt_amd/csrc/salt_vcf_line.h) as a program:  vcf_model [--pass-only] genome.fa sites.vcf  prints one line
// "contig <TAB> 0-based position <TAB> allele mask <TAB> reference code" per site and a last line with the counters; exit 3 and the message on
// stderr when the text is refused.  The genome and the text sit in allocations of exactly their sizes, so tests/test_vcf_host.py, which
// builds this with AddressSanitizer + UBSan, proves the line function's bounds rules on the CPU, where a stray read is reported.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -o vcf_model tools/vcf_model.cc salt_amd/host/salt_idx.cc -lz -lpthread
#include "../include/salt_host.h"
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static bool slurp(const char *fn, std::string &out)
{
    FILE *f = fopen(fn, "rb");
    if (!f) return false;
    char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    salt_vcf_opt_t opt = {};
    int a = 1;
    if (a < argc && !strcmp(argv[a], "--pass-only")) { opt.pass_only = 1; ++a; }
    if (argc - a != 2) { fprintf(stderr, "usage: vcf_model [--pass-only] genome.fa sites.vcf\n"); return 1; }
    std::string fa, vcf;
    if (!slurp(argv[a], fa) || !slurp(argv[a + 1], vcf)) { fprintf(stderr, "cannot read the input\n"); return 1; }
    std::vector<std::string> names, seqs;
    for (size_t p = 0; p < fa.size();) {
        size_t e = fa.find('\n', p); if (e == std::string::npos) e = fa.size();
        if (fa[p] == '>') { size_t q = p + 1; while (q < e && fa[q] != ' ' && fa[q] != '\t') ++q; names.push_back(fa.substr(p + 1, q - p - 1)); seqs.emplace_back(); }
        else if (!seqs.empty()) seqs.back().append(fa, p, e - p);
        p = e + 1;
    }
    // exact-size copies: one byte past a contig or past the text is outside its allocation
    std::vector<std::unique_ptr<char[]>> own; std::vector<salt_idx_contig_t> contigs;
    for (size_t i = 0; i < names.size(); ++i) {
        own.emplace_back(new char[seqs[i].size() ? seqs[i].size() : 1]);
        memcpy(own.back().get(), seqs[i].data(), seqs[i].size());
        contigs.push_back(salt_idx_contig_t{ names[i].c_str(), nullptr, own.back().get(), seqs[i].size() });
    }
    std::unique_ptr<char[]> text(new char[vcf.size() ? vcf.size() : 1]);
    memcpy(text.get(), vcf.data(), vcf.size());
    salt_vcf_t *v = salt_vcf_snps(contigs.data(), (int)contigs.size(), text.get(), vcf.size(), &opt);
    if (!v) { fprintf(stderr, "%s\n", salt_idx_last_error()); return 3; }
    for (size_t i = 0; i < contigs.size(); ++i) {
        salt_idx_snps_t g;
        if (salt_vcf_group(v, (int)i, &g) != 0) return 1;
        for (uint32_t j = 0; j < g.n; ++j) printf("%s\t%u\t%u\t%u\n", g.chr, g.pos[j], g.alleles[j], g.ref[j]);
    }
    salt_vcf_counters_t c;
    salt_vcf_counters(v, &c);
    printf("lines=%llu kept=%llu sites=%llu unknown_contig=%llu out_of_range=%llu not_snv=%llu ref_mismatch=%llu filtered=%llu first_unknown_line=%llu\n",
           (unsigned long long)c.lines, (unsigned long long)c.kept, (unsigned long long)c.sites, (unsigned long long)c.unknown_contig, (unsigned long long)c.out_of_range,
           (unsigned long long)c.not_snv, (unsigned long long)c.ref_mismatch, (unsigned long long)c.filtered, (unsigned long long)c.first_unknown_line);
    salt_vcf_free(v);
    return 0;
}
