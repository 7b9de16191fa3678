// tools/snp_file_read.cc -- times salt-idx's reader of the four-column SNP file (read_snp_groups, salt_amd/host/salt_idx.cc) by itself: the
// baseline of the `salt-idx --vcf` measurement (profiles/r25/vcf.md).  The reader is internal to salt_idx.cc, so that file is compiled in.
//   g++ -O2 -std=c++17 -o tools/snp_file_read tools/snp_file_read.cc -lz -lpthread ;  tools/snp_file_read snps.txt [runs]
#include "../salt_amd/host/salt_idx.cc"

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: snp_file_read snps.txt [runs]\n"); return 1; }
    const int runs = argc > 2 ? atoi(argv[2]) : 1;
    for (int r = 0; r < runs; ++r) {
        std::vector<Group> groups;
        const double t0 = now_s();
        if (!read_snp_groups(argv[1], groups)) { fprintf(stderr, "%s\n", g_ierr.c_str()); return 1; }
        uint64_t n = 0;
        for (const Group &g : groups) n += g.pos.size();
        printf("{\"what\": \"read_snp_groups\", \"run\": %d, \"seconds\": %.3f, \"groups\": %zu, \"lines\": %llu}\n", r, now_s() - t0, groups.size(), (unsigned long long)n);
    }
    return 0;
}
