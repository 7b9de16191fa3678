// salt_amd/host/salt_idx_main.cc -- `salt-idx [-k seedlen] [--gpu [device]] [--no-lp] <ref.fa> <snps.txt> <out.prefix>`
// (Index_src/index1.c:46-185: index_main / index_usage; default seed length 25).
// --gpu sorts the suffixes on an MI355X through libsalt_gpu.so (loaded here, so that the tool still runs on a machine without
// ROCm); without it the host suffix sorter is used.  The files are the same either way.
// --vcf: the second positional is a VCF (plain, BGZF or gzip) whose single-base records become the SNP sites, matched to the contigs by
// NAME; --vcf-contigs FILE renames CHROM first, --vcf-pass-only drops records whose FILTER is neither PASS nor '.',
// --snp-out FILE also writes the sites as a four-column SNP file.  With --gpu the VCF is parsed on the device (25 times the host
// parser's rate on a dbSNP-shaped file, profiles/r25/vcf.md; SALT_VCF_DEVICE=0 keeps the host parser); the files are the same either way.
#include "../../include/salt_host.h"
#include <dlfcn.h>
#include <getopt.h>
#include <unistd.h>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>

static int usage()
{
    fprintf(stderr, "Usage: salt-idx [-k seed_length(25)] [--gpu[=device]] [--no-lp] [--all-files] <ref.fa> <snp file> <index prefix>\n"
                    "       salt-idx ... --vcf [--vcf-contigs map.tsv] [--vcf-pass-only] [--snp-out snps.txt] <ref.fa> <sites.vcf[.gz]> <index prefix>\n");
    return 1;
}

int main(int argc, char **argv)
{
    int k = 25, c, gpu = -1, flags = 0;
    bool vcf = false;
    salt_vcf_opt_t vo = {};
    static const struct option lo[] = { { "gpu", 2, 0, 1000 }, { "no-lp", 0, 0, 1001 }, { "all-files", 0, 0, 1002 }, { "vcf", 0, 0, 1003 }, { "vcf-contigs", 1, 0, 1004 },
                                        { "vcf-pass-only", 0, 0, 1005 }, { "snp-out", 1, 0, 1006 }, { "help", 0, 0, 'h' }, { 0, 0, 0, 0 } };
    while ((c = getopt_long(argc, argv, "k:h", lo, nullptr)) >= 0) {
        if (c == 'k') k = atoi(optarg);
        else if (c == 1000) gpu = optarg ? atoi(optarg) : 0;
        else if (c == 1001) flags |= SALT_IDX_NO_LP;
        else if (c == 1002) flags |= SALT_IDX_ALL_FILES;          // the files the reference indexer writes and `salt` never reads, too
        else if (c == 1003) vcf = true;
        else if (c == 1004) vo.rename_file = optarg;
        else if (c == 1005) vo.pass_only = 1;
        else if (c == 1006) vo.snp_out = optarg;
        else return usage();
    }
    if (argc - optind != 3) return usage();
    if (!vcf && (vo.rename_file || vo.pass_only || vo.snp_out)) { fprintf(stderr, "[salt-idx] --vcf-contigs, --vcf-pass-only and --snp-out go with --vcf\n"); return 1; }
    salt_idx_backend_t be, *bep = nullptr;
    salt_vcf_device_t vd;
    if (gpu >= 0) {
        char exe[PATH_MAX]; ssize_t n = readlink("/proc/self/exe", exe, sizeof exe - 1);
        std::string dir = n > 0 ? std::string(exe, (size_t)n) : std::string(argv[0]);
        dir = dir.substr(0, dir.find_last_of('/'));
        const std::string lib = dir + "/../lib/libsalt_gpu.so";
        void *h = dlopen(lib.c_str(), RTLD_NOW | RTLD_GLOBAL);
        if (!h) { fprintf(stderr, "[salt-idx] --gpu: %s\n", dlerror()); return 1; }
        be.device = gpu;
        be.build_c = reinterpret_cast<decltype(be.build_c)>(dlsym(h, "salt_gpu_idx_build_c"));
        be.build_r = reinterpret_cast<decltype(be.build_r)>(dlsym(h, "salt_gpu_idx_build_r"));
        be.last_error = reinterpret_cast<decltype(be.last_error)>(dlsym(h, "salt_gpu_idx_last_error"));
        if (!be.build_c || !be.build_r || !be.last_error) { fprintf(stderr, "[salt-idx] --gpu: %s lacks the index-construction entry points\n", lib.c_str()); return 1; }
        bep = &be;
        // the device ingest is looked up on its own: a library without it still sorts suffixes, and is refused only for --gpu --vcf on the device
        const char *dv = getenv("SALT_VCF_DEVICE");
        if (vcf && (!dv || atoi(dv))) {
            vd.device = gpu;
            vd.open = reinterpret_cast<decltype(vd.open)>(dlsym(h, "salt_gpu_vcf_open"));
            vd.add = reinterpret_cast<decltype(vd.add)>(dlsym(h, "salt_gpu_vcf_add"));
            vd.finish = reinterpret_cast<decltype(vd.finish)>(dlsym(h, "salt_gpu_vcf_finish"));
            vd.fetch = reinterpret_cast<decltype(vd.fetch)>(dlsym(h, "salt_gpu_vcf_fetch"));
            vd.close = reinterpret_cast<decltype(vd.close)>(dlsym(h, "salt_gpu_vcf_close"));
            vd.last_error = reinterpret_cast<decltype(vd.last_error)>(dlsym(h, "salt_gpu_last_error"));
            if (!vd.open || !vd.add || !vd.finish || !vd.fetch || !vd.close || !vd.last_error) { fprintf(stderr, "[salt-idx] --gpu --vcf: %s lacks the VCF entry points\n", lib.c_str()); return 1; }
            vo.device = &vd;
        }
    }
    if (vcf) {
        salt_vcf_counters_t ct = {};
        char unknown[256] = "";
        vo.counters = &ct; vo.unknown_name = unknown; vo.unknown_name_cap = sizeof unknown;
        const int rc = salt_idx_build_vcf(argv[optind], argv[optind + 1], argv[optind + 2], k, bep, flags, &vo);
        if (ct.lines || rc == 0)
            fprintf(stderr, "[salt-idx] vcf (%s): lines=%llu kept=%llu sites=%llu unknown_contig=%llu out_of_range=%llu not_snv=%llu ref_mismatch=%llu filtered=%llu\n",
                    vo.device ? "device" : "host", (unsigned long long)ct.lines, (unsigned long long)ct.kept, (unsigned long long)ct.sites, (unsigned long long)ct.unknown_contig,
                    (unsigned long long)ct.out_of_range, (unsigned long long)ct.not_snv, (unsigned long long)ct.ref_mismatch, (unsigned long long)ct.filtered);
        if (ct.unknown_contig) fprintf(stderr, "[salt-idx] vcf: first unknown contig \"%s\" at line %llu (see --vcf-contigs)\n", unknown, (unsigned long long)ct.first_unknown_line);
        if (rc != 0) { fprintf(stderr, "[salt-idx] %s\n", salt_idx_last_error()); return 1; }
        return 0;
    }
    if (salt_idx_build_ex(argv[optind], argv[optind + 1], argv[optind + 2], k, bep, flags) != 0) {
        fprintf(stderr, "[salt-idx] %s\n", salt_idx_last_error());
        return 1;
    }
    return 0;
}
