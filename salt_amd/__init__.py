"""salt_amd -- MI355X-native implementation of salt's per-read alignment hot path.

Only what the path needs: csrc/ (HIP kernels + the C ABI of include/salt_gpu.h), host/ (index
files + SAM text, include/salt_host.h) and api.py (ctypes bindings that mirror the reference's
batch-level interface)."""
from .api import (AlnOpt, GpuAligner, Index, SaltError, RESULT_DTYPE, read_fastq, sam_text, sam_text_pe, interleave_pairs,  # noqa: F401
                  gpu_lib, host_lib, idx_build, idx_build_mem, vcf_snps, VCF_COUNTERS, suffix_array, IDX_NO_LP, bgzf_deflate, bgzf_inflate, BGZF_CUT, BGZF_EOF, bam_header, bam_from_sam,
                  BAM_MAX_NAME, Polisher, POLISH_STATS, snp_sites, snp_count_sam, depth_add_sam, depth_text, errprof_add_sam, errprof_text, ERRPROF_SHAPE, stats_add_sam, stats_text, stats_split, STATS_TABLES, STATS_CELLS, STATS_CT_LDS, STATS_CHUNK,
                  gt_add_sam, gt_text, gt_header, gt_table, GT_Q_NONE,
                  disc_add_sam, disc_text, DISC_ALT, DISC_DIFF, DISC_FIELD_BITS, DISC_DEFAULTS,
                  indel_add_sam, indel_text, indel_header, INDEL_DEFAULTS, INDEL_STATS, INDEL_PROBE, INDEL_MAX_INS, INDEL_MAX_DEL, INDEL_MAX_SHIFT,
                  trim_span, trim_fastq, TRIM_COUNTERS, trim_pair_span, trim_fastq_pair, TRIM_PAIR_COUNTERS,
                  diag_pack, pack_geom, PACK_FILL)
