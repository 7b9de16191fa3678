"""The context record's geometry (salt_amd/csrc/salt_ctx_record.h) on the GPU: whatever bases the record holds, the rows k_heavy drops
with it never change a result -- for reads of 100 and of 150 bases and seed lengths 21 and 19 (side A starts a number of seed lengths
behind the suffix) -- and on reads whose first seed is a repeat it drops more rows than the symmetric record did."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tandem_index(tmp_path, k):
    """The tandem-repeat genome of test_gpu_context_table_rules_rows_out_without_changing_a_result (every seed hits hundreds of diverged
    copies, one SNP per ~60 bases), indexed with seed length k."""
    from salt_amd import workload
    genome = workload.make_tandem(divergence=0.08)
    pos, mask = workload.make_snps(genome, 20000, seed=6)
    fa, snp, prefix = str(tmp_path / "g.fa"), str(tmp_path / "s.txt"), str(tmp_path / ("idx%d" % k))
    workload.write_fasta(fa, "tandem", genome)
    workload.write_snps(snp, "tandem", genome, pos, mask)
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", str(k), fa, snp, prefix], check=True, stderr=subprocess.DEVNULL)
    return genome, pos, mask, prefix


def run_both(idx, opt, seqs, offs):
    """(result rows, counters) with the context table ("0") and without it ("1")."""
    import salt_amd
    n = len(offs) - 1
    got = {}
    for no_ctx in ("0", "1"):
        os.environ["SALT_GPU_NO_CTX"] = no_ctx
        try:
            aln = salt_amd.GpuAligner(idx, device=0, max_reads=n, max_bases=int(offs[-1]) + 64)
            aln.counters()
            got[no_ctx] = (aln.alnse_core1(opt, seqs, offs).copy(), aln.counters())
            aln.close()
        finally:
            del os.environ["SALT_GPU_NO_CTX"]
    return got


def repeat_reads(genome, pos, mask, n, L, seed):
    """Reads that start inside the block of repeat copies (make_tandem: 30 000-base flanks around 40 000 x 30 bases): the seed of slot 0
    is a repeat seed at read offset 0, which the seed extension cannot shrink."""
    from salt_amd import workload
    flank, block = 30000, 40000 * 30
    seqs, offs, _, _ = workload.make_reads(genome[flank:flank + block], pos[(pos >= flank) & (pos < flank + block)] - flank,
                                           mask[(pos >= flank) & (pos < flank + block)], n, L, seed=seed)
    return seqs, offs


@pytest.mark.parametrize("k", [21, 19])
def test_gpu_context_geometry_changes_no_result_for_either_read_length_or_seed_length(tmp_path, k):
    """Reads of 100 and of 150 bases over the tandem genome, with N in some and four at the genome's ends, index built with -k 21 and
    -k 19: rows with the table == rows without it, byte for byte == the oracle's, and the table did rule rows out."""
    import salt_amd
    from salt_amd import workload
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    genome, pos, mask, prefix = tandem_index(tmp_path, k)
    idx = salt_amd.Index.reload(prefix)
    assert idx.l_seed == k
    opt, _ = salt_amd.AlnOpt.from_argv([], idx.l_seed)
    opt.collect_counters = 1
    ora = oracle_py.Oracle(prefix)
    try:
        for L in (100, 150):
            n0 = 1500
            seqs, offs, _, _ = workload.make_reads(genome, pos, mask, n0, L, seed=21 + L)
            seqs = seqs.copy()
            rng = np.random.default_rng(4)
            for r in rng.choice(n0, n0 // 10, replace=False):
                seqs[int(offs[r]) + rng.integers(0, L, 3)] = 4
            ends = np.concatenate([genome[:L], genome[-L:], genome[1:L + 1], genome[-L - 1:-1]]).astype(np.uint8)
            seqs = np.concatenate([seqs, ends]); offs = np.concatenate([offs, offs[-1] + L * np.arange(1, 5, dtype=np.uint32)]).astype(np.uint32)
            got = run_both(idx, opt, seqs, offs)
            print("k %d L %d: %s" % (k, L, {c: got["0"][1][c] for c in ("d_ctx_rows", "d_ctx_rejected", "d_verify_heavy")}))
            assert got["0"][1]["d_ctx_rejected"] > 0 and got["0"][1]["d_ctx_rows"] > got["0"][1]["d_ctx_rejected"], got["0"][1]
            assert got["1"][1]["d_ctx_rows"] == 0
            assert got["0"][0].tobytes() == got["1"][0].tobytes()
            want = ora.align(ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref), seqs, offs, n_threads=8)
            bad = oracle_py.compare(got["0"][0], want)
            assert len(bad) == 0, (L, bad[:5])
    finally:
        ora.close()
        idx.destroy()


# d_ctx_rejected / d_ctx_rows of the test below with the symmetric record (23 in front, 23 behind the seed), measured once on the commit
# before the geometry changed: 327 205 of 612 490 rows (100 bases), 388 926 of 711 570 (150 bases)
PARENT_SHARE_100 = 0.5342
PARENT_SHARE_150 = 0.5466


def test_gpu_context_geometry_rejects_more_rows_of_reads_that_start_in_a_repeat(tmp_path):
    """3 000 reads of 100 and of 150 bases that start inside a repeat copy (slot 0 holds a wide interval at read offset 0, where the
    bases in front of the suffix face nothing): d_ctx_rejected / d_ctx_rows is above what the symmetric record (23 in front, 23
    behind the seed) of the parent commit gave on the same input, and the rows equal the run without the table.
    Measured on one MI355X, the same rows in both: 100 bases 0.5342 -> 0.7492 with 9 bases in front and 37 behind from 2 k on
    (0.7348 with the 37 from 3 k on), 150 bases 0.5466 -> 0.7386 (0.7273); the test prints what the geometry of the header gives."""
    import salt_amd
    genome, pos, mask, prefix = tandem_index(tmp_path, 21)
    idx = salt_amd.Index.reload(prefix)
    opt, _ = salt_amd.AlnOpt.from_argv([], idx.l_seed)
    opt.collect_counters = 1
    try:
        for L, parent in ((100, PARENT_SHARE_100), (150, PARENT_SHARE_150)):
            seqs, offs = repeat_reads(genome, pos, mask, 3000, L, seed=5 + L)
            got = run_both(idx, opt, seqs, offs)
            c = got["0"][1]
            share = c["d_ctx_rejected"] / c["d_ctx_rows"]
            print("L %d: rejected %d of %d context rows = %.4f (parent %.4f), d_verify_heavy %d" % (L, c["d_ctx_rejected"], c["d_ctx_rows"], share, parent, c["d_verify_heavy"]))
            assert got["0"][0].tobytes() == got["1"][0].tobytes()
            assert share > parent, (L, share, parent)
    finally:
        idx.destroy()
