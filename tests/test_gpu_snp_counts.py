"""Allele counts at the SNP sites on the device: the site table (k_snp_bits, the scan, k_snp_rank, k_snp_pos) against salt_snp_sites, and
k_snp_count behind every entry point that leaves result rows against the host twin (salt_snp_count_sam) over the SAM text the same call
returned -- single and paired end, text, host-buffer and resident entry points, soft clips, indels, reads over the contig boundary --,
then the state (two calls, a fork, reset, off) and the `salt` binary with --snp-counts, plain and under --polish."""
import os
import subprocess

import numpy as np
import pytest

import gap_cases
import snp_check
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT

pytestmark = pytest.mark.gpu

SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")

# name -> (salt arguments, FASTQ files under tests/golden/lambda, plain or .gz)
SE_SETS = {
    "se_default": (["-d", "-c"], ["reads_se.fq"]), "ragged_default": EXTRA_CASES["ragged_default"], "span_default": EXTRA_CASES["span_default"],
    "gap_se_mid": (gap_cases.GAP_CASES["gap_se_mid"][0], ["reads_gap_se_mid.fq.gz"]),
}
PE_SETS = {
    "pe_default": (["-d", "-p", "-c", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"]), "ragged_pe": EXTRA_CASES["ragged_pe"],
    "gap_pe_short": (gap_cases.GAP_CASES["gap_pe_short"][0], ["reads_gap_pe_short_1.fq.gz", "reads_gap_pe_short_2.fq.gz"]),
}


def _fq(name):
    import gzip
    data = open(os.path.join(LAMBDA, name), "rb").read()
    return gzip.decompress(data) if name.endswith(".gz") else data


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=8192)
    aln.set_contigs(ix)
    yield salt_amd, ix, aln
    aln.close()
    ix.destroy()


def _opt(salt_amd, ix, args):
    return salt_amd.AlnOpt.from_argv(list(args), ix.l_seed)[0]


def test_before_the_first_enable_there_is_no_table(lam):
    salt_amd, ix, _ = lam
    other = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    try:
        for call in (other.snp_sites, other.snp_counts):
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
        with pytest.raises(salt_amd.SaltError, match="255"):
            other.snp_enable(True, 256)
        other.snp_enable(False)                                      # stopping what never ran is no error, and builds nothing
        with pytest.raises(salt_amd.SaltError, match="never enabled"):
            other.snp_sites()
    finally:
        other.close()


def test_device_sites_equal_the_host_twins_on_lambda(lam):
    salt_amd, ix, aln = lam
    aln.snp_enable(True)
    got, want = aln.snp_sites(), salt_amd.snp_sites(ix)
    aln.snp_enable(False)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert len(want) == 3858 and want[-1] == 97003 and 97004 % 64 == 44          # the last window is partial, and its last position is a site
    # cap too small: an error that says so, not a short list
    import ctypes
    n, few = ctypes.c_uint32(), np.zeros(10, dtype=np.uint32)
    lib = salt_amd.gpu_lib()
    assert not aln.snp_counts().any()
    assert lib.salt_gpu_index_snp_sites(aln._ix, ctypes.byref(n), few.ctypes.data, 10) == -1 and b"10 positions" in lib.salt_gpu_last_error()
    assert lib.salt_gpu_index_snp_counts(aln._ix, few.ctypes.data, 10, 0) == -1 and b"10 words" in lib.salt_gpu_last_error()
    assert not few.any()


def test_device_sites_at_the_window_edges(tmp_path):
    """SNPs at 0, 63, 64, 127, ref_len - 1 and at all 64 positions of one window, among 400 others, in a genome of 64 * 800 + 13 bases: where
    the rank of a window, the mask of a lookup and the partial last window can go wrong."""
    import salt_amd
    from salt_amd import workload
    n = 64 * 800 + 13
    g = workload.make_genome(n, seed=3)
    rnd, _ = workload.make_snps(g, 400, seed=9)
    pos = np.array(sorted({0, 63, 64, 127, n - 1} | set(range(64 * 300, 64 * 301)) | set(int(p) for p in rnd)), dtype=np.int64)
    ref = g[pos]
    mask = ((1 << ref) | (1 << ((ref + 1) & 3))).astype(np.uint8)
    tri = (pos % 7) == 0
    mask[tri] |= (1 << ((ref[tri] + 2) & 3)).astype(np.uint8)
    contigs, groups = workload.as_builder_input(g, pos, mask)
    prefix = str(tmp_path / "edge")
    salt_amd.idx_build_mem(contigs, groups, prefix, 19, flags=salt_amd.IDX_NO_LP)
    ix = salt_amd.Index.reload(prefix)
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    try:
        aln.snp_enable(True)
        got, want = aln.snp_sites(), salt_amd.snp_sites(ix)
        counts = aln.snp_counts()
    finally:
        aln.close()
        ix.destroy()
    assert np.array_equal(want, pos.astype(np.uint32))
    assert np.array_equal(got, want)
    assert counts.shape == (len(pos), 4) and not counts.any()


def _check(name, got, want, sam, min_mapq):
    assert got.shape == want.shape and got.dtype == np.uint32
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError("%s, min_mapq %d: %d sites differ; first %s: device %s, twin %s" % (name, min_mapq, len(bad), bad[:3], got[bad[:3]], want[bad[:3]]))
    assert want.sum() > 0


@pytest.fixture(scope="module")
def se_counts(lam):
    """name -> (SAM of the text call, device counts at min_mapq 0 and 20 of that call): computed once, shared."""
    salt_amd, ix, aln = lam
    out = {}
    for name, (args, files) in SE_SETS.items():
        opt, fq = _opt(salt_amd, ix, args), _fq(files[0])
        per_q = {}
        for q in (0, 20):
            aln.snp_enable(True, q)
            aln.snp_counts(reset=True)
            sam, n = aln.align_se_text(opt, fq)
            per_q[q] = aln.snp_counts()
            aln.snp_enable(False)
            assert sam == per_q.setdefault("sam", sam) and n > 0
        out[name] = per_q
    return out


@pytest.fixture(scope="module")
def pe_counts(lam):
    salt_amd, ix, aln = lam
    out = {}
    for name, (args, files) in PE_SETS.items():
        opt, fq1, fq2 = _opt(salt_amd, ix, args), _fq(files[0]), _fq(files[1])
        per_q = {}
        for q in (0, 20):
            aln.snp_enable(True, q)
            aln.snp_counts(reset=True)
            sam, n = aln.align_pe_text(opt, ix, fq1, fq2)
            per_q[q] = aln.snp_counts()
            aln.snp_enable(False)
            assert sam == per_q.setdefault("sam", sam) and n > 0
        out[name] = per_q
    return out


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("name", sorted(SE_SETS))
def test_single_end_text_counts_equal_the_twin_over_the_calls_own_sam(name, min_mapq, lam, se_counts):
    salt_amd, ix, _ = lam
    sam = se_counts[name]["sam"]
    _check(name, se_counts[name][min_mapq], salt_amd.snp_count_sam(ix, sam, min_mapq), sam, min_mapq)


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("name", sorted(PE_SETS))
def test_paired_end_text_counts_equal_the_twin_over_the_calls_own_sam(name, min_mapq, lam, pe_counts):
    salt_amd, ix, _ = lam
    sam = pe_counts[name]["sam"]
    _check(name, pe_counts[name][min_mapq], salt_amd.snp_count_sam(ix, sam, min_mapq), sam, min_mapq)


def test_the_calls_cover_indels_clips_a_deep_site_and_the_contig_boundary(lam, se_counts, pe_counts):
    """None of the comparisons above passes on empty ground."""
    salt_amd, ix, _ = lam
    assert snp_check.census(se_counts["gap_se_mid"]["sam"])[0] >= 1000
    assert snp_check.census(pe_counts["gap_pe_short"]["sam"])[0] >= 300
    assert snp_check.census(pe_counts["pe_default"]["sam"])[1] >= 40 and snp_check.census(pe_counts["ragged_pe"]["sam"])[1] >= 40
    assert int(se_counts["span_default"][0].sum(axis=1).max()) >= 30
    assert int(se_counts["se_default"][0].sum()) == 7574 and int(se_counts["se_default"][20].sum()) == 3508
    # the Python statement of the rule agrees with both, on the file with the most shapes
    sites, _ = snp_check.sites_of_ref(os.path.join(LAMBDA, "idx.ref"))
    want, _ = snp_check.count_sam(sites, snp_check.contig_offsets(os.path.join(LAMBDA, "idx.C.ann")), pe_counts["gap_pe_short"]["sam"], 20)
    assert np.array_equal(pe_counts["gap_pe_short"][20], want)


@pytest.mark.parametrize("name", sorted(SE_SETS))
def test_alnse_core1_counts_what_the_text_call_counts(name, lam, se_counts):
    salt_amd, ix, aln = lam
    args, files = SE_SETS[name]
    names, seqs, offs, quals = salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
    aln.snp_enable(True, 20)
    aln.snp_counts(reset=True)
    aln.alnse_core1(_opt(salt_amd, ix, args), seqs, offs)
    got = aln.snp_counts()
    aln.snp_enable(False)
    _check(name, got, se_counts[name][20], None, 20)


@pytest.mark.parametrize("name", sorted(PE_SETS))
def test_alnpe_core1_counts_what_the_text_call_counts(name, lam, pe_counts):
    salt_amd, ix, aln = lam
    args, files = PE_SETS[name]
    names, seqs, offs, quals = salt_amd.interleave_pairs(salt_amd.read_fastq(os.path.join(LAMBDA, files[0])), salt_amd.read_fastq(os.path.join(LAMBDA, files[1])))
    aln.snp_enable(True, 0)
    aln.snp_counts(reset=True)
    aln.alnpe_core1(_opt(salt_amd, ix, args), ix, seqs, offs)
    got = aln.snp_counts()
    aln.snp_enable(False)
    _check(name, got, pe_counts[name][0], None, 0)


def test_resident_entry_points_count_on_the_callers_stream(lam, se_counts, pe_counts):
    import torch
    salt_amd, ix, aln = lam
    isz = salt_amd.RESULT_DTYPE.itemsize
    st = torch.cuda.Stream()
    for name, sets, want in (("ragged_default", SE_SETS, se_counts), ("ragged_pe", PE_SETS, pe_counts)):
        args, files = sets[name]
        if len(files) == 1:
            _, seqs, offs, _ = salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
        else:
            _, seqs, offs, _ = salt_amd.interleave_pairs(salt_amd.read_fastq(os.path.join(LAMBDA, files[0])), salt_amd.read_fastq(os.path.join(LAMBDA, files[1])))
        n, max_len = len(offs) - 1, int(np.diff(offs).max())
        d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(64, dtype=np.uint8)])).cuda()
        d_offs = torch.from_numpy(np.asarray(offs).astype(np.int32)).cuda()
        d_res = torch.zeros(n * isz, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        opt = _opt(salt_amd, ix, args)
        aln.snp_enable(True, 0)
        aln.snp_counts(reset=True)
        with torch.cuda.stream(st):
            if len(files) == 1:
                aln.align_resident(opt, n, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
            else:
                aln.align_pe_resident(opt, ix, n // 2, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
        got = aln.snp_counts()                                       # (synchronises the device)
        aln.snp_enable(False)
        _check(name, got, want[name][0], None, 0)


def test_two_calls_accumulate_a_fork_adds_to_the_same_table_reset_zeroes_and_off_counts_nothing(lam, se_counts, pe_counts):
    salt_amd, ix, aln = lam
    opt_se, opt_pe = _opt(salt_amd, ix, SE_SETS["se_default"][0]), _opt(salt_amd, ix, PE_SETS["ragged_pe"][0])
    fq, fq1, fq2 = _fq("reads_se.fq"), _fq("reads_ragged_pe_1.fq"), _fq("reads_ragged_pe_2.fq")
    one, two = se_counts["se_default"][0], pe_counts["ragged_pe"][0]
    aln.snp_enable(True, 0)
    aln.snp_counts(reset=True)
    sam_on, _ = aln.align_se_text(opt_se, fq)
    aln.align_se_text(opt_se, fq)
    assert np.array_equal(aln.snp_counts(), 2 * one)
    fork = aln.fork()
    try:
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert np.array_equal(fork.snp_counts(), 2 * one + two)
        assert np.array_equal(aln.snp_counts(reset=True), 2 * one + two)
        assert not aln.snp_counts().any() and not fork.snp_counts().any()
        aln.snp_enable(False)
        sam_off, _ = aln.align_se_text(opt_se, fq)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert not aln.snp_counts().any()
        assert sam_on == sam_off == se_counts["se_default"]["sam"]   # the SAM bytes do not depend on the counting
        # a block that is aligned and then dropped leaves the table as it was
        aln.snp_enable(True, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        aln.align_se_text(opt_se, fq)
        lib = salt_amd.gpu_lib()
        assert lib.salt_gpu_ws_snp_uncount(fork._ws) == 0 and np.array_equal(aln.snp_counts(), one)
        assert lib.salt_gpu_ws_snp_uncount(fork._ws) == 0 and np.array_equal(aln.snp_counts(), one)      # only once
        assert lib.salt_gpu_ws_snp_uncount(aln._ws) == 0 and not aln.snp_counts().any()
    finally:
        aln.snp_enable(False)
        fork.close()


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("snpidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


def test_cli_file_equals_the_twin_over_its_stdout_plain_and_under_polish(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    reads = os.path.join(LAMBDA, "reads_se.fq")
    f, fp = tmp_path / "counts.tsv", tmp_path / "counts_polish.tsv"
    run = subprocess.run([SALT, "-d", "-c", "--snp-counts", str(f), "--snp-min-mapq", "20", lambda_cli_index, reads], capture_output=True, timeout=300)
    assert run.returncode == 0 and b"text path" in run.stderr and b"counted on the device" in run.stderr, run.stderr[-600:]
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    rows, counts = snp_check.parse_counts_file(f.read_bytes())
    want = salt_amd.snp_count_sam(ix, run.stdout, 20)
    assert len(rows) == 3858 and np.array_equal(counts, want.astype(np.uint64)) and int(want.sum()) == 3508
    pol = subprocess.run([SALT, "-d", "-c", "--polish", "--snp-counts", str(fp), "--snp-min-mapq", "20", lambda_cli_index, reads], capture_output=True, timeout=300)
    assert pol.returncode == 0 and b"counted on the device" in pol.stderr, pol.stderr[-600:]
    assert fp.read_bytes() == f.read_bytes()
    alone = subprocess.run([SALT, "-d", "-c", "--polish", lambda_cli_index, reads], capture_output=True, timeout=300)
    assert alone.returncode == 0 and pol.stdout == alone.stdout and len(alone.stdout) > 100000


def test_cli_counts_every_written_block_once_across_the_hand_over(lam, lambda_cli_index, tmp_path):
    """A multi-line record in the middle of the file, chunks of 9 000 bytes: the blocks the workers had aligned behind the refused chunk
    are dropped and their adds taken back (salt_gpu_ws_snp_uncount); the host pipeline aligns those reads again."""
    salt_amd, ix, _ = lam
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq, f = tmp_path / "mid_multiline.fq", tmp_path / "counts.tsv"
    fq.write_bytes(b"\n".join(out) + b"\n")
    run = subprocess.run([SALT, "-d", "-c", "-t", "8", "--snp-counts", str(f), lambda_cli_index, str(fq)], capture_output=True, timeout=300,
                         env=dict(os.environ, SALT_CHUNK_BYTES="9000"))
    assert run.returncode == 0, run.stderr[-600:]
    assert b"the host parser takes over" in run.stderr and b"counted on the device" in run.stderr
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    _, counts = snp_check.parse_counts_file(f.read_bytes())
    want = salt_amd.snp_count_sam(ix, run.stdout, 0)
    assert np.array_equal(counts, want.astype(np.uint64)) and int(want.sum()) == 7574
