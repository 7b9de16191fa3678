"""Coverage on the device: k_depth_mark behind every entry point that leaves result rows against the host twin (salt_depth_add_sam) over the
SAM text the same call returned -- single and paired end, text, host-buffer and resident entry points --, the state of the array (two
calls, a fork, reset, off, uncount, fetch / add and their range errors), and the text kernels against salt_depth_text on the same array at
tile sizes that put a carry, a run's start and a window's partial sum on every kind of tile edge."""
import gzip
import os

import numpy as np
import pytest

import depth_check
import snp_check
import gap_cases
from conftest import EXTRA_CASES, LAMBDA, ROOT

pytestmark = pytest.mark.gpu

EDGE, REF_LEN = 48502, 97004
TILES = [64, 1000, 48502, 97004, 1 << 20]

# the sets of tests/test_gpu_snp_counts.py: name -> (salt arguments, FASTQ files under tests/golden/lambda, plain or .gz)
SE_SETS = {
    "se_default": (["-d", "-c"], ["reads_se.fq"]), "ragged_default": EXTRA_CASES["ragged_default"], "span_default": EXTRA_CASES["span_default"],
    "gap_se_mid": (gap_cases.GAP_CASES["gap_se_mid"][0], ["reads_gap_se_mid.fq.gz"]),
}
PE_SETS = {
    "pe_default": (["-d", "-p", "-c", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"]), "ragged_pe": EXTRA_CASES["ragged_pe"],
    "gap_pe_short": (gap_cases.GAP_CASES["gap_pe_short"][0], ["reads_gap_pe_short_1.fq.gz", "reads_gap_pe_short_2.fq.gz"]),
}


def _fq(name):
    data = open(os.path.join(LAMBDA, name), "rb").read()
    return gzip.decompress(data) if name.endswith(".gz") else data


def _opt(salt_amd, ix, args):
    return salt_amd.AlnOpt.from_argv(list(args), ix.l_seed)[0]


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=8192)
    aln.set_contigs(ix)
    yield salt_amd, ix, aln
    aln.close()
    ix.destroy()


def _diff(aln):
    return aln.depth_fetch(0, REF_LEN + 1)


def test_before_the_first_enable_every_call_says_never_enabled(lam):
    salt_amd, ix, _ = lam
    other = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    try:
        other.set_contigs(ix)
        calls = (other.depth_reset, lambda: other.depth_fetch(0, 1), lambda: other.depth_add(0, np.zeros(1, dtype=np.uint32)), other.depth_text, other.depth_uncount)
        for call in calls:
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
        with pytest.raises(salt_amd.SaltError, match="255"):
            other.depth_enable(True, 256)
        other.depth_enable(False)                                    # stopping what never ran is no error, and allocates nothing
        for call in calls:
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
    finally:
        other.close()


@pytest.fixture(scope="module")
def se_diffs(lam):
    """name -> {"sam": SAM of the text call, 0 / 20: the device's array at that min_mapq after that call alone}: computed once, shared."""
    salt_amd, ix, aln = lam
    out = {}
    for name, (args, files) in SE_SETS.items():
        opt, fq = _opt(salt_amd, ix, args), _fq(files[0])
        per_q = {}
        for q in (0, 20):
            aln.depth_enable(True, q)
            aln.depth_reset()
            sam, n = aln.align_se_text(opt, fq)
            per_q[q] = _diff(aln)
            aln.depth_enable(False)
            assert sam == per_q.setdefault("sam", sam) and n > 0
        out[name] = per_q
    return out


@pytest.fixture(scope="module")
def pe_diffs(lam):
    salt_amd, ix, aln = lam
    out = {}
    for name, (args, files) in PE_SETS.items():
        opt, fq1, fq2 = _opt(salt_amd, ix, args), _fq(files[0]), _fq(files[1])
        per_q = {}
        for q in (0, 20):
            aln.depth_enable(True, q)
            aln.depth_reset()
            sam, n = aln.align_pe_text(opt, ix, fq1, fq2)
            per_q[q] = _diff(aln)
            aln.depth_enable(False)
            assert sam == per_q.setdefault("sam", sam) and n > 0
        out[name] = per_q
    return out


def _same(name, got, want, min_mapq):
    assert got.shape == want.shape == (REF_LEN + 1,) and got.dtype == np.uint32
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s, min_mapq %d: %d words differ; first at %s: device %s, twin %s" % (name, min_mapq, len(bad), bad[:4], got[bad[:4]], want[bad[:4]]))
    assert want.any()


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("name", sorted(SE_SETS))
def test_single_end_text_call_marks_what_the_twin_marks_over_the_calls_own_sam(name, min_mapq, lam, se_diffs):
    salt_amd, ix, _ = lam
    _same(name, se_diffs[name][min_mapq], salt_amd.depth_add_sam(ix, se_diffs[name]["sam"], min_mapq)[0], min_mapq)


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("name", sorted(PE_SETS))
def test_paired_end_text_call_marks_what_the_twin_marks_over_the_calls_own_sam(name, min_mapq, lam, pe_diffs):
    salt_amd, ix, _ = lam
    _same(name, pe_diffs[name][min_mapq], salt_amd.depth_add_sam(ix, pe_diffs[name]["sam"], min_mapq)[0], min_mapq)


def test_the_calls_cover_indels_clips_and_the_contig_boundary(lam, se_diffs, pe_diffs):
    """None of the comparisons above passes on empty ground; and the Python statement agrees on the file with the most shapes."""
    assert snp_check.census(se_diffs["gap_se_mid"]["sam"])[0] >= 1000
    assert snp_check.census(pe_diffs["gap_pe_short"]["sam"])[0] >= 300
    assert snp_check.census(pe_diffs["pe_default"]["sam"])[1] >= 40 and snp_check.census(pe_diffs["ragged_pe"]["sam"])[1] >= 40
    span = depth_check.depth_of(se_diffs["span_default"][0])
    assert (int(span[EDGE - 1]), int(span[EDGE])) == (37, 37)
    want, _ = depth_check.diff_of_sam(depth_check.lambda_contigs(), pe_diffs["gap_pe_short"]["sam"], 20)
    assert np.array_equal(pe_diffs["gap_pe_short"][20], want)


@pytest.mark.parametrize("name", sorted(SE_SETS))
def test_alnse_core1_marks_what_the_text_call_marks(name, lam, se_diffs):
    salt_amd, ix, aln = lam
    args, files = SE_SETS[name]
    names, seqs, offs, quals = salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
    aln.depth_enable(True, 20)
    aln.depth_reset()
    aln.alnse_core1(_opt(salt_amd, ix, args), seqs, offs)
    got = _diff(aln)
    aln.depth_enable(False)
    _same(name, got, se_diffs[name][20], 20)


@pytest.mark.parametrize("name", sorted(PE_SETS))
def test_alnpe_core1_marks_what_the_text_call_marks(name, lam, pe_diffs):
    salt_amd, ix, aln = lam
    args, files = PE_SETS[name]
    names, seqs, offs, quals = salt_amd.interleave_pairs(salt_amd.read_fastq(os.path.join(LAMBDA, files[0])), salt_amd.read_fastq(os.path.join(LAMBDA, files[1])))
    aln.depth_enable(True, 0)
    aln.depth_reset()
    aln.alnpe_core1(_opt(salt_amd, ix, args), ix, seqs, offs)
    got = _diff(aln)
    aln.depth_enable(False)
    _same(name, got, pe_diffs[name][0], 0)


def test_resident_entry_points_mark_on_the_callers_stream(lam, se_diffs, pe_diffs):
    import torch
    salt_amd, ix, aln = lam
    isz = salt_amd.RESULT_DTYPE.itemsize
    st = torch.cuda.Stream()
    for name, sets, want in (("ragged_default", SE_SETS, se_diffs), ("ragged_pe", PE_SETS, pe_diffs)):
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
        aln.depth_enable(True, 0)
        aln.depth_reset()
        with torch.cuda.stream(st):
            if len(files) == 1:
                aln.align_resident(opt, n, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
            else:
                aln.align_pe_resident(opt, ix, n // 2, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
        got = _diff(aln)                                             # (synchronises the device)
        aln.depth_enable(False)
        _same(name, got, want[name][0], 0)


def test_two_calls_accumulate_a_fork_adds_to_the_same_array_reset_off_and_uncount(lam, se_diffs, pe_diffs):
    salt_amd, ix, aln = lam
    opt_se, opt_pe = _opt(salt_amd, ix, SE_SETS["se_default"][0]), _opt(salt_amd, ix, PE_SETS["ragged_pe"][0])
    fq, fq1, fq2 = _fq("reads_se.fq"), _fq("reads_ragged_pe_1.fq"), _fq("reads_ragged_pe_2.fq")
    one, two = se_diffs["se_default"][0], pe_diffs["ragged_pe"][0]
    aln.depth_enable(True, 0)
    aln.depth_reset()
    sam_on, _ = aln.align_se_text(opt_se, fq)
    aln.align_se_text(opt_se, fq)
    assert np.array_equal(_diff(aln), 2 * one)
    fork = aln.fork()
    try:
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert np.array_equal(_diff(fork), 2 * one + two) and np.array_equal(_diff(aln), 2 * one + two)
        aln.depth_reset()
        assert not _diff(aln).any() and not _diff(fork).any()
        # off: nothing is marked, the array stays as it is
        aln.depth_add(0, one)
        aln.depth_enable(False)
        sam_off, _ = aln.align_se_text(opt_se, fq)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert np.array_equal(_diff(aln), one)
        assert sam_on == sam_off == se_diffs["se_default"]["sam"]   # the SAM bytes do not depend on the marking
        # a block that is aligned and then dropped leaves the array word for word as it was
        aln.depth_reset()
        aln.depth_enable(True, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        aln.align_se_text(opt_se, fq)
        fork.depth_uncount()
        assert np.array_equal(_diff(aln), one)
        fork.depth_uncount()                                         # only once
        assert np.array_equal(_diff(aln), one)
        aln.depth_uncount()
        assert not _diff(aln).any()
    finally:
        aln.depth_enable(False)
        fork.close()


def test_fetch_and_add_ranges_and_adding_an_array_to_itself(lam, se_diffs):
    salt_amd, ix, aln = lam
    one = se_diffs["se_default"][0]
    aln.depth_enable(False)
    aln.depth_reset()
    aln.depth_add(0, one)
    assert np.array_equal(_diff(aln), one)
    assert np.array_equal(aln.depth_fetch(1000, 5000), one[1000:6000]) and aln.depth_fetch(REF_LEN + 1, 0).size == 0
    assert np.array_equal(aln.depth_fetch(REF_LEN, 1), one[REF_LEN:])
    # the sum path of several GPUs: an index's own array, fetched and added back in chunks, doubles every depth
    for first in range(0, REF_LEN + 1, 30000):
        n = min(30000, REF_LEN + 1 - first)
        aln.depth_add(first, aln.depth_fetch(first, n))
    assert np.array_equal(_diff(aln), 2 * one)
    assert np.array_equal(depth_check.depth_of(_diff(aln)), 2 * depth_check.depth_of(one))
    for call in (lambda: aln.depth_fetch(REF_LEN, 2), lambda: aln.depth_fetch(REF_LEN + 2, 0), lambda: aln.depth_fetch(0, REF_LEN + 2),
                 lambda: aln.depth_add(REF_LEN, np.zeros(2, dtype=np.uint32)), lambda: aln.depth_add(1 << 40, np.zeros(1, dtype=np.uint32))):
        with pytest.raises(salt_amd.SaltError, match=r"leave the array's \[0, 97004\]"):
            call()
    assert np.array_equal(_diff(aln), 2 * one)


def _arrays(salt_amd, ix):
    zero = np.zeros(REF_LEN + 1, dtype=np.uint32)
    alt = np.ones(REF_LEN + 1, dtype=np.uint32)                      # depth 1 2 1 2 ...: every position its own run
    alt[2::2] = 0xFFFFFFFF
    alt[REF_LEN] = 0
    contig_a = zero.copy()
    contig_a[0], contig_a[EDGE] = 3, (1 << 32) - 3
    big = zero.copy()
    big[10], big[60000] = 4000000000, (1 << 32) - 4000000000
    wrap = zero.copy()
    wrap[500], wrap[999], wrap[1001], wrap[48600] = 3000000000, 3000000000, (1 << 32) - 3000000000, (1 << 32) - 3000000000
    out = {"zero": zero, "every_position": alt, "contig_a": contig_a, "ten_digits": big, "wrap": wrap}
    for golden in ("expect_span_default.sam", "expect_se_default.sam", "expect_gap_pe_short.sam.gz"):
        out[golden] = salt_amd.depth_add_sam(ix, snp_check.golden_sam(golden))[0]
    return out


ARRAYS = ["zero", "every_position", "contig_a", "ten_digits", "wrap", "expect_span_default.sam", "expect_se_default.sam", "expect_gap_pe_short.sam.gz"]


@pytest.mark.parametrize("name", ARRAYS)
def test_text_kernels_equal_the_twin_on_the_same_array_at_every_tile_size(name, lam):
    salt_amd, ix, aln = lam
    arr = _arrays(salt_amd, ix)[name]
    aln.depth_enable(False)
    aln.depth_reset()
    aln.depth_add(0, arr)
    want = {w: salt_amd.depth_text(ix, arr, w) for w in (0, 1000, 7)}
    if name == "zero":
        assert want[0] == b"lambdaA\t0\t48502\t0\nlambdaB_div2pct\t0\t48502\t0\n"
    if name == "every_position":
        assert want[0].count(b"\n") == REF_LEN
    if name == "contig_a":
        assert want[0] == b"lambdaA\t0\t48502\t3\nlambdaB_div2pct\t0\t48502\t0\n"
    if name == "expect_span_default.sam":
        assert b"\t48502\t37\nlambdaB_div2pct\t0\t" in want[0]
    for tile in TILES:
        for w in (0, 1000, 7):
            pieces = aln.depth_text(window=w, tile_positions=tile, pieces=True)
            got = b"".join(pieces)
            assert got == want[w], (name, tile, w, len(got), len(want[w]))
            if name == "every_position" and tile == 64 and w == 0:
                assert len(pieces) > REF_LEN // 64                     # the lines of a tile outgrow its buffer and leave in several pieces
    assert aln.depth_text() == want[0] and aln.depth_text(window=1000) == want[1000]      # the default tile
    assert np.array_equal(_diff(aln), arr)                           # the array is only read


def test_finishing_twice_bgzf_pieces_and_marking_after_finishing(lam, se_diffs):
    salt_amd, ix, aln = lam
    one = se_diffs["se_default"][0]
    opt = _opt(salt_amd, ix, SE_SETS["se_default"][0])
    aln.depth_reset()
    aln.depth_enable(True, 0)
    aln.align_se_text(opt, _fq("reads_se.fq"))
    first = aln.depth_text(tile_positions=1000)
    assert first == salt_amd.depth_text(ix, one) and first.count(b"\n") == 3940
    assert aln.depth_text(tile_positions=1000) == first
    for w, tile in ((0, 1000), (0, 0), (1000, 48502), (0, 64)):
        blocks = aln.depth_text(window=w, tile_positions=tile, bgzf=True)
        assert blocks[:4] == b"\x1f\x8b\x08\x04" and gzip.decompress(blocks) == salt_amd.depth_text(ix, one, w)
    aln.align_se_text(opt, _fq("reads_se.fq"))                       # marking goes on after a text was made
    aln.depth_enable(False)
    assert np.array_equal(_diff(aln), 2 * one)
    assert aln.depth_text(window=64) == salt_amd.depth_text(ix, 2 * one, 64)


# ---- the `salt` binary on the GPU ----
SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    import subprocess
    prefix = str(tmp_path_factory.mktemp("depthidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


def _salt(args, **env):
    import subprocess
    return subprocess.run([SALT] + args, capture_output=True, timeout=300, env=dict(os.environ, **env))


def _twin_text(salt_amd, ix, sam, min_mapq=0, window=0):
    diff, n = salt_amd.depth_add_sam(ix, sam, min_mapq)
    assert n > 0
    return salt_amd.depth_text(ix, diff, window)


def test_cli_file_equals_the_twin_over_its_stdout_plain_gz_and_with_snp_counts(lam, lambda_cli_index, tmp_path):
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    reads = os.path.join(LAMBDA, "reads_se.fq")
    f, fz, c = tmp_path / "d.bed", tmp_path / "d.bed.gz", tmp_path / "counts.tsv"
    off = _salt(["-d", "-c", lambda_cli_index, reads])
    run = _salt(["-d", "-c", "--depth", str(f), "--depth-min-mapq", "20", lambda_cli_index, reads])
    assert off.returncode == 0 and run.returncode == 0 and b"text path" in run.stderr and b"marked and printed on the device" in run.stderr, run.stderr[-600:]
    assert strip_pg(run.stdout) == strip_pg(off.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert f.read_bytes() == _twin_text(salt_amd, ix, run.stdout, 20)
    gz = _salt(["-d", "-c", "--depth", str(fz), "--depth-min-mapq", "20", "--snp-counts", str(c), lambda_cli_index, reads])
    assert gz.returncode == 0 and strip_pg(gz.stdout) == strip_pg(off.stdout), gz.stderr[-600:]
    z = fz.read_bytes()
    assert z.endswith(BGZF_EOF) and gzip.decompress(z) == f.read_bytes()
    _, counts = snp_check.parse_counts_file(c.read_bytes())
    assert np.array_equal(counts, salt_amd.snp_count_sam(ix, gz.stdout, 0).astype(np.uint64))


def test_cli_windows_of_1000_as_bgzf(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    fw = tmp_path / "w.bed.gz"
    win = _salt(["-d", "-c", "--depth", str(fw), "--depth-window", "1000", lambda_cli_index, os.path.join(LAMBDA, "reads_se.fq")])
    assert win.returncode == 0 and b"windows of 1000" in win.stderr, win.stderr[-600:]
    text = gzip.decompress(fw.read_bytes())
    assert text == _twin_text(salt_amd, ix, win.stdout, 0, 1000) and text.count(b"\n") == 98


def test_cli_paired_end_and_under_polish(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    args = ["-d", "-p", "-c", "-a", "350", "-b", "650"]
    files = [os.path.join(LAMBDA, "reads_pe_1.fq"), os.path.join(LAMBDA, "reads_pe_2.fq")]
    f, fp = tmp_path / "pe.bed", tmp_path / "pe_polish.bed"
    run = _salt(args + ["--depth", str(f), lambda_cli_index] + files)
    assert run.returncode == 0 and b"marked and printed on the device" in run.stderr, run.stderr[-600:]
    assert f.read_bytes() == _twin_text(salt_amd, ix, run.stdout)
    pol = _salt(args + ["--polish", "--depth", str(fp), lambda_cli_index] + files)
    alone = _salt(args + ["--polish", lambda_cli_index] + files)
    assert pol.returncode == 0 and alone.returncode == 0, pol.stderr[-600:]
    assert fp.read_bytes() == f.read_bytes()                         # the rows are marked, whatever is printed of them
    assert pol.stdout == alone.stdout and len(alone.stdout) > 100000


def test_cli_marks_every_written_block_once_across_the_hand_over(lam, lambda_cli_index, tmp_path):
    """A multi-line record in the middle of the file, chunks of 9 000 bytes: the blocks the workers had aligned behind the refused chunk
    are dropped and their marks taken back (salt_gpu_ws_depth_uncount); the host pipeline aligns those reads again."""
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq, f = tmp_path / "mid_multiline.fq", tmp_path / "d.bed"
    fq.write_bytes(b"\n".join(out) + b"\n")
    run = _salt(["-d", "-c", "-t", "8", "--depth", str(f), lambda_cli_index, str(fq)], SALT_CHUNK_BYTES="9000")
    assert run.returncode == 0, run.stderr[-600:]
    assert b"the host parser takes over" in run.stderr and b"marked and printed on the device" in run.stderr
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert f.read_bytes() == _twin_text(salt_amd, ix, run.stdout) and f.read_bytes().count(b"\n") == 3940
