"""Genotypes at the SNP sites on the device (salt --genotype).  The sums: k_gt_add behind every entry point that leaves result
rows against the host twin (salt_gt_add_sam) over the SAM text of the same reads -- text, host-buffer with and without set_quals, resident,
single and paired end, with the fixtures' own qualities and with quality lines rewritten by a seeded pattern.  The state: two calls, a
fork, reset, off, uncount, the errors.  The call and the text: a hand-made table (gt_check.hand_made) through gt_add, the device's text
against salt_gt_text byte for byte.  Then the `salt` binary with --genotype."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import gap_cases
import gt_check
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
ALL_SETS = dict(SE_SETS, **PE_SETS)
EDGE_BYTES = (33, 34, 35, 93, 126)                 # q 0, 1, 2 (the clamp's edge), 60 (the other edge), 93 (the last row)


def _fq(name):
    data = open(os.path.join(LAMBDA, name), "rb").read()
    return gzip.decompress(data) if name.endswith(".gz") else data


def _pattern(rng, n, extra=()):
    """n quality bytes: the edge bytes (and `extra`) often, the rest uniform in 33 .. 126"""
    q = rng.randint(33, 127, size=n).astype(np.uint8)
    special = np.array(EDGE_BYTES + tuple(extra), dtype=np.uint8)
    pick = rng.randint(0, 3, size=n) == 0
    q[pick] = special[rng.randint(0, len(special), size=int(pick.sum()))]
    return q


def _rewrite_fastq(fq, seed):
    """the strict 4-line FASTQ with every quality line replaced by the pattern"""
    lines = fq.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    rng = np.random.RandomState(seed)
    for i in range(3, len(lines) - 1, 4):
        assert lines[i - 1].startswith(b"+") and len(lines[i]) == len(lines[i - 2])
        lines[i] = _pattern(rng, len(lines[i])).tobytes()
    return b"\n".join(lines)


def _sam_with_quals(sam, quals_of):
    """the SAM text with every record's QUAL replaced by quals_of(name, mate) as printed: reversed for a reverse read, bytes outside
    33 .. 126 as '5' (q 20 = SALT_GT_Q_NONE); quals_of None: `*`"""
    out = []
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            out.append(line)
            continue
        f = line.split(b"\t")
        if quals_of is None:
            f[10] = b"*"
        else:
            flag = int(f[1])
            q = np.array(quals_of[(f[0], 1 if flag & 0x80 else 0)], dtype=np.uint8)
            q = np.where((q < 33) | (q > 126), 33 + gt_check.Q_NONE, q).astype(np.uint8)
            f[10] = (q[::-1] if flag & 0x10 else q).tobytes()
            assert len(f[10]) == len(f[9])
        out.append(b"\t".join(f))
    return b"\n".join(out)


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


def _check(what, got, want):
    assert got.shape == want.shape and got.dtype == np.uint64
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=(1, 2)))
        raise AssertionError("%s: %d sites differ; first %s: device %s, twin %s" % (what, len(bad), bad[:2], got[bad[:2]].tolist(), want[bad[:2]].tolist()))
    assert int(want[:, :, 0].sum()) > 0


def _counted(aln, min_mapq, call):
    aln.gt_enable(True, min_mapq)
    aln.gt_reset()
    try:
        out = call()
        return out, aln.gt_fetch()
    finally:
        aln.gt_enable(False)


def _text_call(salt_amd, ix, aln, name, fqs, min_mapq):
    opt = _opt(salt_amd, ix, ALL_SETS[name][0])
    if len(fqs) == 1:
        return _counted(aln, min_mapq, lambda: aln.align_se_text(opt, fqs[0])[0])
    return _counted(aln, min_mapq, lambda: aln.align_pe_text(opt, ix, fqs[0], fqs[1])[0])


@pytest.fixture(scope="module")
def text_sums(lam):
    """name -> (SAM of the text call, the device's sums of that call at min_mapq 0): computed once, shared"""
    salt_amd, ix, aln = lam
    return {name: _text_call(salt_amd, ix, aln, name, [_fq(f) for f in files], 0) for name, (_, files) in ALL_SETS.items()}


def test_before_the_first_enable_the_errors(lam):
    salt_amd, ix, _ = lam
    other = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    other.set_contigs(ix)
    try:
        for call in (other.gt_reset, lambda: other.gt_fetch(0, 1), lambda: other.gt_add(0, np.zeros((1, 4, 4), dtype=np.uint64)), other.gt_text, other.gt_uncount):
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
        with pytest.raises(salt_amd.SaltError, match="256"):
            other.gt_enable(True, 256)
        other.gt_enable(False)                                       # stopping what never ran is no error, and builds nothing
        with pytest.raises(salt_amd.SaltError, match="never enabled"):
            other.gt_fetch(0, 1)
        with pytest.raises(salt_amd.SaltError, match="never enabled"):
            other.snp_counts()                                       # ... and the genotype sums' enable does not turn the SNP counts on
    finally:
        other.close()


@pytest.mark.parametrize("name", sorted(ALL_SETS))
def test_text_call_sums_equal_the_twin_over_the_calls_own_sam(name, lam, text_sums):
    salt_amd, ix, _ = lam
    sam, got = text_sums[name]
    want, n = salt_amd.gt_add_sam(ix, sam, 0)
    _check(name, got, want)
    assert n > 0


@pytest.mark.parametrize("name", sorted(ALL_SETS))
def test_text_call_with_rewritten_quality_lines_at_min_mapq_20(name, lam, text_sums):
    salt_amd, ix, aln = lam
    fqs = [_rewrite_fastq(_fq(f), 7 + k) for k, f in enumerate(ALL_SETS[name][1])]
    sam, got = _text_call(salt_amd, ix, aln, name, fqs, 20)
    quals = b"".join(line.split(b"\t")[10] for line in sam.split(b"\n") if line and not line.startswith(b"@"))
    assert all(bytes([b]) in quals for b in EDGE_BYTES)
    want, n = salt_amd.gt_add_sam(ix, sam, 20)
    _check(name, got, want)
    assert n > 0 and not np.array_equal(got, text_sums[name][1])


def test_the_python_statement_agrees_on_the_set_with_the_most_shapes(lam, text_sums):
    salt_amd, ix, _ = lam
    sam, got = text_sums["gap_pe_short"]
    want, _ = gt_check.add_sam(gt_check.Genome(), sam, 0)
    assert np.array_equal(got, gt_check.as_array(want))


def _read_set(salt_amd, files):
    if len(files) == 1:
        return salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
    return salt_amd.interleave_pairs(salt_amd.read_fastq(os.path.join(LAMBDA, files[0])), salt_amd.read_fastq(os.path.join(LAMBDA, files[1])))


def _quals_of(names, offs, flat, pe):
    out = {(bytes(nm), (i & 1) if pe else 0): flat[offs[i]:offs[i + 1]] for i, nm in enumerate(names)}
    assert len(out) == len(names)
    return out


@pytest.mark.parametrize("name", ["se_default", "gap_se_mid", "pe_default", "gap_pe_short"])
def test_host_buffer_calls_with_and_without_set_quals(name, lam, text_sums):
    salt_amd, ix, aln = lam
    pe = name in PE_SETS
    args, files = ALL_SETS[name]
    names, seqs, offs, quals = _read_set(salt_amd, files)
    opt = _opt(salt_amd, ix, args)
    call = (lambda: aln.alnpe_core1(opt, ix, seqs, offs)) if pe else (lambda: aln.alnse_core1(opt, seqs, offs))
    sam = text_sums[name][0]
    # without: every event at SALT_GT_Q_NONE, as the twin counts a record with QUAL *
    _, got = _counted(aln, 0, call)
    _check(name + " without", got, salt_amd.gt_add_sam(ix, _sam_with_quals(sam, None), 0)[0])
    assert np.array_equal(got[:, :, 1], got[:, :, 0] * np.uint64(gt_check.TABLE[gt_check.Q_NONE][0]))
    # with the fixture's own: the text call's sums
    own = np.frombuffer(b"".join(quals), dtype=np.uint8)
    aln.set_quals(own)
    _, got = _counted(aln, 0, call)
    _check(name + " own", got, text_sums[name][1])
    # with the pattern, bytes 0 and 255 among it; the bytes are consumed: the call behind it counts without again
    flat = _pattern(np.random.RandomState(11), len(own), extra=(0, 255, 10, 32, 127))
    assert all((flat == b).any() for b in EDGE_BYTES + (0, 255))
    aln.set_quals(flat)
    _, got = _counted(aln, 20, call)
    _check(name + " pattern", got, salt_amd.gt_add_sam(ix, _sam_with_quals(sam, _quals_of(names, offs, flat, pe)), 20)[0])
    _, again = _counted(aln, 20, call)
    _check(name + " consumed", again, salt_amd.gt_add_sam(ix, _sam_with_quals(sam, None), 20)[0])


def test_resident_entry_points_with_device_quals_on_the_callers_stream(lam, text_sums):
    import torch
    salt_amd, ix, aln = lam
    isz = salt_amd.RESULT_DTYPE.itemsize
    st = torch.cuda.Stream()
    for name in ("ragged_default", "ragged_pe"):
        args, files = ALL_SETS[name]
        names, seqs, offs, quals = _read_set(salt_amd, files)
        n, max_len = len(offs) - 1, int(np.diff(offs).max())
        flat = _pattern(np.random.RandomState(13), int(offs[-1]), extra=(0, 255))
        d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(64, dtype=np.uint8)])).cuda()
        d_quals = torch.from_numpy(flat.copy()).cuda()
        d_offs = torch.from_numpy(np.asarray(offs).astype(np.int32)).cuda()
        d_res = torch.zeros(n * isz, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        opt = _opt(salt_amd, ix, args)

        def call():
            with torch.cuda.stream(st):
                if len(files) == 1:
                    aln.align_resident(opt, n, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
                else:
                    aln.align_pe_resident(opt, ix, n // 2, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)

        sam = text_sums[name][0]
        aln.set_quals(d_quals.data_ptr(), on_device=True)
        _, got = _counted(aln, 0, call)                              # (gt_fetch synchronises the device)
        _check(name + " device quals", got, salt_amd.gt_add_sam(ix, _sam_with_quals(sam, _quals_of(names, offs, flat, len(files) == 2)), 0)[0])
        _, got = _counted(aln, 0, call)
        _check(name + " none", got, salt_amd.gt_add_sam(ix, _sam_with_quals(sam, None), 0)[0])


def test_two_calls_add_a_fork_shares_the_sums_reset_off_and_uncount(lam, text_sums):
    salt_amd, ix, aln = lam
    opt_se, opt_pe = _opt(salt_amd, ix, SE_SETS["se_default"][0]), _opt(salt_amd, ix, PE_SETS["ragged_pe"][0])
    fq, fq1, fq2 = _fq("reads_se.fq"), _fq("reads_ragged_pe_1.fq"), _fq("reads_ragged_pe_2.fq")
    (sam_one, one), (_, two) = text_sums["se_default"], text_sums["ragged_pe"]
    n_sites = len(one)
    aln.gt_enable(True, 0)
    aln.gt_reset()
    fork = aln.fork()
    try:
        sam_on, _ = aln.align_se_text(opt_se, fq)
        aln.align_se_text(opt_se, fq)
        assert np.array_equal(aln.gt_fetch(), 2 * one)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert np.array_equal(fork.gt_fetch(), 2 * one + two)
        assert np.array_equal(aln.gt_fetch(100, 50), (2 * one + two)[100:150]) and aln.gt_fetch(n_sites, 0).shape == (0, 4, 4)
        for call in (lambda: aln.gt_fetch(n_sites - 1, 2), lambda: aln.gt_fetch(n_sites + 1, 0), lambda: aln.gt_add(n_sites, np.ones((1, 4, 4), dtype=np.uint64))):
            with pytest.raises(salt_amd.SaltError, match=str(n_sites)):
                call()
        with pytest.raises(salt_amd.SaltError, match="300"):
            aln.gt_enable(True, 300)
        aln.gt_reset()
        assert not aln.gt_fetch().any() and not fork.gt_fetch().any()
        aln.gt_enable(False)
        sam_off, _ = aln.align_se_text(opt_se, fq)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert not aln.gt_fetch().any()
        assert sam_on == sam_off == sam_one                          # the SAM bytes do not depend on the tally
        # a block that is aligned and then dropped leaves the sums as they were
        aln.gt_enable(True, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        aln.align_se_text(opt_se, fq)
        fork.gt_uncount()
        assert np.array_equal(aln.gt_fetch(), one)
        fork.gt_uncount()                                            # only once
        assert np.array_equal(aln.gt_fetch(), one)
        aln.gt_uncount()
        assert not aln.gt_fetch().any()
        # gt_add: word by word, on top of what is there
        aln.gt_add(0, one)
        aln.gt_add(10, two[10:200])
        want = one.copy()
        want[10:200] += two[10:200]
        assert np.array_equal(aln.gt_fetch(), want)
    finally:
        aln.gt_enable(False)
        aln.gt_reset()
        fork.close()


def test_under_set_polish_the_sums_are_the_plain_calls(lam, text_sums):
    salt_amd, ix, aln = lam
    aln.set_pac(ix)
    aln.set_polish(1)
    try:
        _, got = _text_call(salt_amd, ix, aln, "se_default", [_fq("reads_se.fq")], 0)
        assert np.array_equal(got, text_sums["se_default"][1])
    finally:
        aln.set_polish(0)


def _gunzip_members(data):
    """the text of back-to-back gzip members"""
    import zlib
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        data = d.unused_data
    return b"".join(out)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """the small index with two-, three- and four-allele sites, its hand-made sums on the device, and the twin's text of them"""
    import salt_amd
    prefix = gt_check.synth_index(tmp_path_factory.mktemp("gtsynth"))
    ix = salt_amd.Index.reload(prefix)
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    aln.set_contigs(ix)
    sums, census = gt_check.hand_made(gt_check.Genome(prefix))
    sums = gt_check.as_array(sums)
    aln.gt_enable(True)
    aln.gt_enable(False)
    aln.gt_add(0, sums)
    yield salt_amd, aln, sums, salt_amd.gt_text(ix, sums)
    aln.close()
    ix.destroy()


@pytest.mark.parametrize("tile_sites", [1, 7, 64, 0])
def test_device_text_equals_the_twins_byte_for_byte(tile_sites, synth):
    salt_amd, aln, sums, want = synth
    pieces = aln.gt_text(tile_sites=tile_sites, pieces=True)
    assert b"".join(pieces) == want
    assert len(pieces) == (len(sums) + tile_sites - 1) // tile_sites if tile_sites else len(pieces) == 1
    assert want.count(b"\n") == len(sums) and b"./." in want and b",G,T" in want


def test_bgzf_pieces_inflate_to_the_text_twice_the_same_and_the_sums_stay(synth):
    salt_amd, aln, sums, want = synth
    z = aln.gt_text(tile_sites=64, bgzf=True, pieces=True)
    assert len(z) == (len(sums) + 63) // 64 and all(p[:4] == b"\x1f\x8b\x08\x04" for p in z)
    assert _gunzip_members(b"".join(z)) == want
    assert not b"".join(z).endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))      # no end-of-file block
    assert aln.gt_text(tile_sites=64, bgzf=True, pieces=True) == z and aln.gt_text() == want
    assert np.array_equal(aln.gt_fetch(), sums)


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("gtidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


def _want_file(salt_amd, ix, sam, min_mapq, sample=None):
    sums, n = salt_amd.gt_add_sam(ix, sam, min_mapq)
    assert n > 0
    return salt_amd.gt_header(ix, sample) + salt_amd.gt_text(ix, sums)


def test_cli_file_equals_header_and_twin_over_its_stdout_plain_and_gz(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    reads = os.path.join(LAMBDA, "reads_se.fq")
    f, fz = tmp_path / "calls.vcf", tmp_path / "calls.vcf.gz"
    run = subprocess.run([SALT, "-d", "-c", "--genotype", str(f), "--genotype-min-mapq", "20", lambda_cli_index, reads], capture_output=True, timeout=300)
    assert run.returncode == 0 and b"text path" in run.stderr and b"summed, called and printed on the device" in run.stderr, run.stderr[-600:]
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    want = _want_file(salt_amd, ix, run.stdout, 20)
    assert f.read_bytes() == want and want.count(b"\n") == 3858 + want.count(b"\n#") + 1
    gz = subprocess.run([SALT, "-d", "-c", "--genotype", str(fz), "--genotype-min-mapq", "20", lambda_cli_index, reads], capture_output=True, timeout=300)
    assert gz.returncode == 0 and strip_pg(gz.stdout) == strip_pg(run.stdout), gz.stderr[-600:]
    z = fz.read_bytes()
    assert z.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")) and _gunzip_members(z) == want


def test_cli_under_polish_the_file_is_the_plain_runs(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    reads = os.path.join(LAMBDA, "reads_se.fq")
    fp = tmp_path / "calls_polish.vcf"
    pol = subprocess.run([SALT, "-d", "-c", "--polish", "--genotype", str(fp), "--genotype-min-mapq", "20", lambda_cli_index, reads], capture_output=True, timeout=300)
    assert pol.returncode == 0 and b"on the device" in pol.stderr, pol.stderr[-600:]
    assert fp.read_bytes() == _want_file(salt_amd, ix, open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read(), 20)      # (the plain run's stdout)
    alone = subprocess.run([SALT, "-d", "-c", "--polish", lambda_cli_index, reads], capture_output=True, timeout=300)
    assert alone.returncode == 0 and pol.stdout == alone.stdout and len(alone.stdout) > 100000


def test_cli_paired_end_on_the_host_pipeline_hands_the_qualities_over(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    args, files = PE_SETS["ragged_pe"]
    f = tmp_path / "calls.vcf"
    run = subprocess.run([SALT] + list(args) + ["--genotype", str(f), "--genotype-sample", "NA12878", lambda_cli_index] + [os.path.join(LAMBDA, x) for x in files],
                         capture_output=True, timeout=300, env=dict(os.environ, SALT_HOST_PIPELINE="1"))
    assert run.returncode == 0 and b"host phases" in run.stderr and b"on the device" in run.stderr, run.stderr[-600:]
    assert f.read_bytes() == _want_file(salt_amd, ix, run.stdout, 0, "NA12878")


def test_cli_counts_every_written_block_once_across_the_hand_over(lam, lambda_cli_index, tmp_path):
    """A multi-line record in the middle of the file, chunks of 9 000 bytes: the blocks the workers had aligned behind the refused chunk
    are dropped and their adds taken back (salt_gpu_ws_gt_uncount); the host pipeline, which hands its batches' qualities over with
    salt_gpu_ws_set_quals, aligns those reads again."""
    salt_amd, ix, _ = lam
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq, f = tmp_path / "mid_multiline.fq", tmp_path / "calls.vcf"
    fq.write_bytes(b"\n".join(out) + b"\n")
    run = subprocess.run([SALT, "-d", "-c", "-t", "8", "--genotype", str(f), lambda_cli_index, str(fq)], capture_output=True, timeout=300,
                         env=dict(os.environ, SALT_CHUNK_BYTES="9000"))
    assert run.returncode == 0, run.stderr[-600:]
    assert b"the host parser takes over" in run.stderr and b"on the device" in run.stderr
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert f.read_bytes() == _want_file(salt_amd, ix, run.stdout, 0)
