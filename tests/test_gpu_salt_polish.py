"""`salt --polish` on the device: the aligner's hits go from the result rows straight into the polish kernels (k_pl_rows, salt_polish.hip) and
stdout carries what `polish` prints for the run's SAM lines.  Against the outputs of the REAL reference `polish` committed under
tests/golden/lambda (the ACGT-only reads of the fixtures: the reference's output for the others is undefined), through the binary and through
GpuAligner.set_polish; against the two-step result -- the product's own `salt`, then its own `polish`, on the same device -- for the inputs
the reference cannot run (reads with N, ragged lengths, skipped reads); block cuts, the host pipeline, --bgzf, the unchanged SAM output, the
errors.  Two-step result: the record lines `salt` prints without the option, the header and the empty lines taken out and -- paired end --
both records of a pair with a skipped mate (more than 200 N) taken out too, through `polish [-p] [-s]`."""
import os
import subprocess
import sys

import pytest

import bgzf_check
from conftest import GOLDEN, LAMBDA, ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)

SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
POLISH = os.path.join(ROOT, "salt_amd", "bin", "polish")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
PE = ["-p", "-a", "350", "-b", "650"]


def golden(name):
    return open(os.path.join(LAMBDA, name), "rb").read()


def records(path):
    """the 4-line records of a FASTQ fixture"""
    lines = open(path, "rb").read().split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    assert len(lines) % 4 == 0
    return [lines[i:i + 4] for i in range(0, len(lines), 4)]


def acgt_only(paths, d):
    """the fixture files without the reads (the pairs) that hold a base outside ACGT, written into d"""
    recs = [records(os.path.join(LAMBDA, p)) for p in paths]
    keep = [i for i in range(len(recs[0])) if all(set(r[i][1]) <= set(b"ACGT") for r in recs)]
    out = []
    for p, r in zip(paths, recs):
        out.append(str(d / ("acgt_" + p)))
        with open(out[-1], "wb") as f:
            f.write(b"".join(b"\n".join(r[i]) + b"\n" for i in keep))
    return out, len(keep)


def stop_at_a_fault(rc, text):
    """a device fault, an abort or a segmentation fault ends the session: nothing more is started on that device"""
    if rc in (134, 139, -6, -11) or b"illegal memory access" in text or b"HSA_STATUS_ERROR" in text:
        pytest.exit("a child died or the device faulted (status %s): %s" % (rc, text[-600:].decode("latin-1")), returncode=3)


def run(cmd, env=None, timeout=120):
    p = subprocess.run(cmd, capture_output=True, env=dict(os.environ, **(env or {})), timeout=timeout)
    stop_at_a_fault(p.returncode, p.stderr)
    assert p.returncode == 0, (cmd, p.stderr[-600:])
    return p


def salt(prefix, args, files, env=None):
    return run([SALT] + list(args) + [prefix] + list(files), env).stdout


def skipped(rec):
    return sum(1 for c in rec[1] if c not in b"ACGTacgt") > 200


def two_step(prefix, args, files, sw, tmp_path):
    """`salt`, then `polish`, with what a user has to do in between"""
    paired = "-p" in args
    lines = [l for l in salt(prefix, args, files).split(b"\n") if l and not l.startswith(b"@")]
    if paired:
        r1, r2 = records(files[0]), records(files[1])
        assert len(lines) == 2 * len(r1)
        lines = [l for i, l in enumerate(lines) if not skipped(r1[i // 2]) and not skipped(r2[i // 2])]
    sam = tmp_path / "two_step.sam"
    sam.write_bytes(b"".join(l + b"\n" for l in lines))
    return run([POLISH] + (["-p"] if paired else []) + (["-s"] if sw else []) + [prefix, str(sam)]).stdout


def same(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
    assert len(g) == len(w) and not bad, (len(g), len(w), len(bad), [(g[i][:200], w[i][:200]) for i in bad[:2]])


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("saltpolidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), p], check=True, stderr=subprocess.DEVNULL)
    return p


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    d = tmp_path_factory.mktemp("acgt")
    se, n_se = acgt_only(["reads_se.fq"], d)
    pe, n_pe = acgt_only(["reads_pe_1.fq", "reads_pe_2.fq"], d)
    assert (n_se, n_pe) == (1921, 1000)
    return se, pe


REFERENCE = {
    "expect_polish_se_lv.sam": (["--polish"], False),
    "expect_polish_se_sw.sam": (["--polish=sw"], False),
    "expect_polish_se_r1_lv.sam": (["--polish", "-r", "1", "-m", "500", "-n", "20"], False),
    "expect_polish_pe_lv.sam": (["--polish"] + PE, True),
    "expect_polish_pe_sw.sam": (["--polish=sw"] + PE, True),
}


@pytest.mark.parametrize("name", sorted(REFERENCE))
def test_the_binary_prints_what_the_reference_polish_printed(name, prefix, clean):
    args, paired = REFERENCE[name]
    same(salt(prefix, args, clean[1] if paired else clean[0]), golden(name))


@pytest.fixture(scope="module")
def lambda_index():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield ix
    ix.destroy()


@pytest.fixture(scope="module")
def aligner(lambda_index):
    import salt_amd
    aln = salt_amd.GpuAligner(lambda_index, device=0, max_reads=8192)
    aln.set_contigs(lambda_index)
    aln.set_pac(lambda_index)
    yield aln
    aln.close()


def api_call(aligner, ix, args, files):
    import salt_amd
    opt = salt_amd.AlnOpt.from_argv([a for a in args if not a.startswith("--polish")], ix.l_seed)[0]
    fq = [open(f, "rb").read() for f in files]
    try:
        return aligner.align_pe_text(opt, ix, *fq) if len(fq) == 2 else aligner.align_se_text(opt, fq[0])
    except salt_amd.SaltError as e:
        stop_at_a_fault(0, str(e).encode())
        raise


@pytest.mark.parametrize("name", sorted(REFERENCE))
def test_the_library_returns_what_the_reference_polish_printed(name, aligner, lambda_index, clean):
    args, paired = REFERENCE[name]
    aligner.set_polish("sw" if "--polish=sw" in args else "lv")
    try:
        got, n = api_call(aligner, lambda_index, args, clean[1] if paired else clean[0])
    finally:
        aligner.set_polish(0)
    same(got, golden(name))
    assert n == (1000 if paired else 1921)                       # reads / pairs of the input, as without the option


def test_after_set_polish_0_the_workspace_returns_sam_again(aligner, lambda_index):
    files = [os.path.join(LAMBDA, "reads_se.fq")]
    sam, n = api_call(aligner, lambda_index, ["-d", "-c"], files)
    aligner.set_polish(1)
    polished, n1 = api_call(aligner, lambda_index, ["-d", "-c"], files)
    aligner.set_polish(0)
    assert api_call(aligner, lambda_index, ["-d", "-c"], files) == (sam, n) and n1 == n
    assert polished != sam and sam == b"".join(l for l in golden("expect_se_default.sam").splitlines(keepends=True) if not l.startswith(b"@"))


def written_fastq(d):
    """one read, one pair, a read of 250 N between two normal reads, a pair whose first mate is 250 N: (single-end file, mate files)"""
    se, m1, m2 = records(os.path.join(LAMBDA, "reads_se.fq")), records(os.path.join(LAMBDA, "reads_pe_1.fq")), records(os.path.join(LAMBDA, "reads_pe_2.fq"))
    n250 = lambda name: [name, b"N" * 250, b"+", b"I" * 250]
    text = lambda recs: b"".join(b"\n".join(r) + b"\n" for r in recs)
    out = {"one_read": [text(se[:1])], "one_pair": [text(m1[:1]), text(m2[:1])],
           "n250_between": [text([se[0], n250(b"@allN"), se[1]])],
           "n250_mate": [text([m1[0], n250(b"@allN/1"), m1[2]]), text([m2[0], m2[1], m2[2]])]}
    files = {}
    for k, parts in out.items():
        files[k] = []
        for j, t in enumerate(parts):
            files[k].append(str(d / ("%s_%d.fq" % (k, j + 1))))
            open(files[k][-1], "wb").write(t)
    return files


TWO_STEP = {
    "reads_se": ([], ["reads_se.fq"]), "reads_se_sw": ([], ["reads_se.fq"]), "ragged": ([], ["reads_ragged.fq"]),
    "ragged_pe": (["-p", "-a", "300", "-b", "700"], ["reads_ragged_pe_1.fq", "reads_ragged_pe_2.fq"]),
    "ragged_pe_sw": (["-p", "-a", "300", "-b", "700"], ["reads_ragged_pe_1.fq", "reads_ragged_pe_2.fq"]),
    "one_read": ([], None), "one_pair": (PE, None), "n250_between": ([], None), "n250_mate": (PE, None),
}


@pytest.mark.parametrize("name", sorted(TWO_STEP))
def test_the_binary_prints_the_two_step_result(name, prefix, tmp_path):
    args, files = TWO_STEP[name]
    files = [os.path.join(LAMBDA, f) for f in files] if files else written_fastq(tmp_path)[name]
    sw = name.endswith("_sw")
    want = two_step(prefix, args, files, sw, tmp_path)
    got = salt(prefix, ["--polish=sw" if sw else "--polish"] + args, files)
    same(got, want)
    n_in = len(records(files[0])) * len(files)
    expect = {"n250_between": 2, "n250_mate": 4}.get(name, n_in)   # no record for a skipped read, none for either mate of its pair
    assert got.count(b"\n") == expect and not got.startswith(b"@")


def test_irrelevant_options_change_nothing(prefix):
    files = [os.path.join(LAMBDA, "reads_ragged.fq")]
    assert salt(prefix, ["--polish", "-c", "-d", "-g", "grp1"], files) == salt(prefix, ["--polish"], files)


def test_block_cuts_do_not_show(prefix):
    files = [os.path.join(LAMBDA, "reads_se.fq")]
    whole = salt(prefix, ["--polish"], files)
    assert os.path.getsize(files[0]) > 4 * 65536                 # several chunks, cut wherever 64 KiB end
    assert salt(prefix, ["--polish"], files, {"SALT_CHUNK_BYTES": "65536"}) == whole and whole.count(b"\n") > 1900


@pytest.mark.parametrize("paired", [False, True])
def test_the_host_pipeline_prints_the_same_bytes(paired, prefix, tmp_path):
    if paired:
        args, files = ["-p", "-a", "300", "-b", "700"], [os.path.join(LAMBDA, "reads_ragged_pe_1.fq"), os.path.join(LAMBDA, "reads_ragged_pe_2.fq")]
    else:
        args, files = [], written_fastq(tmp_path)["n250_between"]
    text = run([SALT, "--polish"] + args + [prefix] + files)
    host = run([SALT, "--polish"] + args + [prefix] + files, {"SALT_HOST_PIPELINE": "1"})
    assert b"text path" in text.stderr and b"text path" not in host.stderr
    same(host.stdout, text.stdout)
    assert len(text.stdout) > 200


def test_polish_bgzf_inflates_to_the_plain_bytes(prefix):
    files = [os.path.join(LAMBDA, "reads_se.fq")]
    plain = salt(prefix, ["--polish"], files)
    z = salt(prefix, ["--polish", "--bgzf"], files)
    assert bgzf_check.stream_text(z) == plain and len(z) < len(plain) // 2


@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_without_the_option_the_sam_stream_is_the_golden(case, prefix):
    args, files = (["-d", "-c"], ["reads_se.fq"]) if case == "se_default" else (["-d", "-p", "-c", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"])
    got = salt(prefix, args, [os.path.join(LAMBDA, f) for f in files])
    lines = lambda t: [l for l in t.split(b"\n") if not l.startswith(b"@")]      # (the header names the command line)
    assert lines(got) == lines(golden("expect_%s.sam" % case)) and got.startswith(b"@")


def test_set_polish_needs_the_genome_and_excludes_bam(lambda_index):
    import salt_amd
    aln = salt_amd.GpuAligner(lambda_index, device=0, max_reads=64)     # its own device index: no 2-bit genome yet
    try:
        aln.set_contigs(lambda_index)
        with pytest.raises(salt_amd.SaltError, match="salt_gpu_index_set_pac"):
            aln.set_polish(1)
        aln.set_pac(lambda_index)
        aln.set_sam_bam(True)
        with pytest.raises(salt_amd.SaltError, match="salt_gpu_ws_set_sam_bam"):
            aln.set_polish(1)
        aln.set_sam_bam(False)
        aln.set_polish(2)
        with pytest.raises(salt_amd.SaltError, match="salt_gpu_ws_set_polish"):
            aln.set_sam_bam(True)
        with pytest.raises(salt_amd.SaltError, match="polish mode"):
            aln.set_polish(3)
    finally:
        aln.close()
