"""`salt --genotype` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_snp_counts_cli_stub.py.  The stub
has no salt_gpu_index_gt_enable, so the sums come from the SAM lines of every block and batch through the host twin (salt_gt_add_sam) and
the records from salt_gt_text: what is tested is the driver -- the options, the file (header + records, plain and .gz), that every line
that is written is counted once on the text path, the host pipeline and across the hand-over between them, with several "devices" -- and
that stdout is what it is without the option."""
import gzip
import os
import shutil
import subprocess

import pytest

import gt_check
from bam_check import decode_stream
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    import salt_amd
    d = tmp_path_factory.mktemp("gtstub")
    os.makedirs(d / "bin"); os.makedirs(d / "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "salt_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    shutil.copy(os.path.join(ROOT, "salt_amd", "bin", "salt"), d / "bin" / "salt")
    shutil.copy(os.path.join(ROOT, "salt_amd", "lib", "libsalt_host.so"), d / "lib" / "libsalt_host.so")
    subprocess.run(["gcc", "-O2", "-g", "-fPIC", "-shared", "-Wall", "-o", str(d / "lib" / "libsalt_gpu.so"),
                    os.path.join(ROOT, "tests", "stub", "salt_gpu_stub.c"), os.path.join(ROOT, "oracle", "salt_oracle.c"), "-lm", "-lpthread"], check=True)
    prefix = str(d / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    ix = salt_amd.Index.reload(prefix)
    yield d, prefix, ix
    ix.destroy()


def _env(d, prefix, **kw):
    return dict(os.environ, SALT_STUB_PREFIX=prefix, LD_LIBRARY_PATH=str(d / "lib"), **kw)


def _files(case):
    return [os.path.join(LAMBDA, f) for f in (EXTRA_CASES[case][1] if case in EXTRA_CASES else ["reads_pe_1.fq", "reads_pe_2.fq"] if case.startswith("pe") else ["reads_se.fq"])]


def _args(case):
    return EXTRA_CASES[case][0] if case in EXTRA_CASES else read_cases()[case]


def _check_file(data, ix, sam_lines, min_mapq=0, sample=None):
    """FILE = salt_gt_header + the twin's records for the twin's sums over the SAM lines the run printed; the Python statement agrees"""
    import salt_amd
    sums, n = salt_amd.gt_add_sam(ix, sam_lines, min_mapq)
    assert n > 0 and data == salt_amd.gt_header(ix, sample) + salt_amd.gt_text(ix, sums)
    genome = gt_check.Genome()
    py, n_py = gt_check.add_sam(genome, sam_lines, min_mapq)
    assert n_py == n and data == gt_check.header(genome, sample or "sample") + gt_check.text(genome, py)
    return sums


@pytest.mark.parametrize("bam", [False, True])
@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("pipeline", ["text", "host"])
@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_file_equals_header_and_twin_over_the_runs_own_stdout(case, pipeline, gpus, bam, stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    out_file = tmp_path / "calls.vcf"
    base = [str(d / "bin" / "salt")] + _args(case) + ["-t", "8", "--gpus", str(gpus)] + (["--bam"] if bam else [])
    plain = subprocess.run(base + [prefix] + _files(case), capture_output=True, env=env, timeout=300)
    run = subprocess.run(base + ["--genotype", str(out_file), prefix] + _files(case), capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-600:]
    assert (b"host phases" in run.stderr) == (pipeline == "host")
    assert b"summed on the host from the SAM lines" in run.stderr
    if bam:
        (text, lines, _), (text0, lines0, _) = decode_stream(run.stdout), decode_stream(plain.stdout)
        assert lines == lines0 and strip_pg(text) == strip_pg(text0)       # (the @PG line holds the command line)
    else:
        lines = run.stdout
        assert strip_pg(run.stdout) == strip_pg(plain.stdout)
    _check_file(out_file.read_bytes(), ix, lines)


def test_gz_file_min_mapq_sample_name_and_the_other_tallies_beside_it(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    case = "ragged_pe"
    f, fz = tmp_path / "calls.vcf", tmp_path / "calls.vcf.gz"
    side = ["--snp-counts", str(tmp_path / "c.tsv"), "--depth", str(tmp_path / "d.bg"), "--error-profile", str(tmp_path / "e.tsv")]
    alone = subprocess.run([str(d / "bin" / "salt")] + _args(case) + side + [prefix] + _files(case), capture_output=True, env=_env(d, prefix), timeout=300)
    kept = [(tmp_path / n).read_bytes() for n in ("c.tsv", "d.bg", "e.tsv")]
    for out, more in ((f, []), (fz, side)):
        run = subprocess.run([str(d / "bin" / "salt")] + _args(case) + ["--genotype", str(out), "--genotype-min-mapq", "20", "--genotype-sample", "NA12878"] + more +
                             [prefix] + _files(case), capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
        assert run.returncode == 0 and alone.returncode == 0, run.stderr[-600:]
        assert strip_pg(run.stdout) == strip_pg(alone.stdout)
    import salt_amd
    z = fz.read_bytes()
    assert z[:4] == b"\x1f\x8b\x08\x04" and z.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    assert gzip.decompress(z) == f.read_bytes()
    sums = _check_file(f.read_bytes(), ix, run.stdout, 20, "NA12878")
    assert sums[:, :, 0].sum() < salt_amd.gt_add_sam(ix, run.stdout, 0)[0][:, :, 0].sum()
    assert kept == [(tmp_path / n).read_bytes() for n in ("c.tsv", "d.bg", "e.tsv")]       # no byte of any other output changes


def test_every_written_line_counts_once_across_the_hand_over(stub_tree, tmp_path):
    """A multi-line record in the middle of the file: the blocks the text path wrote and the batches of the host pipeline behind them."""
    d, prefix, ix = stub_tree
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq = tmp_path / "mid_multiline.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    f = tmp_path / "calls.vcf"
    res = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["-t", "8", "--gpus", "2", "--genotype", str(f), prefix, str(fq)], capture_output=True,
                         env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    assert strip_pg(res.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert int(_check_file(f.read_bytes(), ix, res.stdout)[:, :, 0].sum()) == 7574


def test_bad_options_exit_1_before_the_index_is_loaded(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt, reads = str(d / "bin" / "salt"), os.path.join(LAMBDA, "reads_se.fq")
    for extra, word in ((["--genotype", str(tmp_path / "c.vcf"), "--genotype-min-mapq", "256"], b"0 to 255"),
                        (["--genotype", str(tmp_path / "c.vcf"), "--genotype-min-mapq", "-1"], b"0 to 255"),
                        (["--genotype", str(tmp_path / "c.vcf"), "--genotype-min-mapq", "2x"], b"0 to 255"),
                        (["--genotype", str(tmp_path / "c.vcf"), "--genotype-sample", "a\tb"], b"sample name"),
                        (["--genotype", str(tmp_path / "c.vcf"), "--genotype-sample", ""], b"sample name"),
                        (["--genotype", str(tmp_path / "no_such_dir" / "c.vcf")], b"cannot open"),
                        (["--genotype", str(tmp_path / "c.vcf"), "--polish"], b"--polish")):
        run = subprocess.run([salt] + extra + [prefix, reads], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 1 and word in run.stderr, run.stderr[-400:]
        assert b"Reload index" not in run.stderr and run.stdout == b""
    usage = subprocess.run([salt, "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    assert b"--genotype " in usage.stderr and b"--genotype-min-mapq" in usage.stderr and b"--genotype-sample" in usage.stderr
