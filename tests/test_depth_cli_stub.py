"""`salt --depth` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_snp_counts_cli_stub.py.  The stub has no
salt_gpu_index_depth_enable, so the coverage is summed from the SAM lines of every block and batch through the host twin
(salt_depth_add_sam) and printed by salt_depth_text: what is tested is the driver -- the options, the file, that every line that is
written counts once on the text path, the host pipeline and across the hand-over between them, with several "devices" -- and that stdout
is what it is without the option."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_check
from bam_check import decode_stream
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    import salt_amd
    d = tmp_path_factory.mktemp("depthstub")
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


def _check_file(data, ix, sam_lines, min_mapq=0, window=0):
    """FILE = the text of the difference array of the SAM lines the run printed, by the host twin and by the Python statement"""
    import salt_amd
    diff, n = salt_amd.depth_add_sam(ix, sam_lines, min_mapq)
    assert n > 0 and data == salt_amd.depth_text(ix, diff, window)
    assert data == depth_check.text_of(depth_check.lambda_contigs(), depth_check.diff_of_sam(depth_check.lambda_contigs(), sam_lines, min_mapq)[0], window)
    return diff


@pytest.mark.parametrize("bam", [False, True])
@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("pipeline", ["text", "host"])
@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_file_equals_the_twin_over_the_runs_own_stdout(case, pipeline, gpus, bam, stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    out_file = tmp_path / "depth.bed"
    base = [str(d / "bin" / "salt")] + _args(case) + ["-t", "8", "--gpus", str(gpus)] + (["--bam"] if bam else [])
    plain = subprocess.run(base + [prefix] + _files(case), capture_output=True, env=env, timeout=300)
    run = subprocess.run(base + ["--depth", str(out_file), prefix] + _files(case), capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-600:]
    assert (b"host phases" in run.stderr) == (pipeline == "host")
    assert b"summed on the host from the SAM lines" in run.stderr and b"MAPQ >= 0" in run.stderr
    if bam:
        (text, lines, _), (text0, lines0, _) = decode_stream(run.stdout), decode_stream(plain.stdout)
        assert lines == lines0 and strip_pg(text) == strip_pg(text0)       # (the @PG line holds the command line)
    else:
        lines = run.stdout
        assert strip_pg(run.stdout) == strip_pg(plain.stdout)
    diff = _check_file(out_file.read_bytes(), ix, lines)
    golden = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    assert np.array_equal(diff, depth_check.diff_of_sam(depth_check.lambda_contigs(), golden)[0])


def test_window_min_mapq_gz_and_the_contig_boundary(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt = str(d / "bin" / "salt")
    for case, q in (("ragged_pe", 20), ("span_default", 0)):
        texts = {}
        for w in (0, 1000):
            f, fz = tmp_path / ("%s_%d.bed" % (case, w)), tmp_path / ("%s_%d.bed.gz" % (case, w))
            extra = ["--depth-min-mapq", str(q)] + (["--depth-window", str(w)] if w else [])
            run = subprocess.run([salt] + _args(case) + ["--depth", str(f)] + extra + [prefix] + _files(case), capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
            gz = subprocess.run([salt] + _args(case) + ["--depth", str(fz)] + extra + [prefix] + _files(case), capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
            assert run.returncode == 0 and gz.returncode == 0, run.stderr[-600:] + gz.stderr[-600:]
            assert strip_pg(run.stdout) == strip_pg(gz.stdout) and (b"MAPQ >= %d" % q) in run.stderr and (b"windows of 1000" in run.stderr) == (w == 1000)
            texts[w] = f.read_bytes()
            _check_file(texts[w], ix, run.stdout, q, w)
            z = fz.read_bytes()
            assert z[:4] == b"\x1f\x8b\x08\x04" and z.endswith(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 66, 67, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))
            assert gzip.decompress(z) == texts[w]                    # FILE.gz decompresses to the plain FILE's bytes
        if case == "span_default":
            assert b"\t48502\t37\nlambdaB_div2pct\t0\t" in texts[0]     # cut at the contig's end at equal depth
            assert texts[1000].count(b"\n") == 2 * 49 and b"lambdaA\t48000\t48502\t" in texts[1000]


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
    f = tmp_path / "depth.bed"
    res = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["-t", "8", "--gpus", "2", "--depth", str(f), prefix, str(fq)], capture_output=True,
                         env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    assert strip_pg(res.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    data = f.read_bytes()
    _check_file(data, ix, res.stdout)
    assert data.count(b"\n") == 3940


def test_with_snp_counts_and_bgzf_output_at_the_same_time(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    f, c = tmp_path / "depth.bed", tmp_path / "counts.tsv"
    run = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["--bgzf", "--depth", str(f), "--snp-counts", str(c), prefix] + _files("se_default"),
                         capture_output=True, env=_env(d, prefix), timeout=300)
    assert run.returncode == 0, run.stderr[-600:]
    _check_file(f.read_bytes(), ix, gzip.decompress(run.stdout))
    assert c.read_bytes().count(b"\n") == 3858 + 1


def test_bad_options_exit_1_before_the_index_is_loaded(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt, reads = str(d / "bin" / "salt"), os.path.join(LAMBDA, "reads_se.fq")
    f = str(tmp_path / "d.bed")
    for extra, word in ((["--depth", f, "--depth-min-mapq", "256"], b"0 to 255"), (["--depth", f, "--depth-min-mapq", "-1"], b"0 to 255"),
                        (["--depth", f, "--depth-min-mapq", "2x"], b"0 to 255"), (["--depth", f, "--depth-window", "0"], b"from 1 to"),
                        (["--depth", f, "--depth-window", "-5"], b"from 1 to"), (["--depth", f, "--depth-window", "4294967296"], b"from 1 to"),
                        (["--depth", f, "--depth-window", "1k"], b"from 1 to"), (["--depth", str(tmp_path / "no_such_dir" / "d.bed")], b"cannot open"),
                        (["--depth", f, "--polish"], b"--polish")):
        run = subprocess.run([salt] + extra + [prefix, reads], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 1 and word in run.stderr, run.stderr[-400:]
        assert b"Reload index" not in run.stderr and run.stdout == b""
    usage = subprocess.run([salt, "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    assert b"--depth " in usage.stderr and b"--depth-min-mapq" in usage.stderr and b"--depth-window" in usage.stderr
