"""`salt --error-profile` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_depth_cli_stub.py.  The stub
has none of the error profile's symbols, so the profile is summed from the SAM lines of every block and batch through the host twin
(salt_errprof_add_sam) and printed by salt_errprof_text: what is tested is the driver -- the options, the file, that every line that is
written counts once on the text path, the host pipeline and across the hand-over between them, with several "devices" -- and that stdout
is what it is without the option."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import errprof_check as ec
from bam_check import decode_stream
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    import salt_amd
    d = tmp_path_factory.mktemp("errprofstub")
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


def _check_file(data, ix, sam_lines, min_mapq=0, full=False):
    """FILE = the text of the tables of the SAM lines the run printed, by the host twin and by the Python statement"""
    import salt_amd
    E, R, n = salt_amd.errprof_add_sam(ix, sam_lines, min_mapq)
    assert n > 0 and data == salt_amd.errprof_text(E, R, min_mapq, full)
    mE, mR, _ = ec.tables_of_sam(ec.lambda_masks(), ec.lambda_offsets(), sam_lines, min_mapq)
    assert data == ec.text_of(mE, mR, min_mapq, full)
    p = ec.parse_file(data)
    assert p["min_mapq"] == min_mapq and np.array_equal(p["R"], mR) and (p["E"] is not None) == full
    return mE


@pytest.mark.parametrize("bam", [False, True])
@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("pipeline", ["text", "host"])
@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_file_equals_the_model_over_the_runs_own_stdout(case, pipeline, gpus, bam, stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    out_file = tmp_path / "errprof.tsv"
    base = [str(d / "bin" / "salt")] + _args(case) + ["-t", "8", "--gpus", str(gpus)] + (["--bam"] if bam else [])
    plain = subprocess.run(base + [prefix] + _files(case), capture_output=True, env=env, timeout=300)
    run = subprocess.run(base + ["--error-profile", str(out_file), prefix] + _files(case), capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-600:]
    assert (b"host phases" in run.stderr) == (pipeline == "host")
    assert b"counted on the host from the SAM lines" in run.stderr and b"MAPQ >= 0" in run.stderr and run.stderr.count(b"[salt] error profile:") == 1
    if bam:
        (text, lines, _), (text0, lines0, _) = decode_stream(run.stdout), decode_stream(plain.stdout)
        assert lines == lines0 and strip_pg(text) == strip_pg(text0)       # (the @PG line holds the command line)
    else:
        lines = run.stdout
        assert strip_pg(run.stdout) == strip_pg(plain.stdout)
    E = _check_file(out_file.read_bytes(), ix, lines)
    golden = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    assert np.array_equal(E, ec.tables_of_sam(ec.lambda_masks(), ec.lambda_offsets(), golden)[0])
    assert (len(np.flatnonzero(E.sum(axis=(0, 1, 3, 4)))), bool(E[1].any())) == ((21, False) if case == "se_default" else (1, True))


def test_full_and_min_mapq(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt = str(d / "bin" / "salt")
    for case, q in (("ragged_pe", 20), ("span_default", 0), ("se_default", 255)):
        f, ff = tmp_path / ("%s.tsv" % case), tmp_path / ("%s_full.tsv" % case)
        extra = ["--error-profile-min-mapq", str(q)]
        run = subprocess.run([salt] + _args(case) + ["--error-profile", str(f)] + extra + [prefix] + _files(case), capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
        full = subprocess.run([salt] + _args(case) + ["--error-profile-full", "--error-profile", str(ff)] + extra + [prefix] + _files(case), capture_output=True,
                              env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
        assert run.returncode == 0 and full.returncode == 0, run.stderr[-600:] + full.stderr[-600:]
        assert strip_pg(run.stdout) == strip_pg(full.stdout) and (b"MAPQ >= %d" % q) in run.stderr
        if q == 255:                                                 # nothing counts: the sections are there, and empty but for R and S
            p = ec.parse_file(ff.read_bytes())
            assert not p["Q"] and not p["C"] and not p["S"].any() and int(p["R"][0, 3]) == 1907 and not p["E"].any()
            continue
        _check_file(f.read_bytes(), ix, run.stdout, q)
        _check_file(ff.read_bytes(), ix, run.stdout, q, True)
        assert ff.read_bytes().startswith(f.read_bytes()) and b"\n#E\t" in ff.read_bytes() and b"\n#E\t" not in f.read_bytes()


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
    f = tmp_path / "e.tsv"
    res = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["-t", "8", "--gpus", "2", "--error-profile", str(f), "--error-profile-full", prefix, str(fq)],
                         capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    assert strip_pg(res.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    E = _check_file(f.read_bytes(), ix, res.stdout, 0, True)
    assert int(E.sum()) == 182760


def test_with_depth_snp_counts_and_bgzf_output_at_the_same_time(stub_tree, tmp_path):
    import gzip
    d, prefix, ix = stub_tree
    f, b, c = tmp_path / "e.tsv", tmp_path / "depth.bed", tmp_path / "counts.tsv"
    run = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["--bgzf", "--error-profile", str(f), "--depth", str(b), "--snp-counts", str(c), prefix] +
                         _files("se_default"), capture_output=True, env=_env(d, prefix), timeout=300)
    assert run.returncode == 0, run.stderr[-600:]
    _check_file(f.read_bytes(), ix, gzip.decompress(run.stdout))
    assert c.read_bytes().count(b"\n") == 3858 + 1 and b.read_bytes().count(b"\n") == 3940


def test_bad_options_exit_1_before_the_index_is_loaded(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt, reads = str(d / "bin" / "salt"), os.path.join(LAMBDA, "reads_se.fq")
    f = str(tmp_path / "e.tsv")
    for extra, word in ((["--error-profile", f, "--error-profile-min-mapq", "256"], b"0 to 255"), (["--error-profile", f, "--error-profile-min-mapq", "-1"], b"0 to 255"),
                        (["--error-profile", f, "--error-profile-min-mapq", "2x"], b"0 to 255"),
                        (["--error-profile", str(tmp_path / "no_such_dir" / "e.tsv")], b"cannot open"),
                        (["--error-profile", f, "--polish"], b"--error-profile with --polish needs a libsalt_gpu")):
        run = subprocess.run([salt] + extra + [prefix, reads], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 1 and word in run.stderr, run.stderr[-400:]
        assert b"Reload index" not in run.stderr and run.stdout == b""
    usage = subprocess.run([salt, "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    assert b"--error-profile <file>" in usage.stderr and b"--error-profile-min-mapq" in usage.stderr and b"--error-profile-full" in usage.stderr
