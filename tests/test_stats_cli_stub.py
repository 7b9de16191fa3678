"""`salt --stats` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_errprof_cli_stub.py.  The stub has
none of the summary's symbols, so the tables are summed from the SAM lines of every block and batch through the host twin
(salt_stats_add_sam) and printed by salt_stats_text: what is tested is the driver -- the options, the file, that every line that is
written counts once on the text path, the host pipeline and across the hand-over between them, with several "devices" -- and that stdout
is what it is without the option."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import stats_check as sc
from bam_check import decode_stream
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    import salt_amd
    d = tmp_path_factory.mktemp("statsstub")
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


def _check_file(data, ix, sam_lines, min_mapq=0):
    """FILE = the text of the tables of the SAM lines the run printed, by the host twin and by the Python statement"""
    import salt_amd
    contigs = sc.lambda_contigs()
    cells, ct, n = salt_amd.stats_add_sam(ix, sam_lines, min_mapq)
    assert data == salt_amd.stats_text(ix, cells, ct, min_mapq)
    m_cells, m_ct, m_n = sc.tables_of_sam(contigs, sam_lines, min_mapq)
    assert data == sc.text_of(contigs, m_cells, m_ct, min_mapq) and n == m_n
    p = sc.parse_file(data)
    assert p["min_mapq"] == min_mapq and np.array_equal(p["cells"], m_cells) and np.array_equal(p["ct"], m_ct)
    return sc.split(m_cells), m_ct


@pytest.mark.parametrize("bam", [False, True])
@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("pipeline", ["text", "host"])
@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_file_equals_the_model_over_the_runs_own_stdout(case, pipeline, gpus, bam, stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    out_file = tmp_path / "stats.tsv"
    base = [str(d / "bin" / "salt")] + _args(case) + ["-t", "8", "--gpus", str(gpus)] + (["--bam"] if bam else [])
    plain = subprocess.run(base + [prefix] + _files(case), capture_output=True, env=env, timeout=300)
    run = subprocess.run(base + ["--stats", str(out_file), prefix] + _files(case), capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-600:]
    assert (b"host phases" in run.stderr) == (pipeline == "host")
    assert b"counted on the host from the SAM lines" in run.stderr and b"MAPQ >= 0" in run.stderr and run.stderr.count(b"[salt] stats:") == 1 and b"[salt] stats:" not in plain.stderr
    if bam:
        (text, lines, _), (text0, lines0, _) = decode_stream(run.stdout), decode_stream(plain.stdout)
        assert lines == lines0 and strip_pg(text) == strip_pg(text0)       # (the @PG line holds the command line)
    else:
        lines = run.stdout
        assert strip_pg(run.stdout) == strip_pg(plain.stdout)
    T, ct = _check_file(out_file.read_bytes(), ix, lines)
    golden = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    g_cells, g_ct, _ = sc.tables_of_sam(sc.lambda_contigs(), golden)
    assert np.array_equal(np.concatenate([T[k].reshape(-1) for k in ("SN", "MQ", "RL", "GC", "XA", "IS", "OR", "ID")]), g_cells) and np.array_equal(ct, g_ct)
    assert (int(T["SN"][0, 0]), int(T["SN"][1, 0]), bool(T["IS"].any())) == ((2000, 0, False) if case == "se_default" else (1000, 1000, True))
    assert (b"\nSN\t1\t" in out_file.read_bytes()) == (case == "pe_default")


def test_min_mapq(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt = str(d / "bin" / "salt")
    for case, q in (("ragged_pe", 20), ("span_default", 0), ("se_default", 255)):
        f = tmp_path / ("%s.tsv" % case)
        run = subprocess.run([salt] + _args(case) + ["--stats", str(f), "--stats-min-mapq", str(q), prefix] + _files(case), capture_output=True,
                             env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
        assert run.returncode == 0, run.stderr[-600:]
        assert (b"MAPQ >= %d" % q) in run.stderr
        T, ct = _check_file(f.read_bytes(), ix, run.stdout, q)
        if q == 255:                                                 # nothing counts: every mapped record is below the floor
            assert int(T["SN"][0, 3]) == 1907 and not T["SN"][0, 4:11].any() and not T["SN"][0, 12:].any() and int(T["MQ"].sum()) == 1907 and not ct[:, 2:].any()


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
    f = tmp_path / "s.tsv"
    res = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["-t", "8", "--gpus", "2", "--stats", str(f), prefix, str(fq)],
                         capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    assert strip_pg(res.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    T, ct = _check_file(f.read_bytes(), ix, res.stdout)
    assert int(T["SN"][0, 0]) == 2000 and int(T["SN"][0, 4]) == 1907 and int(T["SN"][0, 11]) == 200000


def test_with_depth_and_bgzf_output_at_the_same_time(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    f, b = tmp_path / "s.tsv", tmp_path / "depth.bed"
    run = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["--bgzf", "--stats", str(f), "--depth", str(b), prefix] +
                         _files("se_default"), capture_output=True, env=_env(d, prefix), timeout=300)
    assert run.returncode == 0, run.stderr[-600:]
    _check_file(f.read_bytes(), ix, gzip.decompress(run.stdout))
    assert b.read_bytes().count(b"\n") == 3940


def test_bad_options_exit_1_before_the_index_is_loaded(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt, reads = str(d / "bin" / "salt"), os.path.join(LAMBDA, "reads_se.fq")
    f = str(tmp_path / "s.tsv")
    for extra, word in ((["--stats", f, "--stats-min-mapq", "256"], b"0 to 255"), (["--stats", f, "--stats-min-mapq", "-1"], b"0 to 255"),
                        (["--stats", f, "--stats-min-mapq", "2x"], b"0 to 255"),
                        (["--stats", str(tmp_path / "no_such_dir" / "s.tsv")], b"cannot open"),
                        (["--stats", f, "--polish"], b"--stats with --polish needs a libsalt_gpu")):
        run = subprocess.run([salt] + extra + [prefix, reads], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 1 and word in run.stderr, run.stderr[-400:]
        assert b"Reload index" not in run.stderr and run.stdout == b""
    usage = subprocess.run([salt, "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    assert b"--stats <file>" in usage.stderr and b"--stats-min-mapq" in usage.stderr
