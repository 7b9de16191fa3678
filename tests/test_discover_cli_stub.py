"""`salt --discover` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_genotype_cli_stub.py.  The stub
has no salt_gpu_index_disc_enable, so the arrays come from the SAM lines of every block and batch through the host twin
(salt_disc_add_sam) and the lines from salt_disc_text: what is tested is the driver -- the options, the file (plain and .gz), that every
line that is written is counted once on the text path, the host pipeline and across the hand-over between them, with several "devices",
the warning for a contig without a line -- and that stdout and the other tallies' files are what they are without the option."""
import gzip
import os
import shutil
import subprocess

import pytest

import disc_check
from bam_check import decode_stream
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases

LOOSE = ["--discover-min-mapq", "0", "--discover-min-baseq", "0", "--discover-min-alt", "1", "--discover-min-pct", "0"]      # the goldens are shallow: over 1 000 lines this way


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    import salt_amd
    d = tmp_path_factory.mktemp("discstub")
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
    yield d, prefix, ix, disc_check.Genome()
    ix.destroy()


def _env(d, prefix, **kw):
    return dict(os.environ, SALT_STUB_PREFIX=prefix, LD_LIBRARY_PATH=str(d / "lib"), **kw)


def _files(case):
    return [os.path.join(LAMBDA, f) for f in (EXTRA_CASES[case][1] if case in EXTRA_CASES else ["reads_pe_1.fq", "reads_pe_2.fq"] if case.startswith("pe") else ["reads_se.fq"])]


def _args(case):
    return EXTRA_CASES[case][0] if case in EXTRA_CASES else read_cases()[case]


def _check_file(data, ix, genome, sam_lines, min_mapq=20, min_baseq=20, min_alt=3, min_pct=20, all_sites=False):
    """FILE = the twin's lines for the twin's arrays over the SAM lines the run printed; the Python statement agrees"""
    import salt_amd
    alt, diff, n = salt_amd.disc_add_sam(ix, sam_lines, min_mapq, min_baseq)
    assert n > 0 and data == salt_amd.disc_text(ix, alt, diff, min_alt, min_pct, all_sites)
    py_alt, py_diff, n_py = disc_check.add_sam(genome, sam_lines, min_mapq, min_baseq)
    assert n_py == n and data == disc_check.text(genome, py_alt, py_diff, min_alt, min_pct, all_sites)
    return disc_check.parse(data)


@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("pipeline", ["text", "host"])
@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_file_equals_the_twin_over_the_runs_own_stdout(case, pipeline, gpus, stub_tree, tmp_path):
    d, prefix, ix, genome = stub_tree
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    out_file = tmp_path / "found.txt"
    bam = gpus == 3                                                    # --bam on half of the cases
    base = [str(d / "bin" / "salt")] + _args(case) + ["-t", "8", "--gpus", str(gpus)] + (["--bam"] if bam else [])
    plain = subprocess.run(base + [prefix] + _files(case), capture_output=True, env=env, timeout=300)
    run = subprocess.run(base + ["--discover", str(out_file)] + LOOSE + [prefix] + _files(case), capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-600:]
    assert (b"host phases" in run.stderr) == (pipeline == "host")
    assert b"counted on the host from the SAM lines" in run.stderr and b"have no line" not in run.stderr
    if bam:
        (text, lines, _), (text0, lines0, _) = decode_stream(run.stdout), decode_stream(plain.stdout)
        assert lines == lines0 and strip_pg(text) == strip_pg(text0)       # (the @PG line holds the command line)
    else:
        lines = run.stdout
        assert strip_pg(run.stdout) == strip_pg(plain.stdout)
    rows = _check_file(out_file.read_bytes(), ix, genome, lines, 0, 0, 1, 0)
    assert len(rows) == (1230 if case == "se_default" else 951)


def test_gz_all_the_defaults_and_the_other_tallies_beside_it(stub_tree, tmp_path):
    d, prefix, ix, genome = stub_tree
    case = "ragged_pe"
    f, fz = tmp_path / "found.txt", tmp_path / "found.txt.gz"
    side = ["--snp-counts", str(tmp_path / "c.tsv"), "--depth", str(tmp_path / "d.bg"), "--error-profile", str(tmp_path / "e.tsv"), "--genotype", str(tmp_path / "g.vcf")]
    names = ("c.tsv", "d.bg", "e.tsv", "g.vcf")
    alone = subprocess.run([str(d / "bin" / "salt")] + _args(case) + side + [prefix] + _files(case), capture_output=True, env=_env(d, prefix), timeout=300)
    kept = [(tmp_path / n).read_bytes() for n in names]
    for out, more in ((f, []), (fz, side)):
        run = subprocess.run([str(d / "bin" / "salt")] + _args(case) + ["--discover", str(out), "--discover-all", "--discover-min-alt", "2", "--discover-min-pct", "10"] + more +
                             [prefix] + _files(case), capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
        assert run.returncode == 0 and alone.returncode == 0, run.stderr[-600:]
        assert strip_pg(run.stdout) == strip_pg(alone.stdout)
        assert b"MAPQ >= 20, base quality >= 20, min_alt 2, min_pct 10, all sites" in run.stderr and b"have no line" not in run.stderr
    z = fz.read_bytes()
    assert z[:4] == b"\x1f\x8b\x08\x04" and z.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    assert gzip.decompress(z) == f.read_bytes()
    rows = _check_file(f.read_bytes(), ix, genome, run.stdout, 20, 20, 2, 10, True)
    assert len(rows) >= len(genome.sites)                                  # a whole SNP file: every site of the index has its line
    assert kept == [(tmp_path / n).read_bytes() for n in names]            # no byte of any other output changes


def test_the_defaults_find_nothing_in_a_shallow_run_and_say_which_contig_has_no_line(stub_tree, tmp_path):
    d, prefix, ix, genome = stub_tree
    f = tmp_path / "found.txt"
    run = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["--discover", str(f), prefix] + _files("se_default"), capture_output=True, env=_env(d, prefix),
                         timeout=300)
    assert run.returncode == 0, run.stderr[-600:]
    assert _check_file(f.read_bytes(), ix, genome, run.stdout) == [] and f.read_bytes() == b""
    assert b"2 of 2 contigs have no line" in run.stderr and b"the first is lambdaA:" in run.stderr and b"MAPQ >= 20, base quality >= 20, min_alt 3, min_pct 20," in run.stderr


def test_every_written_line_counts_once_across_the_hand_over(stub_tree, tmp_path):
    """A multi-line record in the middle of the file: the blocks the text path wrote and the batches of the host pipeline behind them."""
    d, prefix, ix, genome = stub_tree
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq = tmp_path / "mid_multiline.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    f = tmp_path / "found.txt"
    res = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["-t", "8", "--gpus", "2", "--discover", str(f)] + LOOSE + [prefix, str(fq)], capture_output=True,
                         env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    assert strip_pg(res.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    rows = _check_file(f.read_bytes(), ix, genome, res.stdout, 0, 0, 1, 0)
    assert sum(sum(x for x in r[5] if x is not None) for r in rows) == 1243


def test_bad_options_exit_1_before_the_index_is_loaded(stub_tree, tmp_path):
    d, prefix, ix, genome = stub_tree
    salt, reads = str(d / "bin" / "salt"), os.path.join(LAMBDA, "reads_se.fq")
    on = ["--discover", str(tmp_path / "c.txt")]
    for extra, word in ((on + ["--discover-min-mapq", "256"], b"0 to 255"), (on + ["--discover-min-mapq", "-1"], b"0 to 255"), (on + ["--discover-min-mapq", "2x"], b"0 to 255"),
                        (on + ["--discover-min-baseq", "94"], b"0 to 93"), (on + ["--discover-min-baseq", "-1"], b"0 to 93"), (on + ["--discover-min-baseq", ""], b"0 to 93"),
                        (on + ["--discover-min-alt", "0"], b"1 to 2097151"), (on + ["--discover-min-alt", "2097152"], b"1 to 2097151"), (on + ["--discover-min-alt", "3.5"], b"1 to 2097151"),
                        (on + ["--discover-min-pct", "101"], b"0 to 100"), (on + ["--discover-min-pct", "-5"], b"0 to 100"), (on + ["--discover-min-pct", "x"], b"0 to 100"),
                        (["--discover", str(tmp_path / "no_such_dir" / "c.txt")], b"cannot open"),
                        (on + ["--polish"], b"--polish")):
        run = subprocess.run([salt] + extra + [prefix, reads], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 1 and word in run.stderr, run.stderr[-400:]
        assert b"Reload index" not in run.stderr and run.stdout == b""
    usage = subprocess.run([salt, "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    for word in (b"--discover ", b"--discover-min-mapq", b"--discover-min-baseq", b"--discover-min-alt", b"--discover-min-pct", b"--discover-all", b"the only tally"):
        assert word in usage.stderr
