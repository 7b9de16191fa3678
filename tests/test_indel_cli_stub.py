"""`salt --indels` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_discover_cli_stub.py.  The stub has
no salt_gpu_index_indel_enable, so the table comes from the SAM lines of every block and batch through the host twin (salt_indel_add_sam)
and the records from salt_indel_text: what is tested is the driver -- the options, the file (plain and .gz), that every line that is
written is counted once on the text path, the host pipeline and across the hand-over between them, with several "devices" -- and that
stdout and the other tallies' files are what they are without the option."""
import gzip
import os
import shutil
import subprocess

import pytest

import gap_cases
import indel_check
from bam_check import decode_stream
from bgzf_check import strip_pg
from conftest import LAMBDA, ROOT

LOOSE = ["--indels-min-mapq", "0", "--indels-min-alt", "1", "--indels-min-pct", "0"]      # the goldens are shallow: over 1 000 records this way
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    import salt_amd
    d = tmp_path_factory.mktemp("indelstub")
    os.makedirs(d / "bin"); os.makedirs(d / "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "salt_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    shutil.copy(os.path.join(ROOT, "salt_amd", "bin", "salt"), d / "bin" / "salt")
    shutil.copy(os.path.join(ROOT, "salt_amd", "lib", "libsalt_host.so"), d / "lib" / "libsalt_host.so")
    subprocess.run(["gcc", "-O2", "-g", "-fPIC", "-shared", "-Wall", "-o", str(d / "lib" / "libsalt_gpu.so"),
                    os.path.join(ROOT, "tests", "stub", "salt_gpu_stub.c"), os.path.join(ROOT, "oracle", "salt_oracle.c"), "-lm", "-lpthread"], check=True)
    prefix = str(d / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    reads = {c: gap_cases.plain_paths(c, d) for c in ("gap_se_mid", "gap_pe_short")}
    ix = salt_amd.Index.reload(prefix)
    yield d, prefix, ix, indel_check.Genome(), reads
    ix.destroy()


def _env(d, prefix, **kw):
    return dict(os.environ, SALT_STUB_PREFIX=prefix, LD_LIBRARY_PATH=str(d / "lib"), **kw)


def _check_file(data, ix, genome, sam_lines, min_mapq=20, min_alt=3, min_pct=20):
    """FILE = the header and the twin's records for the twin's table over the SAM lines the run printed; the Python statement agrees"""
    import salt_amd
    entries, diff, stats, n = salt_amd.indel_add_sam(ix, sam_lines, min_mapq)
    assert n > 0 and data == salt_amd.indel_header(ix, min_mapq, min_alt, min_pct, 0) + salt_amd.indel_text(ix, entries, diff, min_alt, min_pct)
    table, py_stats, py_diff, n_py = indel_check.add_sam(genome, sam_lines, min_mapq)
    assert n_py == n and py_stats == stats.tolist()
    assert data == indel_check.header(genome, min_mapq, min_alt, min_pct, 0) + indel_check.text(genome, indel_check.entries(table), py_diff, min_alt, min_pct)
    return indel_check.parse(data), stats.tolist()


@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("pipeline", ["text", "host"])
@pytest.mark.parametrize("case", ["gap_se_mid", "gap_pe_short"])
def test_file_equals_the_twin_over_the_runs_own_stdout(case, pipeline, gpus, stub_tree, tmp_path):
    d, prefix, ix, genome, reads = stub_tree
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    out_file = tmp_path / "indels.vcf"
    bam = gpus == 3                                                    # --bam on half of the cases
    base = [str(d / "bin" / "salt")] + gap_cases.GAP_CASES[case][0] + ["-t", "8", "--gpus", str(gpus)] + (["--bam"] if bam else [])
    plain = subprocess.run(base + [prefix] + reads[case], capture_output=True, env=env, timeout=300)
    run = subprocess.run(base + ["--indels", str(out_file)] + LOOSE + [prefix] + reads[case], capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-600:]
    assert (b"host phases" in run.stderr) == (pipeline == "host")
    assert b"tabled on the host from the SAM lines" in run.stderr and b"WARNING" not in run.stderr
    if bam:
        (text, lines, _), (text0, lines0, _) = decode_stream(run.stdout), decode_stream(plain.stdout)
        assert lines == lines0 and strip_pg(text) == strip_pg(text0)       # (the @PG line holds the command line)
    else:
        lines = run.stdout
        assert strip_pg(run.stdout) == strip_pg(plain.stdout) == gap_cases.golden(case)
    rows, stats = _check_file(out_file.read_bytes(), ix, genome, lines, 0, 1, 0)
    assert (len(rows), stats) == ((1200, [1220, 0, 0, 155]) if case == "gap_se_mid" else (358, [358, 0, 0, 22]))
    assert b"tabled %d, dropped 0, long 0, unanchored %d" % (stats[0], stats[3]) in run.stderr


def test_gz_the_defaults_and_the_other_tallies_beside_it(stub_tree, tmp_path):
    d, prefix, ix, genome, reads = stub_tree
    case = "gap_se_mid"
    f, fz = tmp_path / "indels.vcf", tmp_path / "indels.vcf.gz"
    side = ["--snp-counts", str(tmp_path / "c.tsv"), "--depth", str(tmp_path / "d.bg"), "--error-profile", str(tmp_path / "e.tsv"), "--genotype", str(tmp_path / "g.vcf"),
            "--discover", str(tmp_path / "f.txt"), "--discover-min-alt", "1", "--discover-min-pct", "0", "--stats", str(tmp_path / "s.tsv")]
    names = ("c.tsv", "d.bg", "e.tsv", "g.vcf", "f.txt", "s.tsv")
    salt = [str(d / "bin" / "salt")] + gap_cases.GAP_CASES[case][0]
    alone = subprocess.run(salt + side + [prefix] + reads[case], capture_output=True, env=_env(d, prefix), timeout=300)
    kept = [(tmp_path / n).read_bytes() for n in names]
    assert all(len(k) > 100 for k in kept)
    for out, more in ((f, []), (fz, side)):
        run = subprocess.run(salt + ["--indels", str(out), "--indels-min-alt", "2", "--indels-min-pct", "10", "--indels-slots", "1024"] + more + [prefix] + reads[case],
                             capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
        assert run.returncode == 0 and alone.returncode == 0, run.stderr[-600:]
        assert strip_pg(run.stdout) == strip_pg(alone.stdout)
        assert b"MAPQ >= 20, min_alt 2, min_pct 10," in run.stderr
    z = fz.read_bytes()
    assert z[:4] == b"\x1f\x8b\x08\x04" and z.endswith(BGZF_EOF)
    assert gzip.decompress(z) == f.read_bytes()
    rows, _ = _check_file(f.read_bytes(), ix, genome, run.stdout, 20, 2, 10)
    assert len(rows) >= 10 and all(r[4]["AO"] >= 2 for r in rows)
    assert kept == [(tmp_path / n).read_bytes() for n in names]            # no byte of any other output changes
    # the defaults: on this shallow golden a handful of alleles are seen three times or more
    run = subprocess.run(salt + ["--indels", str(f), prefix] + reads[case], capture_output=True, env=_env(d, prefix), timeout=300)
    rows, _ = _check_file(f.read_bytes(), ix, genome, run.stdout)
    assert run.returncode == 0 and b"MAPQ >= 20, min_alt 3, min_pct 20," in run.stderr and 1 <= len(rows) < 10


def test_every_written_line_counts_once_across_the_hand_over(stub_tree, tmp_path):
    """A multi-line record in the middle of the file: the blocks the text path wrote and the batches of the host pipeline behind them."""
    d, prefix, ix, genome, reads = stub_tree
    recs = open(reads["gap_se_mid"][0], "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1000 else r      # (behind the 256 KiB the driver looks at before it chooses the text path)
    fq = tmp_path / "mid_multiline.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    f = tmp_path / "indels.vcf"
    res = subprocess.run([str(d / "bin" / "salt")] + gap_cases.GAP_CASES["gap_se_mid"][0] + ["-t", "8", "--gpus", "2", "--indels", str(f)] + LOOSE + [prefix, str(fq)],
                         capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    assert strip_pg(res.stdout) == gap_cases.golden("gap_se_mid")
    rows, stats = _check_file(f.read_bytes(), ix, genome, res.stdout, 0, 1, 0)
    assert stats == [1220, 0, 0, 155] and sum(r[4]["AO"] for r in rows) == 1220


def test_bad_options_exit_1_before_the_index_is_loaded(stub_tree, tmp_path):
    d, prefix, ix, genome, reads = stub_tree
    salt, fq = str(d / "bin" / "salt"), os.path.join(LAMBDA, "reads_se.fq")
    on = ["--indels", str(tmp_path / "c.vcf")]
    for extra, word in ((on + ["--indels-min-mapq", "256"], b"0 to 255"), (on + ["--indels-min-mapq", "-1"], b"0 to 255"), (on + ["--indels-min-mapq", "2x"], b"0 to 255"),
                        (on + ["--indels-min-alt", "0"], b"1 to 4294967295"), (on + ["--indels-min-alt", "4294967296"], b"1 to 4294967295"), (on + ["--indels-min-alt", "3.5"], b"1 to 4294967295"),
                        (on + ["--indels-min-pct", "101"], b"0 to 100"), (on + ["--indels-min-pct", "-5"], b"0 to 100"), (on + ["--indels-min-pct", "x"], b"0 to 100"),
                        (on + ["--indels-slots", "32"], b"power of two"), (on + ["--indels-slots", "1000"], b"power of two"), (on + ["--indels-slots", "536870912"], b"power of two"),
                        (on + ["--indels-slots", "0"], b"power of two"), (on + ["--indels-slots", "64k"], b"power of two"), (on + ["--indels-slots", "-64"], b"power of two"),
                        (["--indels", str(tmp_path / "no_such_dir" / "c.vcf")], b"cannot open"),
                        (on + ["--polish"], b"--polish")):
        run = subprocess.run([salt] + extra + [prefix, fq], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 1 and word in run.stderr, (extra, run.stderr[-400:])
        assert b"Reload index" not in run.stderr and run.stdout == b""
    for slots in ("64", "268435456"):                                  # the ends of the range are taken
        run = subprocess.run([salt, "-d", "-c"] + on + ["--indels-slots", slots, prefix, fq], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 0, run.stderr[-400:]
    usage = subprocess.run([salt, "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    for word in (b"--indels ", b"--indels-min-mapq", b"--indels-min-alt", b"--indels-min-pct", b"--indels-slots"):
        assert word in usage.stderr
