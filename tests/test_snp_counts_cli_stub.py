"""`salt --snp-counts` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_bam_cli_stub.py.  The stub has no
salt_gpu_index_snp_enable, so the counts come from the SAM lines of every block and batch through the host twin (salt_snp_count_sam): what is
tested is the driver -- the options, the file, that every line that is written is counted once on the text path, the host pipeline and
across the hand-over between them, with several "devices" -- and that stdout is what it is without the option."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import snp_check
from bam_check import decode_stream
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    import salt_amd
    d = tmp_path_factory.mktemp("snpstub")
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


def _genome():
    """the concatenated genome's letters, and [(name, offset)] of its contigs"""
    seq, contigs = [], []
    for line in open(os.path.join(LAMBDA, "genome.fa")):
        if line.startswith(">"):
            contigs.append((line[1:].split()[0], sum(len(s) for s in seq)))
        else:
            seq.append(line.strip().upper())
    return "".join(seq), contigs


def _check_file(path, ix, sam_lines, min_mapq=0):
    """FILE = one line per site in genome order, its counts those of the host twin over the SAM lines the run printed"""
    import salt_amd
    rows, counts = snp_check.parse_counts_file(open(path, "rb").read())
    sites, masks = snp_check.sites_of_ref(os.path.join(LAMBDA, "idx.ref"))
    genome, contigs = _genome()
    want_rows = []
    for g in sites:
        name, off = [c for c in contigs if c[1] <= g][-1]
        want_rows.append((name, int(g) - off + 1, genome[g], "".join("ACGT"[b] for b in range(4) if masks[g] >> b & 1)))
    assert rows == want_rows
    want = salt_amd.snp_count_sam(ix, sam_lines, min_mapq)
    assert np.array_equal(counts, want.astype(np.uint64))
    assert want.sum() > 0
    return counts


@pytest.mark.parametrize("bam", [False, True])
@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("pipeline", ["text", "host"])
@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_file_equals_the_twin_over_the_runs_own_stdout(case, pipeline, gpus, bam, stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    out_file = tmp_path / "counts.tsv"
    base = [str(d / "bin" / "salt")] + _args(case) + ["-t", "8", "--gpus", str(gpus)] + (["--bam"] if bam else [])
    plain = subprocess.run(base + [prefix] + _files(case), capture_output=True, env=env, timeout=300)
    run = subprocess.run(base + ["--snp-counts", str(out_file), prefix] + _files(case), capture_output=True, env=env, timeout=300)
    assert plain.returncode == 0 and run.returncode == 0, run.stderr[-600:]
    assert (b"host phases" in run.stderr) == (pipeline == "host")
    assert b"counted on the host from the SAM lines" in run.stderr
    if bam:
        (text, lines, _), (text0, lines0, _) = decode_stream(run.stdout), decode_stream(plain.stdout)
        assert lines == lines0 and strip_pg(text) == strip_pg(text0)       # (the @PG line holds the command line)
    else:
        lines = run.stdout
        assert strip_pg(run.stdout) == strip_pg(plain.stdout)
    counts = _check_file(out_file, ix, lines)
    golden = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    assert int(counts.sum()) == int(snp_check.count_sam(*_py(ix), golden)[0].sum())


def _py(ix):
    return snp_check.sites_of_ref(os.path.join(LAMBDA, "idx.ref"))[0], snp_check.contig_offsets(os.path.join(LAMBDA, "idx.C.ann"))


def test_min_mapq_and_soft_clips_and_the_contig_boundary(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    for case, q in (("ragged_pe", 20), ("span_default", 0)):
        f = tmp_path / ("%s.tsv" % case)
        run = subprocess.run([str(d / "bin" / "salt")] + _args(case) + ["--snp-counts", str(f), "--snp-min-mapq", str(q), prefix] + _files(case),
                             capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
        assert run.returncode == 0, run.stderr[-600:]
        counts = _check_file(f, ix, run.stdout, q)
        if q:
            import salt_amd
            assert counts.sum() < salt_amd.snp_count_sam(ix, run.stdout, 0).sum()


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
    f = tmp_path / "counts.tsv"
    res = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["-t", "8", "--gpus", "2", "--snp-counts", str(f), prefix, str(fq)], capture_output=True,
                         env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    assert strip_pg(res.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert int(_check_file(f, ix, res.stdout).sum()) == 7574


def test_gzip_input_and_bgzf_output(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    gz = tmp_path / "reads.fq.gz"
    with gzip.open(gz, "wb") as fo:
        fo.write(open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read())
    f = tmp_path / "counts.tsv"
    run = subprocess.run([str(d / "bin" / "salt")] + _args("se_default") + ["--bgzf", "--snp-counts", str(f), prefix, str(gz)], capture_output=True,
                         env=_env(d, prefix), timeout=300)
    assert run.returncode == 0, run.stderr[-600:]
    assert int(_check_file(f, ix, gzip.decompress(run.stdout)).sum()) == 7574


def test_bad_options_exit_1_before_the_index_is_loaded(stub_tree, tmp_path):
    d, prefix, ix = stub_tree
    salt, reads = str(d / "bin" / "salt"), os.path.join(LAMBDA, "reads_se.fq")
    for extra, word in ((["--snp-counts", str(tmp_path / "c.tsv"), "--snp-min-mapq", "256"], b"0 to 255"),
                        (["--snp-counts", str(tmp_path / "c.tsv"), "--snp-min-mapq", "-1"], b"0 to 255"),
                        (["--snp-counts", str(tmp_path / "c.tsv"), "--snp-min-mapq", "2x"], b"0 to 255"),
                        (["--snp-counts", str(tmp_path / "no_such_dir" / "c.tsv")], b"cannot open"),
                        (["--snp-counts", str(tmp_path / "c.tsv"), "--polish"], b"--polish")):
        run = subprocess.run([salt] + extra + [prefix, reads], capture_output=True, env=_env(d, prefix), timeout=300)
        assert run.returncode == 1 and word in run.stderr, run.stderr[-400:]
        assert b"Reload index" not in run.stderr and run.stdout == b""
    usage = subprocess.run([salt, "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    assert b"--snp-counts" in usage.stderr and b"--snp-min-mapq" in usage.stderr
