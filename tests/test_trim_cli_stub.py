"""`salt --trim-*` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_bam_cli_stub.py.  The stub has no trim
kernel, so the whole run goes through the host pipeline, whose parser trims with the host twin (salt_trim_span) -- and stdout must be, the
@PG line apart, what `salt` without the options prints for the FASTQ that salt_amd.trim_fastq trimmed beforehand, which takes the text
path.  The adapter-carrying reads are built here, seeded, from the golden reads (trim_check.constructed)."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import salt_amd
import trim_check as tc
from bam_check import decode_stream
from bgzf_check import stream_text, strip_pg
from conftest import LAMBDA, ROOT, read_cases

TRIM = tc.opts(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2, qual=20)
TRIM_ARGS = ["--trim-adapter", tc.ADAPTER, "--trim-adapter2", tc.ADAPTER2, "--trim-qual", "20"]


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("trimstub")
    os.makedirs(d / "bin"); os.makedirs(d / "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "salt_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    shutil.copy(os.path.join(ROOT, "salt_amd", "bin", "salt"), d / "bin" / "salt")
    shutil.copy(os.path.join(ROOT, "salt_amd", "lib", "libsalt_host.so"), d / "lib" / "libsalt_host.so")
    subprocess.run(["gcc", "-O2", "-g", "-fPIC", "-shared", "-Wall", "-o", str(d / "lib" / "libsalt_gpu.so"),
                    os.path.join(ROOT, "tests", "stub", "salt_gpu_stub.c"), os.path.join(ROOT, "oracle", "salt_oracle.c"), "-lm", "-lpthread"], check=True)
    prefix = str(d / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return d, prefix


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """the constructed files and their pre-trimmed copies: name -> path; "counts_se" / "counts_pe": the twin's counters"""
    d = tmp_path_factory.mktemp("trimreads")
    out = {}
    c_se, c_pe = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
    for name, src, ad, seed, mate, counts in (("se", "reads_se.fq", tc.ADAPTER, 1, 0, c_se), ("pe1", "reads_pe_1.fq", tc.ADAPTER, 2, 0, c_pe), ("pe2", "reads_pe_2.fq", tc.ADAPTER2, 3, 1, c_pe)):
        raw = tc.constructed(src, ad, seed)
        out[name], out[name + "_t"] = str(d / (name + ".fq")), str(d / (name + "_trimmed.fq"))
        open(out[name], "wb").write(raw)
        open(out[name + "_t"], "wb").write(salt_amd.trim_fastq(raw, mate, counts=counts, **TRIM))
    out["counts_se"], out["counts_pe"] = c_se, c_pe
    return out


def _env(d, prefix, **kw):
    return dict(os.environ, SALT_STUB_PREFIX=prefix, LD_LIBRARY_PATH=str(d / "lib"), **kw)


def _salt(d, prefix, args, files, **env):
    p = subprocess.run([str(d / "bin" / "salt")] + args + [prefix] + files, capture_output=True, env=_env(d, prefix, **env), timeout=300)
    assert p.returncode == 0, (args, p.stderr[-600:])
    return p


def _files(reads, case, trimmed):
    t = "_t" if trimmed else ""
    return [reads["se" + t]] if case == "se_default" else [reads["pe1" + t], reads["pe2" + t]]


def _text(stdout, fmt):
    """what the stream says, without the @PG line"""
    if fmt == "plain":
        return strip_pg(stdout)
    if fmt == "bgzf":
        return strip_pg(stream_text(stdout))
    text, lines, _ = decode_stream(stdout)
    return strip_pg(text), lines


def counters(stderr):
    """the [salt] trim: line -> (who trimmed, (2, 8) array in trim_check.COUNTERS' order)"""
    lines = [l for l in stderr.decode().split("\n") if l.startswith("[salt] trim: ") and "mate 1" in l]
    assert len(lines) == 1, stderr[-800:]
    who = lines[0][len("[salt] trim: "):].split(":")[0]
    c = np.zeros((2, 8), dtype=np.uint64)
    for m, part in enumerate(lines[0].split("mate ")[1:]):
        got = dict(re.findall(r"(\w+) (\d+)", part.split(":", 1)[1]))
        c[m] = [int(got[k]) for k in tc.COUNTERS]
        assert int(got["reads_clipped"]) == 0
    return who, c


@pytest.mark.parametrize("gpus", [1, 3])
@pytest.mark.parametrize("fmt", ["plain", "bam", "bgzf"])
@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_stdout_is_the_run_on_the_pretrimmed_reads(case, fmt, gpus, stub_tree, reads):
    d, prefix = stub_tree
    args = read_cases()[case] + ["-t", "8", "--gpus", str(gpus)] + ([] if fmt == "plain" else ["--" + fmt])
    want = _salt(d, prefix, args, _files(reads, case, True), SALT_CHUNK_BYTES="9000")
    got = _salt(d, prefix, args + TRIM_ARGS, _files(reads, case, False), SALT_CHUNK_BYTES="9000")
    assert _text(got.stdout, fmt) == _text(want.stdout, fmt) and len(got.stdout) > 50000
    assert b"text path" in want.stderr and b"[salt] trim:" not in want.stderr
    assert b"the whole run goes through the host pipeline" in got.stderr and b"text path" not in got.stderr
    who, c = counters(got.stderr)
    assert who == "host" and (c == reads["counts_se" if case == "se_default" else "counts_pe"]).all()


def test_a_multi_line_record_in_the_middle_and_gzip_input(stub_tree, reads, tmp_path):
    d, prefix = stub_tree
    args = read_cases()["se_default"] + ["-t", "8"]
    want = strip_pg(_salt(d, prefix, args, [reads["se_t"]]).stdout)
    recs = open(reads["se"], "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq = tmp_path / "mid_multiline.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    got = _salt(d, prefix, args + TRIM_ARGS, [str(fq)], SALT_CHUNK_BYTES="9000")
    assert strip_pg(got.stdout) == want
    assert (counters(got.stderr)[1] == reads["counts_se"]).all()
    gz = tmp_path / "reads.fq.gz"
    with gzip.open(gz, "wb") as f:
        f.write(open(reads["se"], "rb").read())
    got = _salt(d, prefix, args + TRIM_ARGS, [str(gz)])
    assert strip_pg(got.stdout) == want and (counters(got.stderr)[1] == reads["counts_se"]).all()


@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_the_stats_and_error_profile_files_are_those_of_the_pretrimmed_run(case, stub_tree, reads, tmp_path):
    d, prefix = stub_tree
    files = {}
    for tag, trimmed in (("want", True), ("got", False)):
        files[tag] = [str(tmp_path / ("%s.%s" % (tag, x))) for x in ("stats", "errprof")]
        _salt(d, prefix, read_cases()[case] + ["-t", "4", "--stats", files[tag][0], "--error-profile", files[tag][1]] + ([] if trimmed else TRIM_ARGS), _files(reads, case, trimmed))
    for a, b in zip(files["got"], files["want"]):
        ta, tb = open(a, "rb").read(), open(b, "rb").read()
        assert ta == tb and len(ta) > 500, a


def test_clips_and_the_default_adapter_of_mate_2(stub_tree, reads, tmp_path):
    """--trim-front / --trim-tail / --trim-min-overlap / --trim-error-pct reach the rule, and without --trim-adapter2 mate 2 is searched with mate 1's."""
    d, prefix = stub_tree
    o = tc.opts(adapter=tc.ADAPTER, front=3, tail=2, min_overlap=8, error_pct=20)
    counts = np.zeros((2, 8), dtype=np.uint64)
    pre = []
    for mate, name in ((0, "pe1"), (1, "pe2")):
        pre.append(str(tmp_path / (name + "_t.fq")))
        open(pre[-1], "wb").write(salt_amd.trim_fastq(open(reads[name], "rb").read(), mate, counts=counts, **o))
    args = read_cases()["pe_default"] + ["-t", "4"]
    want = _salt(d, prefix, args, pre)
    got = _salt(d, prefix, args + ["--trim-adapter", tc.ADAPTER, "--trim-front", "3", "--trim-tail", "2", "--trim-min-overlap", "8", "--trim-error-pct", "20"], [reads["pe1"], reads["pe2"]])
    assert strip_pg(got.stdout) == strip_pg(want.stdout)
    line = [l for l in got.stderr.decode().split("\n") if l.startswith("[salt] trim: ")][-1]
    assert "mate 1: reads 1000 " in line and "mate 2: reads 1000 " in line and line.count("reads_clipped 1000") == 2
    assert " bases_out %d " % counts[0][2] in line and " bases_out %d " % counts[1][2] in line


BAD = [(["--trim-adapter", "ACGN"], "1 to 64 letters of ACGT"), (["--trim-adapter", "A" * 65], "1 to 64 letters of ACGT"), (["--trim-adapter", ""], "1 to 64 letters"),
       (["--trim-adapter", "ACGT", "--trim-adapter2", "AC-T"], "--trim-adapter2"), (["--trim-adapter2", "ACGT"], "needs --trim-adapter"),
       (["--trim-min-overlap", "5"], "give --trim-adapter"), (["--trim-error-pct", "10"], "give --trim-adapter"),
       (["--trim-adapter", "ACGT", "--trim-min-overlap", "0"], "from 1 to 64"), (["--trim-adapter", "ACGT", "--trim-min-overlap", "65"], "from 1 to 64"),
       (["--trim-adapter", "ACGT", "--trim-error-pct", "51"], "from 0 to 50"), (["--trim-adapter", "ACGT", "--trim-error-pct", "-1"], "from 0 to 50"),
       (["--trim-qual", "0"], "from 1 to 93"), (["--trim-qual", "94"], "from 1 to 93"), (["--trim-qual", "2x"], "from 1 to 93"),
       (["--trim-front", "512"], "from 0 to 511"), (["--trim-tail", "512"], "from 0 to 511"), (["--trim-tail", "-1"], "from 0 to 511")]


@pytest.mark.parametrize("args, word", BAD)
def test_a_bad_option_exits_before_the_index_is_loaded(args, word, stub_tree, reads):
    d, prefix = stub_tree
    p = subprocess.run([str(d / "bin" / "salt"), "-d", "-c"] + args + [prefix, reads["se"]], capture_output=True, env=_env(d, prefix), timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"Reload index" not in p.stderr
    assert word.encode() in p.stderr, p.stderr[-300:]


def test_the_usage_text_names_the_options(stub_tree):
    d, prefix = stub_tree
    p = subprocess.run([str(d / "bin" / "salt"), "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    for name in ("--trim-adapter ", "--trim-adapter2", "--trim-qual", "--trim-front", "--trim-tail", "--trim-min-overlap", "--trim-error-pct"):
        assert name.encode() in p.stderr, name


def test_without_the_options_nothing_changes(stub_tree):
    d, prefix = stub_tree
    p = _salt(d, prefix, read_cases()["se_default"] + ["-t", "8"], [os.path.join(LAMBDA, "reads_se.fq")], SALT_CHUNK_BYTES="9000")
    assert strip_pg(p.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert b"trim" not in p.stderr and b"text path" in p.stderr
