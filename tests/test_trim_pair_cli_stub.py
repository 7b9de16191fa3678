"""`salt --trim-pair-overlap` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_trim_cli_stub.py.  The stub
has no trim kernels, so the whole run goes through the host pipeline, whose parser trims every pair with the host twin (salt_trim_pair_span)
-- and stdout must be, the @PG line apart, what `salt` without the options prints for the two files that salt_amd.trim_fastq_pair trimmed
beforehand, which take the text path.  The pairs are cut, seeded, from the golden genome (trim_pair_check.constructed_pairs)."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import salt_amd
import trim_check as tc
import trim_pair_check as pc
from bam_check import decode_stream
from bgzf_check import stream_text, strip_pg
from conftest import LAMBDA, ROOT, read_cases

TRIM = dict(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2, qual=20)
TRIM_ARGS = ["--trim-adapter", tc.ADAPTER, "--trim-adapter2", tc.ADAPTER2, "--trim-qual", "20"]
PAIR_ARGS = ["--trim-pair-overlap"]


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("trimpairstub")
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
    """the constructed files and their pre-trimmed copies under both sets of options: name -> path; "counts*", "pairs*": the twin's counters"""
    d = tmp_path_factory.mktemp("trimpairreads")
    fq1, fq2 = pc.constructed_pairs(600, seed=4)
    out = {"raw": (fq1, fq2)}
    for tag, kw in (("pair", {}), ("both", TRIM), ("p30", dict(min_overlap=30, error_pct=0))):
        counts, pairs = np.zeros((2, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        t1, t2 = salt_amd.trim_fastq_pair(fq1, fq2, counts=counts, pair_counts=pairs, **kw)
        out["counts_" + tag], out["pairs_" + tag] = counts, pairs
        for name, text in (("1", fq1), ("2", fq2), ("1_t_" + tag, t1), ("2_t_" + tag, t2)):
            out[name] = str(d / (name + ".fq"))
            open(out[name], "wb").write(text)
    assert out["pairs_pair"][2] > 150 and out["pairs_pair"][1] > 350 and out["counts_both"][0][3] > 50
    return out


def _env(d, prefix, **kw):
    return dict(os.environ, SALT_STUB_PREFIX=prefix, LD_LIBRARY_PATH=str(d / "lib"), **kw)


def _salt(d, prefix, args, files, **env):
    p = subprocess.run([str(d / "bin" / "salt")] + args + [prefix] + files, capture_output=True, env=_env(d, prefix, **env), timeout=300)
    assert p.returncode == 0, (args, p.stderr[-600:])
    return p


def _text(stdout, fmt):
    if fmt == "plain":
        return strip_pg(stdout)
    if fmt == "bgzf":
        return strip_pg(stream_text(stdout))
    text, lines, _ = decode_stream(stdout)
    return strip_pg(text), lines


def counters(stderr):
    """the two [salt] trim: lines -> (who trimmed, (2, 8) array, (8,) array)"""
    lines = [l for l in stderr.decode().split("\n") if l.startswith("[salt] trim: ")]
    first = [l for l in lines if "reads_floored" in l]
    second = [l for l in lines if l.startswith("[salt] trim: pairs: ")]
    assert len(first) == 1 and len(second) == 1 and lines.index(second[0]) == lines.index(first[0]) + 1, stderr[-800:]
    who = first[0][len("[salt] trim: "):].split(":")[0]
    c = np.zeros((2, 8), dtype=np.uint64)
    for m, part in enumerate(first[0].split("mate ")[1:]):
        got = dict(re.findall(r"(\w+) (\d+)", part.split(":", 1)[1]))
        c[m] = [int(got[k]) for k in tc.COUNTERS]
    m = re.fullmatch(r"\[salt\] trim: pairs: pairs (\d+) overlapping (\d+) trimmed (\d+) mate 1: reads (\d+) bases (\d+) mate 2: reads (\d+) bases (\d+) skipped_long (\d+)", second[0])
    assert m, second[0]
    return who, c, np.array([int(x) for x in m.groups()], dtype=np.uint64)


@pytest.mark.parametrize("fmt", ["plain", "bam", "bgzf"])
@pytest.mark.parametrize("tag, extra", [("pair", []), ("both", TRIM_ARGS)])
def test_stdout_is_the_run_on_the_pretrimmed_files(tag, extra, fmt, stub_tree, reads):
    d, prefix = stub_tree
    args = read_cases()["pe_default"] + ["-t", "8"] + ([] if fmt == "plain" else ["--" + fmt])
    want = _salt(d, prefix, args, [reads["1_t_" + tag], reads["2_t_" + tag]], SALT_CHUNK_BYTES="9000")
    got = _salt(d, prefix, args + PAIR_ARGS + extra, [reads["1"], reads["2"]], SALT_CHUNK_BYTES="9000")
    assert _text(got.stdout, fmt) == _text(want.stdout, fmt) and len(got.stdout) > 30000
    assert b"text path" in want.stderr and b"[salt] trim:" not in want.stderr
    assert b"the whole run goes through the host pipeline" in got.stderr and b"text path" not in got.stderr
    who, c, p = counters(got.stderr)
    assert who == "host" and (c == reads["counts_" + tag]).all() and (p == reads["pairs_" + tag]).all(), (who, c, p)


def test_the_numeric_options_reach_the_rule_and_several_gpus_count_every_pair_once(stub_tree, reads):
    d, prefix = stub_tree
    args = read_cases()["pe_default"] + ["-t", "8", "--gpus", "3"]
    want = _salt(d, prefix, args, [reads["1_t_p30"], reads["2_t_p30"]])
    got = _salt(d, prefix, args + PAIR_ARGS + ["--trim-pair-min-overlap", "30", "--trim-pair-error-pct", "0"], [reads["1"], reads["2"]], SALT_CHUNK_BYTES="9000")
    assert strip_pg(got.stdout) == strip_pg(want.stdout)
    who, c, p = counters(got.stderr)
    assert (c == reads["counts_p30"]).all() and (p == reads["pairs_p30"]).all() and p[0] == 600
    assert (reads["pairs_p30"] != reads["pairs_pair"]).any()


def test_gzip_input_and_a_multi_line_record_in_the_middle(stub_tree, reads, tmp_path):
    d, prefix = stub_tree
    args = read_cases()["pe_default"] + ["-t", "8"]
    want = strip_pg(_salt(d, prefix, args, [reads["1_t_both"], reads["2_t_both"]]).stdout)
    gz = []
    for k in ("1", "2"):
        gz.append(str(tmp_path / ("reads_%s.fq.gz" % k)))
        with gzip.open(gz[-1], "wb") as f:
            f.write(open(reads[k], "rb").read())
    got = _salt(d, prefix, args + PAIR_ARGS + TRIM_ARGS, gz)
    assert strip_pg(got.stdout) == want
    assert (counters(got.stderr)[1] == reads["counts_both"]).all() and (counters(got.stderr)[2] == reads["pairs_both"]).all()
    recs = reads["raw"][1].split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 400 else r
    fq = tmp_path / "mid_multiline_2.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    got = _salt(d, prefix, args + PAIR_ARGS + TRIM_ARGS, [reads["1"], str(fq)], SALT_CHUNK_BYTES="9000")
    assert strip_pg(got.stdout) == want
    assert (counters(got.stderr)[1] == reads["counts_both"]).all() and (counters(got.stderr)[2] == reads["pairs_both"]).all()


def test_the_first_line_is_unchanged_and_without_the_flag_no_second_line(stub_tree, reads):
    """--trim-* alone prints the one line it printed before; with the flag the same line's format stands in front of the new one."""
    d, prefix = stub_tree
    args = read_cases()["pe_default"] + ["-t", "4"]
    plain = _salt(d, prefix, args + TRIM_ARGS, [reads["1"], reads["2"]])
    lines = [l for l in plain.stderr.decode().split("\n") if "trim" in l and not l.startswith("[salt] trim: this libsalt_gpu")]
    assert len(lines) == 1 and "pairs" not in lines[0]
    both = _salt(d, prefix, args + TRIM_ARGS + PAIR_ARGS, [reads["1"], reads["2"]])
    first = [l for l in both.stderr.decode().split("\n") if "reads_floored" in l][0]
    strip = lambda l: re.sub(r"\d+", "#", l)
    assert strip(first) == strip(lines[0])
    # what the per-read steps took before the pair step is what they take without it
    for name in ("reads ", "bases_in ", "reads_qual ", "bases_qual "):
        assert re.findall(name + r"(\d+)", first) == re.findall(name + r"(\d+)", lines[0])


def test_without_the_flag_nothing_changes(stub_tree):
    d, prefix = stub_tree
    files = [os.path.join(LAMBDA, "reads_pe_1.fq"), os.path.join(LAMBDA, "reads_pe_2.fq")]
    p = _salt(d, prefix, read_cases()["pe_default"] + ["-t", "8"], files, SALT_CHUNK_BYTES="9000")
    assert strip_pg(p.stdout) == open(os.path.join(LAMBDA, "expect_pe_default.sam"), "rb").read()
    assert b"trim" not in p.stderr and b"text path" in p.stderr


BAD = [(["-p", "--trim-pair-min-overlap", "20"], "give --trim-pair-overlap"), (["-p", "--trim-pair-error-pct", "10"], "give --trim-pair-overlap"),
       (["--trim-pair-overlap"], "needs the mates"), (["-p", "--trim-pair-overlap", "--trim-pair-min-overlap", "0"], "from 1 to 512"),
       (["-p", "--trim-pair-overlap", "--trim-pair-min-overlap", "513"], "from 1 to 512"), (["-p", "--trim-pair-overlap", "--trim-pair-error-pct", "51"], "from 0 to 50"),
       (["-p", "--trim-pair-overlap", "--trim-pair-error-pct", "-1"], "from 0 to 50"), (["-p", "--trim-pair-overlap", "--trim-pair-min-overlap", "2x"], "from 1 to 512")]


@pytest.mark.parametrize("args, word", BAD)
def test_a_bad_option_exits_before_the_index_is_loaded(args, word, stub_tree, reads):
    d, prefix = stub_tree
    files = [reads["1"], reads["2"]] if "-p" in args else [reads["1"]]
    p = subprocess.run([str(d / "bin" / "salt"), "-d", "-c"] + args + [prefix] + files, capture_output=True, env=_env(d, prefix), timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and b"Reload index" not in p.stderr
    assert b"[opt_parse]" in p.stderr and word.encode() in p.stderr, p.stderr[-300:]


def test_the_usage_text_names_the_options(stub_tree):
    d, prefix = stub_tree
    p = subprocess.run([str(d / "bin" / "salt"), "-h"], capture_output=True, env=_env(d, prefix), timeout=60)
    for name in ("--trim-pair-overlap ", "--trim-pair-min-overlap", "--trim-pair-error-pct"):
        assert name.encode() in p.stderr, name
