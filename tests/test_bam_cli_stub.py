"""`salt --bam` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c, as in test_bgzf_cli_stub.py.  The stub has neither
the record kernels nor the device compressor, so the records come from the host encoder (salt_bam_from_sam) and zlib: what is tested is the
stream -- a BAM header, every record in input order and the end-of-file block, through the text path (single and paired end), the host
pipeline and the hand-over between them, with several "devices" --, decoded by tests/bam_check.py, and that nothing changes without the
option."""
import gzip
import os
import shutil
import subprocess

import pytest

from bam_check import boundary_reads, decode_stream, sam_header, sam_records
from bgzf_check import EOF, members, strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("bamstub")
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


def _env(d, prefix, **kw):
    return dict(os.environ, SALT_STUB_PREFIX=prefix, LD_LIBRARY_PATH=str(d / "lib"), **kw)


def _golden(case):
    return open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()


def _check(stream, stderr, want):
    """The stream decodes to the golden: its header text (without @PG) and its record lines (without the empty ones)."""
    text, lines, recs = decode_stream(stream)
    assert strip_pg(text) == sam_header(want) and text.count(b"@PG\t") == 1
    assert lines == sam_records(want)
    assert b"[salt] BAM output: host records, " in stderr, stderr[-400:]
    return recs


def _cmd(d, case, extra, prefix, files):
    args = EXTRA_CASES[case][0] if case in EXTRA_CASES else read_cases()[case]
    return [str(d / "bin" / "salt")] + args + ["--bam"] + extra + [prefix] + files


@pytest.mark.parametrize("case,gpus", [("se_default", 1), ("se_default", 2), ("se_r5_s4_m16", 1), ("se_r5_s4_m16", 2)])
def test_bam_stream_of_the_text_path_to_a_pipe_and_to_a_file(case, gpus, stub_tree, tmp_path):
    d, prefix = stub_tree
    want = _golden(case)
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000")
    cmd = _cmd(d, case, ["-t", "16", "--gpus", str(gpus)], prefix, [os.path.join(LAMBDA, "reads_se.fq")])
    out = subprocess.run(cmd, capture_output=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert b"text path:" in out.stderr
    _check(out.stdout, out.stderr, want)
    assert len(members(out.stdout)) > 12 and out.stdout[-28:] == EOF
    f = tmp_path / "out.bam"
    with open(f, "wb") as fo:
        res = subprocess.run(cmd, stdout=fo, stderr=subprocess.PIPE, env=env, timeout=300)
    assert res.returncode == 0 and b"blocks written in turn" in res.stderr, res.stderr[-300:]
    _check(f.read_bytes(), res.stderr, want)
    # the same command twice: the same bytes (the header's @PG line carries the date and the command, not the time)
    assert f.read_bytes() == out.stdout
    # --bam --bgzf is --bam
    both = subprocess.run(cmd[:-2] + ["--bgzf"] + cmd[-2:], capture_output=True, env=env, timeout=300)
    assert both.returncode == 0
    assert decode_stream(both.stdout)[1] == sam_records(want)


def test_bam_records_without_cigar_tags(stub_tree):
    """se_plain_t4: no -d, no -c -- records without MD / NM / XV."""
    d, prefix = stub_tree
    out = subprocess.run(_cmd(d, "se_plain_t4", [], prefix, [os.path.join(LAMBDA, "reads_se.fq")]), capture_output=True,
                         env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    recs = _check(out.stdout, out.stderr, _golden("se_plain_t4"))
    assert not any(t.startswith(("MD", "NM", "XV")) for r in recs for t in r["tags"])


@pytest.mark.parametrize("case", ["pe_default", "ragged_pe"])
def test_bam_stream_of_the_paired_end_text_path(case, stub_tree):
    """Soft clips of rescued mates, unmapped mates with MAPQ 255, mate fields; the driver's blank lines leave no record."""
    d, prefix = stub_tree
    files = EXTRA_CASES[case][1] if case in EXTRA_CASES else ["reads_pe_1.fq", "reads_pe_2.fq"]
    out = subprocess.run(_cmd(d, case, ["-t", "16", "--gpus", "2"], prefix, [os.path.join(LAMBDA, f) for f in files]),
                         capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert b"text path (paired end)" in out.stderr
    recs = _check(out.stdout, out.stderr, _golden(case))
    assert any(r["mapq"] == 255 and r["flag"] & 4 for r in recs) and any((w & 15) == 4 for r in recs for w in r["cigar"])
    assert all(r["flag"] & 1 for r in recs)


def test_bam_positions_at_contig_ends(stub_tree):
    d, prefix = stub_tree
    out = subprocess.run(_cmd(d, "span_default", [], prefix, [os.path.join(LAMBDA, "reads_span.fq")]), capture_output=True,
                         env=_env(d, prefix), timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    _check(out.stdout, out.stderr, _golden("span_default"))


def test_bam_bins_of_reads_at_the_16_kb_edges(stub_tree, tmp_path):
    """Reads that end on, or start next to, a multiple of 16 384: bin from POS - 1, not from POS (bam_check recomputes every bin)."""
    d, prefix = stub_tree
    fq = tmp_path / "edges.fq"
    fq.write_bytes(boundary_reads(os.path.join(LAMBDA, "genome.fa")))
    plain = subprocess.run([str(d / "bin" / "salt"), "-d", "-c", prefix, str(fq)], capture_output=True, env=_env(d, prefix), timeout=300)
    out = subprocess.run([str(d / "bin" / "salt"), "-d", "-c", "--bam", prefix, str(fq)], capture_output=True, env=_env(d, prefix), timeout=300)
    assert plain.returncode == 0 and out.returncode == 0, out.stderr[-500:]
    text, lines, recs = decode_stream(out.stdout)
    assert lines == sam_records(plain.stdout) and len(recs) == 16
    assert {r["pos"] for r in recs} >= {16284, 16383, 16384, 32668, 32767, 32768}
    assert {r["bin"] for r in recs} >= {4681, 4682, 4683, 585}


def test_bam_stream_of_the_host_pipeline_on_gzip_input(stub_tree, tmp_path):
    d, prefix = stub_tree
    plain = tmp_path / "reads.fq.gz"
    with gzip.open(plain, "wb") as f:
        f.write(open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read())
    out = subprocess.run(_cmd(d, "se_default", ["-t", "8"], prefix, [str(plain)]), capture_output=True, env=_env(d, prefix), timeout=300)
    assert out.returncode == 0 and b"host phases" in out.stderr, out.stderr[-500:]
    _check(out.stdout, out.stderr, _golden("se_default"))
    # forced onto the host pipeline, paired end
    out = subprocess.run(_cmd(d, "pe_default", ["-t", "8"], prefix, [os.path.join(LAMBDA, "reads_pe_1.fq"), os.path.join(LAMBDA, "reads_pe_2.fq")]),
                         capture_output=True, env=_env(d, prefix, SALT_HOST_PIPELINE="1"), timeout=300)
    assert out.returncode == 0 and b"host phases" in out.stderr, out.stderr[-500:]
    _check(out.stdout, out.stderr, _golden("pe_default"))


@pytest.mark.parametrize("gpus", [1, 2])
def test_bam_stream_across_the_hand_over_to_the_host_parser(gpus, stub_tree, tmp_path):
    """A multi-line record in the middle of the file: one stream, the header once, the end-of-file block once."""
    d, prefix = stub_tree
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq = tmp_path / "mid_multiline.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    res = subprocess.run(_cmd(d, "se_default", ["-t", "8", "--gpus", str(gpus)], prefix, [str(fq)]), capture_output=True,
                         env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    _check(res.stdout, res.stderr, _golden("se_default"))
    assert sum(1 for m, _ in members(res.stdout) if m == EOF) == 1


@pytest.mark.parametrize("pipeline", ["text", "host"])
def test_a_read_name_of_255_bytes_is_an_error_not_a_truncated_name(pipeline, stub_tree, tmp_path):
    d, prefix = stub_tree
    lines = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    lines[4 * 700] = b"@" + b"q" * 255 + b" comment"
    fq = tmp_path / "long_name.fq"
    fq.write_bytes(b"\n".join(lines))
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000", **({"SALT_HOST_PIPELINE": "1"} if pipeline == "host" else {}))
    res = subprocess.run(_cmd(d, "se_default", ["-t", "4"], prefix, [str(fq)]), capture_output=True, env=env, timeout=300)
    assert res.returncode == 1, res.stderr[-600:]
    assert b"at most 254 bytes" in res.stderr and b"BAM output:" not in res.stderr
    assert res.stdout[-28:] != EOF, "a failed run must not end like a complete file"
    lines[4 * 700] = b"@" + b"q" * 254 + b" comment"                 # 254 bytes fit
    fq.write_bytes(b"\n".join(lines))
    res = subprocess.run(_cmd(d, "se_default", ["-t", "4"], prefix, [str(fq)]), capture_output=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert decode_stream(res.stdout)[2][700]["name"] == b"q" * 254
    # and without the option the long name is no error
    res = subprocess.run([a for a in _cmd(d, "se_default", ["-t", "4"], prefix, [str(fq)]) if a != "--bam"], capture_output=True, env=env, timeout=300)
    assert res.returncode == 0


def test_without_the_option_the_output_is_what_it_was(stub_tree):
    d, prefix = stub_tree
    want = _golden("se_default")
    cmd = [str(d / "bin" / "salt")] + read_cases()["se_default"] + ["-t", "16", "--gpus", "2", prefix, os.path.join(LAMBDA, "reads_se.fq")]
    out = subprocess.run(cmd, capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert strip_pg(out.stdout) == want and b"BGZF" not in out.stderr and b"BAM" not in out.stderr
    z = subprocess.run(cmd[:-2] + ["--bgzf"] + cmd[-2:], capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert z.returncode == 0 and strip_pg(gzip.decompress(z.stdout)) == want and b"BAM" not in z.stderr


@pytest.fixture(scope="module")
def salt_sanitized(tmp_path_factory, oracle_lib):
    """salt_main.cc + the host library's sources with ASan+UBSan and with TSan against the stub, built the way test_sanitizers.py builds them."""
    d = tmp_path_factory.mktemp("bamsan")
    os.makedirs(d / "lib")
    host = os.path.join(ROOT, "salt_amd", "host")
    subprocess.run(["gcc", "-O1", "-g", "-fPIC", "-shared", "-o", str(d / "lib" / "libsalt_gpu.so"),
                    os.path.join(ROOT, "tests", "stub", "salt_gpu_stub.c"), os.path.join(ROOT, "oracle", "salt_oracle.c"), "-lm", "-lpthread"], check=True)
    subprocess.run(["make", "-C", host], check=True, stdout=subprocess.DEVNULL)
    bins = {}
    for tag, san in (("asan", "address,undefined"), ("tsan", "thread")):
        out = str(d / ("salt." + tag))
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=" + san, "-fno-omit-frame-pointer", "-o", out,
                        os.path.join(host, "salt_main.cc"), os.path.join(host, "salt_host.cc"), os.path.join(host, "salt_idx.cc"),
                        "-L" + str(d / "lib"), "-lsalt_gpu", "-lz", "-lpthread", "-ldl"], check=True)
        bins[tag] = out
    prefix = str(d / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return d, bins, prefix


@pytest.mark.parametrize("tag", ["asan", "tsan"])
def test_bam_host_encoder_under_sanitizers(tag, salt_sanitized):
    """The host encoder and compressor on the worker threads of two "devices", chunks of 3001 bytes: no sanitizer report, the golden records."""
    d, bins, prefix = salt_sanitized
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=0:exitcode=96:report_signal_unsafe=0", SALT_STUB_PREFIX=prefix, SALT_CHUNK_BYTES="3001", LD_LIBRARY_PATH=str(d / "lib"))
    p = subprocess.run([bins[tag]] + read_cases()["pe_default"] + ["--bam", "-t", "16", "--gpus", "2", prefix, os.path.join(LAMBDA, "reads_pe_1.fq"),
                        os.path.join(LAMBDA, "reads_pe_2.fq")], capture_output=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    for word in (b"runtime error", b"AddressSanitizer", b"ThreadSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    _check(p.stdout, p.stderr, _golden("pe_default"))
