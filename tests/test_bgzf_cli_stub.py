"""`salt --bgzf` without a GPU: the real `salt` binary against tests/stub/salt_gpu_stub.c (the oracle behind the device's C ABI), as in
test_cli_multi_gpu_stub.py.  The stub has no device compressor, so the option takes the host compressor (zlib level 1 on the workers): what
is tested is the stream -- the header, every SAM block in input order and the end-of-file block as valid BGZF members, through the text path
(single and paired end), the host pipeline and the hand-over between them, with several "devices" -- and that nothing changes without the
option."""
import gzip
import os
import shutil
import subprocess

import pytest

from bgzf_check import EOF, members, stream_text, strip_pg
from conftest import LAMBDA, ROOT, read_cases


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("bgzfstub")
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


def _check(stream, stderr, want):
    assert gzip.decompress(stream) == stream_text(stream)          # gzip and the member-by-member reading agree
    assert strip_pg(stream_text(stream)) == want
    assert b"[salt] BGZF output: host deflate, " in stderr, stderr[-400:]


@pytest.mark.parametrize("case,gpus", [("se_default", 1), ("se_default", 2), ("se_r5_s4_m16", 1), ("se_r5_s4_m16", 2)])
def test_bgzf_stream_of_the_text_path_to_a_pipe_and_to_a_file(case, gpus, stub_tree, tmp_path):
    d, prefix = stub_tree
    want = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    env = _env(d, prefix, SALT_CHUNK_BYTES="9000")
    cmd = [str(d / "bin" / "salt")] + read_cases()[case] + ["--bgzf", "-t", "16", "--gpus", str(gpus), prefix, os.path.join(LAMBDA, "reads_se.fq")]
    out = subprocess.run(cmd, capture_output=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert b"text path:" in out.stderr
    _check(out.stdout, out.stderr, want)
    assert len(members(out.stdout)) > 12                            # the header, a run of blocks per chunk, the end-of-file block
    assert len(out.stdout) < len(want) // 2
    f = tmp_path / "out.sam.gz"
    with open(f, "wb") as fo:
        out = subprocess.run(cmd, stdout=fo, stderr=subprocess.PIPE, env=env, timeout=300)
    assert out.returncode == 0 and b"blocks written in turn" in out.stderr, out.stderr[-300:]
    _check(f.read_bytes(), out.stderr, want)


def test_bgzf_stream_of_the_paired_end_text_path(stub_tree, tmp_path):
    """Through the stub's salt_gpu_align_pe_text, set up as in test_salt_pe_text_path_cuts_both_files_by_record_count."""
    d, prefix = stub_tree
    want = open(os.path.join(LAMBDA, "expect_pe_default.sam"), "rb").read()
    f1 = os.path.join(LAMBDA, "reads_pe_1.fq")
    lines = open(os.path.join(LAMBDA, "reads_pe_2.fq"), "rb").read().split(b"\n")
    for i in range(0, len(lines) - 3, 4):
        lines[i] = lines[i] + b" " + b"c" * (i % 37)
    f2 = tmp_path / "mates.fq"
    f2.write_bytes(b"\n".join(lines))
    out = subprocess.run([str(d / "bin" / "salt")] + read_cases()["pe_default"] + ["--bgzf", "-t", "16", "--gpus", "2", prefix, f1, str(f2)],
                         capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="3000"), timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert b"text path (paired end)" in out.stderr
    _check(out.stdout, out.stderr, want)


def test_bgzf_stream_of_the_host_pipeline_on_gzip_input(stub_tree, tmp_path):
    d, prefix = stub_tree
    want = open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    plain = tmp_path / "reads.fq.gz"
    with gzip.open(plain, "wb") as f:
        f.write(open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read())
    out = subprocess.run([str(d / "bin" / "salt")] + read_cases()["se_default"] + ["--bgzf", "-t", "8", prefix, str(plain)],
                         capture_output=True, env=_env(d, prefix), timeout=300)
    assert out.returncode == 0 and b"host phases" in out.stderr, out.stderr[-500:]
    _check(out.stdout, out.stderr, want)
    # forced onto the host pipeline, paired end
    wpe = open(os.path.join(LAMBDA, "expect_pe_default.sam"), "rb").read()
    out = subprocess.run([str(d / "bin" / "salt")] + read_cases()["pe_default"] + ["--bgzf", "-t", "8", prefix, os.path.join(LAMBDA, "reads_pe_1.fq"),
                          os.path.join(LAMBDA, "reads_pe_2.fq")], capture_output=True, env=_env(d, prefix, SALT_HOST_PIPELINE="1"), timeout=300)
    assert out.returncode == 0 and b"host phases" in out.stderr, out.stderr[-500:]
    _check(out.stdout, out.stderr, wpe)


@pytest.mark.parametrize("gpus", [1, 2])
def test_bgzf_stream_across_the_hand_over_to_the_host_parser(gpus, stub_tree, tmp_path):
    """A multi-line record in the middle of the file: the text path writes the blocks in front of it, the host pipeline the rest -- one
    stream, the header once, the end-of-file block once."""
    d, prefix = stub_tree
    want = open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r       # behind the 256 KiB the text path is chosen from
    fq = tmp_path / "mid_multiline.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    res = subprocess.run([str(d / "bin" / "salt")] + read_cases()["se_default"] + ["--bgzf", "-t", "8", "--gpus", str(gpus), prefix, str(fq)],
                         capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert res.returncode == 0, res.stderr[-600:]
    assert b"the host parser takes over" in res.stderr and b"host phases" in res.stderr
    _check(res.stdout, res.stderr, want)
    text = stream_text(res.stdout)
    assert text.count(b"@HD") + text.count(b"@SQ") == want.count(b"@HD") + want.count(b"@SQ") and text.count(b"@PG\t") == 1
    assert sum(1 for m, _ in members(res.stdout) if m == EOF) == 1


def test_without_the_option_the_output_is_what_it_was(stub_tree):
    d, prefix = stub_tree
    want = open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    out = subprocess.run([str(d / "bin" / "salt")] + read_cases()["se_default"] + ["-t", "16", "--gpus", "2", prefix, os.path.join(LAMBDA, "reads_se.fq")],
                         capture_output=True, env=_env(d, prefix, SALT_CHUNK_BYTES="9000"), timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    assert strip_pg(out.stdout) == want and b"BGZF" not in out.stderr
    assert out.stdout.startswith(want[:64]) and not out.stdout.startswith(b"\x1f\x8b")


@pytest.fixture(scope="module")
def salt_sanitized(tmp_path_factory, oracle_lib):
    """salt_main.cc + the host library's sources with ASan+UBSan and with TSan against the stub, built the way test_sanitizers.py builds them."""
    d = tmp_path_factory.mktemp("bgzfsan")
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
def test_bgzf_host_compressor_under_sanitizers(tag, salt_sanitized):
    """The host compressor runs on the worker threads of two "devices", chunks of 3001 bytes: no sanitizer report, the golden text."""
    d, bins, prefix = salt_sanitized
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=0:exitcode=96:report_signal_unsafe=0", SALT_STUB_PREFIX=prefix, SALT_CHUNK_BYTES="3001", LD_LIBRARY_PATH=str(d / "lib"))
    p = subprocess.run([bins[tag]] + read_cases()["se_default"] + ["--bgzf", "-t", "16", "--gpus", "2", prefix, os.path.join(LAMBDA, "reads_se.fq")],
                       capture_output=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    for word in (b"runtime error", b"AddressSanitizer", b"ThreadSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    _check(p.stdout, p.stderr, open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read())
