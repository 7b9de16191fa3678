"""Blocked-gzip FASTQ through the device-inflate path of the `salt` binary, without a GPU: tests/stub/salt_gpu_inflate_stub.cc (the three
workspace entry points over the host model of the kernel's source) linked together with the unchanged tests/stub/salt_gpu_stub.c.  What is
tested is the driver: compressed blocks into the input buffer, record boundaries from windows peeked out of "the device's" text, the
capacity and hand-over paths, the order of the output -- and that the zlib path gives the same bytes.  The device path is taken with
SALT_INFLATE_DEVICE=1 (it is the slower of the two, so it is not the default); SALT_INFLATE_HOST=1 overrides it."""
import os
import shutil
import subprocess

import pytest

import inflate_cases as ic
from bam_check import decode_stream, sam_header, sam_records
from bgzf_check import strip_pg
from conftest import LAMBDA, ROOT, read_cases

STUB_SRC = [os.path.join(ROOT, "tests", "stub", "salt_gpu_stub.c"), os.path.join(ROOT, "oracle", "salt_oracle.c")]
INFLATE_STUB = os.path.join(ROOT, "tests", "stub", "salt_gpu_inflate_stub.cc")


def _stub_lib(d, opt):
    """libsalt_gpu.so of the two stubs: the C one compiled as it always is, the inflate entry points in front of it."""
    objs = []
    for src in STUB_SRC:
        objs.append(str(d / (os.path.basename(src) + ".o")))
        subprocess.run(["gcc", opt, "-g", "-fPIC", "-Wall", "-c", "-o", objs[-1], src], check=True)
    subprocess.run(["g++", opt, "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", str(d / "lib" / "libsalt_gpu.so"), INFLATE_STUB] + objs + ["-lm", "-lpthread"],
                   check=True)


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("inflatestub")
    os.makedirs(d / "bin"); os.makedirs(d / "lib")
    subprocess.run(["make", "-C", os.path.join(ROOT, "salt_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    shutil.copy(os.path.join(ROOT, "salt_amd", "bin", "salt"), d / "bin" / "salt")
    shutil.copy(os.path.join(ROOT, "salt_amd", "lib", "libsalt_host.so"), d / "lib" / "libsalt_host.so")
    _stub_lib(d, "-O2")
    prefix = str(d / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return d, prefix


def _env(d, prefix, **kw):
    return dict(dict(os.environ, SALT_STUB_PREFIX=prefix, SALT_CHUNK_BYTES="9000", SALT_INFLATE_DEVICE="1", LD_LIBRARY_PATH=str(d / "lib")), **kw)


def _salt(d, prefix, fq, gpus, extra=(), exe=None, **kw):
    cmd = [exe or str(d / "bin" / "salt")] + read_cases()["se_default"] + list(extra) + ["-t", "8", "--gpus", str(gpus), prefix, str(fq)]
    return subprocess.run(cmd, capture_output=True, env=_env(d, prefix, **kw), timeout=600)


def _want():
    return open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()


SHAPES = [(700, 1), (700, 3), (65280, 1), (65280, 3)]


@pytest.mark.parametrize("block,gpus", SHAPES)
def test_device_inflate_gives_the_golden_sam_and_the_host_path_the_same_bytes(block, gpus, stub_tree, tmp_path):
    d, prefix = stub_tree
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(ic.bgzf(ic.reads(), block))
    log = str(tmp_path / "stub.log")
    dev = _salt(d, prefix, fq, gpus, SALT_STUB_LOG=log)
    assert dev.returncode == 0, dev.stderr[-600:]
    n_blocks = (len(ic.reads()) + block - 1) // block + 1
    assert b"[salt] BGZF input: device inflate, %d blocks" % n_blocks in dev.stderr and b"the host parser takes over" not in dev.stderr
    assert strip_pg(dev.stdout) == _want()
    rows = [l.split() for l in open(log).read().splitlines()]
    assert sum(int(r[1]) for r in rows) == 2000 and len(rows) > 10            # many chunks, every read exactly once
    assert {int(r[0]) for r in rows} == set(range(gpus))
    host = _salt(d, prefix, fq, gpus, SALT_INFLATE_HOST="1")
    assert host.returncode == 0 and b"[salt] BGZF input: host inflate, %d blocks" % n_blocks in host.stderr, host.stderr[-600:]
    assert host.stdout == dev.stdout


def test_without_the_variable_the_workers_inflate(stub_tree, tmp_path):
    d, prefix = stub_tree
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(ic.bgzf(ic.reads(), 700))
    out = _salt(d, prefix, fq, 3, SALT_INFLATE_DEVICE="")
    assert out.returncode == 0 and b"[salt] BGZF input: host inflate, " in out.stderr and strip_pg(out.stdout) == _want(), out.stderr[-600:]
    out = _salt(d, prefix, fq, 3, SALT_INFLATE_DEVICE="0")
    assert out.returncode == 0 and b"[salt] BGZF input: host inflate, " in out.stderr and strip_pg(out.stdout) == _want(), out.stderr[-600:]


def test_plain_input_says_nothing_about_blocked_gzip(stub_tree):
    d, prefix = stub_tree
    out = _salt(d, prefix, os.path.join(LAMBDA, "reads_se.fq"), 1)
    assert out.returncode == 0 and strip_pg(out.stdout) == _want() and b"BGZF" not in out.stderr


@pytest.mark.parametrize("block,gpus", SHAPES)
def test_bam_behind_the_device_inflate(block, gpus, stub_tree, tmp_path):
    d, prefix = stub_tree
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(ic.bgzf(ic.reads(), block))
    out = _salt(d, prefix, fq, gpus, extra=["--bam"])
    assert out.returncode == 0 and b"device inflate" in out.stderr, out.stderr[-600:]
    text, lines, _ = decode_stream(out.stdout)
    assert strip_pg(text) == sam_header(_want()) and lines == sam_records(_want())


@pytest.mark.parametrize("block,gpus", SHAPES)
def test_the_host_parser_takes_over_mid_file(block, gpus, stub_tree, tmp_path):
    """A record wrapped over several lines behind the golden reads: the chunk that holds it goes to the host parser, from a record start that
    was found in a window of the device's text.  The stream must be the one plain input gives."""
    d, prefix = stub_tree
    lines = ic.reads().split(b"\n")
    r = lines[4 * 1200:4 * 1200 + 4]
    text = ic.reads() + b"\n".join([b"@wrapped", r[1][:40], r[1][40:], b"+", r[3][:15], r[3][15:]]) + b"\n"
    plain_fq, fq = tmp_path / "reads.fq", tmp_path / "reads.fq.gz"
    plain_fq.write_bytes(text)
    fq.write_bytes(ic.bgzf(text, block))
    plain = _salt(d, prefix, plain_fq, gpus)
    assert plain.returncode == 0 and b"the host parser takes over" in plain.stderr, plain.stderr[-600:]
    out = _salt(d, prefix, fq, gpus)
    assert out.returncode == 0, out.stderr[-600:]
    assert b"device inflate" in out.stderr and b"the host parser takes over" in out.stderr
    assert strip_pg(out.stdout) == strip_pg(plain.stdout) and strip_pg(out.stdout).startswith(_want())
    assert strip_pg(out.stdout).count(b"\n") == _want().count(b"\n") + 1


@pytest.mark.parametrize("block,gpus", SHAPES)
def test_a_damaged_block_ends_the_run(block, gpus, stub_tree, tmp_path):
    d, prefix = stub_tree
    raw = ic.reads()
    members = [ic.member(ic.deflate(raw[o:o + block]), raw[o:o + block]) for o in range(0, len(raw), block)]
    k = len(members) // 2                                       # the middle of a payload in the middle of the file (the block table still reads)
    at = sum(len(m) for m in members[:k]) + 18 + (len(members[k]) - 26) // 2
    stream = bytearray(b"".join(members) + ic.EOF)
    stream[at] ^= 0x55
    fq = tmp_path / "damaged.fq.gz"
    fq.write_bytes(bytes(stream))
    for env in ({}, {"SALT_INFLATE_HOST": "1"}):
        out = _salt(d, prefix, fq, gpus, **env)
        assert out.returncode != 0 and b"damaged or oversized gzip block" in out.stderr, out.stderr[-600:]
        assert (b"host inflate" if env else b"device inflate") in out.stderr


@pytest.mark.parametrize("block,gpus", SHAPES)
def test_the_last_record_without_its_newline(block, gpus, stub_tree, tmp_path):
    d, prefix = stub_tree
    assert ic.reads().endswith(b"\n")
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(ic.bgzf(ic.reads()[:-1], block))
    out = _salt(d, prefix, fq, gpus)
    assert out.returncode == 0 and b"device inflate" in out.stderr and b"the host parser takes over" not in out.stderr, out.stderr[-600:]
    assert strip_pg(out.stdout) == _want()


@pytest.mark.parametrize("block,gpus", [(700, 3), (65280, 1)])
def test_a_name_line_longer_than_the_first_window(block, gpus, stub_tree, tmp_path):
    """A comment of 150 000 bytes on one name line: chunks begin and end inside it, the next record start lies beyond the 64 KiB a worker
    peeks first, and the widened window must give the cut the whole buffer gives -- the stream of plain input."""
    d, prefix = stub_tree
    lines = ic.reads().split(b"\n")
    lines[4 * 900] += b" " + b"c" * 150000
    text = b"\n".join(lines)
    plain_fq, fq = tmp_path / "reads.fq", tmp_path / "reads.fq.gz"
    plain_fq.write_bytes(text)
    fq.write_bytes(ic.bgzf(text, block))
    plain = _salt(d, prefix, plain_fq, gpus)
    out = _salt(d, prefix, fq, gpus)
    assert plain.returncode == 0 and out.returncode == 0, out.stderr[-600:]
    assert b"device inflate" in out.stderr and b"the host parser takes over" not in out.stderr
    assert strip_pg(out.stdout) == strip_pg(plain.stdout) == _want()


@pytest.fixture(scope="module")
def salt_asan(tmp_path_factory, oracle_lib):
    """salt_main.cc + the host library's sources with ASan+UBSan against the two stubs, built the way test_sanitizers.py builds them."""
    d = tmp_path_factory.mktemp("inflatesan")
    os.makedirs(d / "lib")
    host = os.path.join(ROOT, "salt_amd", "host")
    _stub_lib(d, "-O1")
    subprocess.run(["make", "-C", host], check=True, stdout=subprocess.DEVNULL)
    exe = str(d / "salt.asan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(host, "salt_main.cc"), os.path.join(host, "salt_host.cc"), os.path.join(host, "salt_idx.cc"),
                    "-L" + str(d / "lib"), "-lsalt_gpu", "-lz", "-lpthread", "-ldl"], check=True)
    prefix = str(d / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return d, exe, prefix


@pytest.mark.parametrize("block,gpus", SHAPES)
def test_device_inflate_path_under_asan_ubsan(block, gpus, salt_asan, tmp_path):
    d, exe, prefix = salt_asan
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(ic.bgzf(ic.reads(), block))
    out = _salt(d, prefix, fq, gpus, exe=exe, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in out.stderr, out.stderr.decode()[-3000:]
    assert b"device inflate" in out.stderr and strip_pg(out.stdout) == _want()
