"""Blocked-gzip input inflated on the device: k_bgzf_inflate on its own (api.bgzf_inflate over salt_gpu_bgzf_inflate) on every stream the
host model of its source has passed in test_inflate_model.py, the round trip through the project's own deflate kernels, damaged members
(each refused, each followed by a good call), and the `salt` binary on blocked-gzip FASTQ with SALT_INFLATE_DEVICE=1 against its zlib path
(the default: DESIGN.md 4.3)."""
import os
import random
import subprocess

import pytest

import inflate_cases as ic
from bam_check import decode_stream, sam_header, sam_records
from bgzf_check import strip_pg
from conftest import LAMBDA, ROOT, read_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deflater(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgzfmodel") / "bgzf_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "bgzf_model.cc")], check=True)
    return exe


def _inflate_twice(stream):
    import salt_amd
    out = salt_amd.bgzf_inflate(stream)
    assert salt_amd.bgzf_inflate(stream) == out, "two runs gave different bytes"
    return out


@pytest.mark.parametrize("name", sorted(ic.valid_cases()) + ["own_deflater"])
def test_unit_valid_members(name, deflater):
    stream, text = ic.valid_cases(deflater)[name]
    assert _inflate_twice(stream) == text


def test_unit_600_blocks_of_mixed_settings_and_sizes():
    """More members than a launch has workgroups resident, of unequal sizes (1 byte to 65 280), every block type among them."""
    src = open(os.path.join(LAMBDA, "expect_pe_default.sam"), "rb").read() + ic.reads()
    sizes, settings = [65280, 700, 13000, 333, 4567, 1], sorted(ic.SETTINGS.values())
    stream, text, at = [], [], 0
    for i in range(600):
        piece = (src + src)[at % len(src):at % len(src) + sizes[i % 6]]
        at += len(piece)
        lv, st = settings[i % 7]
        stream.append(ic.member(ic.deflate(piece, lv, st), piece))
        text.append(piece)
    text = b"".join(text)
    assert len(text) > 8000000
    assert _inflate_twice(b"".join(stream) + ic.EOF) == text


@pytest.mark.parametrize("what", ["sam_8MiB", "random_1MiB"])
def test_unit_round_trip_through_the_deflate_kernels(what):
    import salt_amd
    if what == "sam_8MiB":
        sam = open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
        x = (sam * ((8 << 20) // len(sam) + 1))[:8 << 20]
    else:
        x = random.Random(41).randbytes(1 << 20)
    assert salt_amd.bgzf_inflate(salt_amd.bgzf_deflate(x)) == x


def _damaged():
    payload, text = ic.level6_block()
    d = ic.damaged_cases()
    cases = {k: d[k] for k in ("crc_bit", "truncated_by_half", "distance_in_front_of_the_block", "oversubscribed_code_lengths")}
    for at in [97 * k for k in (1, 20, 77, 130, 190)]:          # five of the model test's offsets
        cases["flip_%d" % at] = ic.flipped(payload, text, at)
    return cases


@pytest.mark.parametrize("name", sorted(_damaged()))
def test_unit_damaged_members_raise_and_leave_the_device_usable(name):
    """Only streams the sanitized host model has refused cleanly (test_inflate_model.py).  A good member in front: the error names member 1."""
    import salt_amd
    good = ic.bgzf(ic.reads()[:5000], 5000, eof=False)
    with pytest.raises(salt_amd.SaltError, match="BGZF member 1: "):
        salt_amd.bgzf_inflate(good + _damaged()[name] + ic.EOF)
    assert salt_amd.bgzf_inflate(good + ic.EOF) == ic.reads()[:5000]


def test_unit_bsize_past_the_end_is_refused_before_the_device_runs():
    import salt_amd
    with pytest.raises(salt_amd.SaltError, match="BGZF member 0: "):
        salt_amd.bgzf_inflate(ic.damaged_cases()["bsize_past_the_end"])


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("lamidx") / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return prefix


def _salt(prefix, fq, extra=(), **env):
    cmd = [os.path.join(ROOT, "salt_amd", "bin", "salt")] + read_cases()["se_default"] + list(extra) + [prefix, str(fq)]
    return subprocess.run(cmd, capture_output=True, env=dict(dict(os.environ, SALT_INFLATE_DEVICE="1"), **env), timeout=600)


@pytest.mark.parametrize("block", [700, 65280])
@pytest.mark.parametrize("chunk", ["3001", "70000"])
def test_cli_blocked_gzip_input_on_the_device(block, chunk, lambda_cli_index, tmp_path):
    want = open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(ic.bgzf(ic.reads(), block))
    dev = _salt(lambda_cli_index, fq, SALT_CHUNK_BYTES=chunk)
    assert dev.returncode == 0, dev.stderr[-600:]
    assert b"text path" in dev.stderr and b"[salt] BGZF input: device inflate, " in dev.stderr and b"the host parser takes over" not in dev.stderr
    assert strip_pg(dev.stdout) == want
    host = _salt(lambda_cli_index, fq, SALT_CHUNK_BYTES=chunk, SALT_INFLATE_HOST="1")
    assert host.returncode == 0 and b"[salt] BGZF input: host inflate, " in host.stderr, host.stderr[-600:]
    assert host.stdout == dev.stdout


def test_cli_bam_behind_the_device_inflate(lambda_cli_index, tmp_path):
    want = open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    fq = tmp_path / "reads.fq.gz"
    fq.write_bytes(ic.bgzf(ic.reads(), 65280))
    out = _salt(lambda_cli_index, fq, extra=["--bam"], SALT_CHUNK_BYTES="70000")
    assert out.returncode == 0 and b"device inflate" in out.stderr and b"BAM output: device records" in out.stderr, out.stderr[-600:]
    text, lines, _ = decode_stream(out.stdout)
    assert strip_pg(text) == sam_header(want) and lines == sam_records(want)


def test_cli_damaged_file_exits_nonzero(lambda_cli_index, tmp_path):
    raw = ic.reads()
    members = [ic.member(ic.deflate(raw[o:o + 65280]), raw[o:o + 65280]) for o in range(0, len(raw), 65280)]
    at = 18 + 97 * 77                                           # the first block is test_inflate_model.py's, and so is the flipped offset: the host model refuses it
    stream = bytearray(b"".join(members) + ic.EOF)
    stream[at] ^= 0x55
    fq = tmp_path / "damaged.fq.gz"
    fq.write_bytes(bytes(stream))
    out = _salt(lambda_cli_index, fq, SALT_CHUNK_BYTES="70000")
    assert out.returncode != 0 and b"device inflate" in out.stderr and b"damaged or oversized gzip block" in out.stderr, out.stderr[-600:]


def test_cli_workspace_recreated_for_shorter_records_inflates_again(lambda_cli_index, tmp_path):
    """A head of 500-byte records and a body of 230-byte ones (as test_cli_text_path_regrows_its_workspace_when_records_get_shorter): a chunk
    holds more reads than the workspace was made for, the worker makes a new one -- whose text buffer is empty, so the chunk is inflated again."""
    src = ic.reads().splitlines()
    recs = [src[i:i + 4] for i in range(0, len(src) - 3, 4)]
    out = []
    for rep in range(16):
        for j, r in enumerate(recs):
            out += [b"@r%d_%d" % (rep, j) + (b"_" + b"x" * 280 if rep == 0 and j < 200 else b""), r[1], b"+", r[3]]
    fq = tmp_path / "mixed.fq.gz"
    fq.write_bytes(ic.bgzf(b"\n".join(out) + b"\n", 65280, 1))
    dev = _salt(lambda_cli_index, fq, extra=["-t", "4"], SALT_CHUNK_MB="4", SALT_TEXT_TRACE="1")
    host = _salt(lambda_cli_index, fq, extra=["-t", "4"], SALT_CHUNK_MB="4", SALT_INFLATE_HOST="1")
    assert dev.returncode == 0 and host.returncode == 0, (dev.stderr[-300:], host.stderr[-300:])
    assert b"device inflate" in dev.stderr and b"workspace re-created" in dev.stderr, dev.stderr[-600:]
    assert dev.stdout == host.stdout and dev.stdout.count(b"\n") > 32000
