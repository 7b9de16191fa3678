"""The device's BGZF member decoder (salt_amd/csrc/salt_inflate_block.h) run on the host by tools/inflate_model.cc, one thread of the
workgroup after the other, plain and under AddressSanitizer + UBSan: every kind of valid member gives its text back, every damaged one is
refused with exit status 3 -- and without a sanitizer report, which is the proof of the decoder's bounds rules that a GPU cannot give.
(The kernel itself: test_gpu_inflate.py.)"""
import os
import subprocess
import zlib

import pytest

import inflate_cases as ic
from conftest import ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflatemodel")
    src = os.path.join(ROOT, "tools", "inflate_model.cc")
    plain, san, deflater = str(d / "inflate_model"), str(d / "inflate_model.san"), str(d / "bgzf_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", san, src], check=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", deflater, os.path.join(ROOT, "tools", "bgzf_model.cc")], check=True)
    return plain, san, deflater


def _run(exe, stream):
    p = subprocess.run([exe], input=stream, capture_output=True, env=SAN_ENV, timeout=120)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    return p


NAMES = sorted(ic.valid_cases()) + ["own_deflater"]


@pytest.mark.parametrize("name", NAMES)
def test_valid_members_give_their_text_back(name, models):
    plain, san, deflater = models
    stream, text = ic.valid_cases(deflater)[name]
    if name == "distance_32768":                                # the hand-made stream is valid to zlib too
        assert len(text) == 65276 and zlib.decompress(stream[18:-8 - len(ic.EOF)], -15) == text
    if name == "flushed":
        assert stream.count(b"\x00\x00\xff\xff") >= 13          # the empty stored blocks of the flushes
    for exe in (plain, san):
        p = _run(exe, stream)
        assert p.returncode == 0, p.stderr[-300:]
        assert p.stdout == text


def test_block_types_of_the_settings_are_what_they_are_meant_to_be():
    """BTYPE of the first deflate block: Z_FIXED 1, Z_RLE 2, Z_HUFFMAN_ONLY 2, level 0 stored."""
    block = ic.reads()[:65280]
    btype = {name: (ic.deflate(block, lv, st)[0] >> 1) & 3 for name, (lv, st) in ic.SETTINGS.items()}
    assert (btype["fixed"], btype["rle"], btype["huffman_only"], btype["level0_stored"], btype["level6"]) == (1, 2, 2, 0, 2)


def test_every_flipped_payload_byte_is_refused(models):
    """One byte ^ 0x55 at every 97th offset of a level-6 payload: zlib's inflate plus the CRC check refuses every one, and so must the model."""
    plain, san, _ = models
    payload, text = ic.level6_block()
    offsets = ic.flip_offsets(payload)
    assert len(offsets) > 150
    for at in offsets:
        stream = ic.flipped(payload, text, at)
        assert ic.zlib_rejects(stream), at
        for exe in (plain, san):
            p = _run(exe, stream)
            assert p.returncode == 3 and p.stdout == b"" and b"block 0: " in p.stderr, (at, p.returncode, p.stderr[-300:])


@pytest.mark.parametrize("name", sorted(ic.damaged_cases()))
def test_damaged_members_are_refused(name, models):
    plain, san, _ = models
    stream = ic.damaged_cases()[name]
    if name != "bsize_past_the_end":
        assert ic.zlib_rejects(stream)
    for exe in (plain, san):
        p = _run(exe, stream)
        assert p.returncode == 3 and p.stdout == b"" and b"block 0: " in p.stderr, (p.returncode, p.stderr[-300:])


def test_a_bad_member_behind_good_ones_is_named(models):
    plain, _, _ = models
    payload, text = ic.level6_block()
    stream = ic.bgzf(text[:3000], 1000, eof=False) + ic.damaged_cases()["crc_bit"]
    p = _run(plain, stream)
    assert p.returncode == 3 and b"block 3: CRC-32 mismatch" in p.stderr and p.stdout == text[:3000]
