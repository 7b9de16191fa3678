"""`salt --bgzf` on the device: the deflate kernels on their own (api.bgzf_deflate over salt_gpu_bgzf_deflate), their size against zlib, and
the `salt` binary with the option through the text path (single and paired end).  The block cut is api.BGZF_CUT = 32 640 text bytes."""
import gzip
import heapq
import os
import random
import subprocess
import zlib

import pytest

from bgzf_check import members, stream_text, strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases

pytestmark = pytest.mark.gpu

CUT = 32640
LENGTHS = [0, 1, CUT - 1, CUT, CUT + 1, 65279, 65280, 65281, 3 * CUT + 17, 3 * 65280 + 17, 8 << 20]


def _golden(name):
    return open(os.path.join(LAMBDA, name), "rb").read()


def _deflate_checked(data):
    """Two runs: identical bytes; members valid, one per CUT bytes, none larger than its text + 31; the text comes back."""
    import salt_amd
    assert salt_amd.BGZF_CUT == CUT
    out = salt_amd.bgzf_deflate(data)
    assert salt_amd.bgzf_deflate(data) == out, "two runs gave different bytes"
    ms = members(out)
    assert [len(t) for _, t in ms] == [min(CUT, len(data) - o) for o in range(0, len(data), CUT)]
    assert all(len(m) <= len(t) + 31 for m, t in ms)
    assert b"".join(t for _, t in ms) == data
    if data:
        assert gzip.decompress(out) == data
    else:
        assert out == b""
    return out, ms


def _huffman_depth(block):
    """Depth of the plain (not length-limited) Huffman tree over the byte counts of `block`."""
    counts = {}
    for b in block:
        counts[b] = counts.get(b, 0) + 1
    heap = [(c, 0) for c in counts.values()]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def _fibonacci_text(n_symbols, seed):
    fib = [1, 1]
    while len(fib) < n_symbols:
        fib.append(fib[-1] + fib[-2])
    text = bytearray(b"".join(bytes([65 + i]) * f for i, f in enumerate(fib)))
    random.Random(seed).shuffle(text)
    return bytes(text)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("src", ["expect_pe_default.sam", "expect_se_default.sam"])
def test_unit_sam_text_of_every_length(src, n):
    sam = _golden(src)
    data = (sam * (n // len(sam) + 1))[:n]
    out, _ = _deflate_checked(data)
    if n >= CUT:
        assert len(out) < n * 0.6


@pytest.mark.parametrize("n", [1, CUT, CUT + 1, 3 * CUT + 17])
def test_unit_zero_bytes(n):
    out, _ = _deflate_checked(bytes(n))
    assert len(out) < 64 + n // 20


@pytest.mark.parametrize("n", [1, 5, CUT - 1, CUT, CUT + 1, 3 * CUT + 17, 1 << 20])
def test_unit_random_bytes_leave_as_stored_blocks(n):
    data = random.Random(n).randbytes(n)
    out, ms = _deflate_checked(data)
    for m, t in ms:                                               # stored (BTYPE 0, the text itself behind 5 bytes), or no larger than that
        assert len(m) <= len(t) + 31
        if len(t) >= 1024:
            assert len(m) == len(t) + 31 and m[18] == 1 and m[23:-8] == t


def test_unit_two_symbol_text():
    r = random.Random(3)
    data = bytes(r.choice(b"ab") for _ in range(3 * CUT + 17))
    out, _ = _deflate_checked(data)
    assert len(out) < len(data) // 3


@pytest.mark.parametrize("n_symbols,cut_to", [(23, 65280), (21, None)])
def test_unit_counts_that_need_the_15_bit_limit(n_symbols, cut_to):
    """Byte counts that are Fibonacci numbers, shuffled with a fixed seed.  The first 23 numbers cut to 65 280 bytes: a plain Huffman tree
    over that text is deeper than 15 (checked here; 18 with this seed); at this block cut it leaves as two blocks.  The first 21 numbers (28 656 bytes) are ONE block
    whose plain tree is 20 deep (checked here): it inflates only if the code lengths are limited to deflate's 15 bits."""
    data = _fibonacci_text(n_symbols, 7)[:cut_to]
    if cut_to:
        assert len(data) == 65280 and _huffman_depth(data) > 15
    else:
        assert len(data) == 28656 <= CUT and _huffman_depth(data) == 20
    out, _ = _deflate_checked(data)
    assert len(out) < len(data) // 2


@pytest.mark.parametrize("src", ["expect_se_default.sam", "expect_pe_default.sam"])
def test_size_between_huffman_only_and_zlib_level_1(src):
    """D <= (H + L) / 2 over the same block cut: H = zlib with Z_HUFFMAN_ONLY (what a coder without matching reaches), L = zlib level 1
    (a chain of 4 candidates per position, probed one after the other; the kernel probes one), 26 bytes of container per block on both."""
    import salt_amd
    data = _golden(src)

    def zsize(strategy):
        total = 0
        for o in range(0, len(data), CUT):
            c = zlib.compressobj(1, zlib.DEFLATED, -15, 9, strategy)
            total += len(c.compress(data[o:o + CUT]) + c.flush()) + 26
        return total
    H, L = zsize(zlib.Z_HUFFMAN_ONLY), zsize(zlib.Z_DEFAULT_STRATEGY)
    D = len(salt_amd.bgzf_deflate(data))
    print("%s: text %d, D %d, H %d, L %d, gate %d" % (src, len(data), D, H, L, (H + L) // 2))
    assert D <= (H + L) / 2, (D, H, L)


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("lamidx") / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return prefix


def _run(cmd, env):
    out = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    return out


def _cli_case(cmd, want, envs):
    for env in envs:
        dev = _run(cmd, env)
        assert b"text path" in dev.stderr and b"[salt] BGZF output: device deflate, " in dev.stderr, dev.stderr[-600:]
        assert gzip.decompress(dev.stdout) == stream_text(dev.stdout)
        assert strip_pg(stream_text(dev.stdout)) == want
        host = _run(cmd, dict(env, SALT_BGZF_HOST="1"))
        assert b"[salt] BGZF output: host deflate, " in host.stderr, host.stderr[-600:]
        assert strip_pg(stream_text(host.stdout)) == want
    again = _run(cmd, envs[0])
    first = _run(cmd, envs[0])
    assert again.stdout == first.stdout, "two device runs gave different files"


@pytest.mark.parametrize("case", ["se_default", "se_r1_m500", "se_plain_t4"])
def test_cli_single_end_on_the_device(case, lambda_cli_index):
    salt = os.path.join(ROOT, "salt_amd", "bin", "salt")
    cmd = [salt] + read_cases()[case] + ["--bgzf", lambda_cli_index, os.path.join(LAMBDA, "reads_se.fq")]
    _cli_case(cmd, _golden("expect_%s.sam" % case), [dict(os.environ, SALT_CHUNK_BYTES="3001"), dict(os.environ, SALT_CHUNK_BYTES="70000")])


@pytest.mark.parametrize("case", ["pe_default", "pe_r5", "ragged_pe"])
def test_cli_paired_end_on_the_device(case, lambda_cli_index):
    salt = os.path.join(ROOT, "salt_amd", "bin", "salt")
    args, files = EXTRA_CASES[case] if case in EXTRA_CASES else (read_cases()[case], ["reads_pe_1.fq", "reads_pe_2.fq"])
    cmd = [salt] + args + ["--bgzf", lambda_cli_index] + [os.path.join(LAMBDA, f) for f in files]
    _cli_case(cmd, _golden("expect_%s.sam" % case), [dict(os.environ, SALT_CHUNK_BYTES="3000"), dict(os.environ)])


def test_cli_default_output_is_unchanged(lambda_cli_index):
    salt = os.path.join(ROOT, "salt_amd", "bin", "salt")
    out = _run([salt] + read_cases()["se_default"] + [lambda_cli_index, os.path.join(LAMBDA, "reads_se.fq")], dict(os.environ, SALT_CHUNK_BYTES="3001"))
    assert strip_pg(out.stdout) == _golden("expect_se_default.sam") and b"BGZF" not in out.stderr
