"""The device's BGZF block algorithm (salt_amd/csrc/salt_bgzf_block.h) run on the host by tools/bgzf_model.cc, one thread of the workgroup
after the other: what it writes must inflate to its input, member by member, on a machine without a GPU.  (The kernels themselves:
test_gpu_bgzf.py.)"""
import gzip
import os
import random
import subprocess

import pytest

from bgzf_check import members
from conftest import LAMBDA, ROOT

CUT = 32640


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgzfmodel") / "bgzf_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tools", "bgzf_model.cc")], check=True)
    return exe


def _cases():
    r = random.Random(11)
    sam = open(os.path.join(LAMBDA, "expect_pe_default.sam"), "rb").read()
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    skew = bytearray(b"".join(bytes([65 + i]) * f for i, f in enumerate(fib)))      # 28 656 bytes: one block whose plain Huffman tree is 20 deep
    r.shuffle(skew)
    return {"sam": sam[:3 * CUT + 17], "one": b"x", "zeros": bytes(CUT + 1), "random": bytes(r.getrandbits(8) for _ in range(2 * CUT)),
            "two_symbols": bytes(r.choice(b"ab") for _ in range(CUT - 1)), "skewed": bytes(skew), "short": b"ACGT" * 31 + b"ACG"}


@pytest.mark.parametrize("name", sorted(_cases()))
def test_block_algorithm_on_the_host_inflates_to_its_input(name, model):
    data = _cases()[name]
    out = subprocess.run([model], input=data, capture_output=True, check=True).stdout
    assert gzip.decompress(out) == data
    ms = members(out)
    assert [len(t) for _, t in ms] == [min(CUT, len(data) - o) for o in range(0, len(data), CUT)]
    assert all(len(m) <= len(t) + 31 for m, t in ms)
    if name in ("sam", "zeros", "skewed", "two_symbols"):
        assert len(out) < len(data) // 2
