"""The host twins of the coverage under AddressSanitizer + UBSan: tools/depth_model.cc, a program of its own, built together with
salt_host.cc, runs salt_depth_add_sam over the goldens -- whole, block by block and line by line, every buffer ending where its text
ends -- and salt_depth_text into buffers of exactly the text's size, then over lines that are no SAM record.  Its arrays and texts must be
the Python statement's (tests/depth_check.py)."""
import os
import subprocess

import numpy as np
import pytest

import depth_check
import snp_check
from conftest import LAMBDA, ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
WINDOWS = [1, 7, 64, 1000, 48502, 100000]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("depthmodel")
    exe = str(d / "depth_model.san")
    host = os.path.join(ROOT, "salt_amd", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tools", "depth_model.cc"), os.path.join(host, "salt_host.cc"), "-lz", "-lpthread"], check=True)
    return exe


def _wsum(data):
    """sum of (i + 1) * byte i, mod 2^64: the model's checksum"""
    b = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.uint64)
    return int((b * np.arange(1, len(b) + 1, dtype=np.uint64)).sum(dtype=np.uint64))


@pytest.mark.parametrize("min_mapq", [0, 20])
def test_the_twins_over_the_goldens_under_sanitizers(min_mapq, model):
    names = sorted(snp_check.GOLDENS)
    p = subprocess.run([model, os.path.join(LAMBDA, "idx"), str(min_mapq)] + [os.path.join(LAMBDA, n) for n in names], capture_output=True, env=SAN_ENV, timeout=300)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-600:])
    out = p.stdout.decode().split("\n")
    assert out[len(names)].startswith("refused ") and int(out[len(names)].split()[1]) >= 10
    contigs = depth_check.lambda_contigs()
    for name, line in zip(names, out):
        diff, n_rec = depth_check.diff_of_sam(contigs, snp_check.golden_sam(name), min_mapq)
        f = line.split(" ")
        assert f[1:5] == ["records", str(n_rec), "sum", str(_wsum(diff.astype("<u4").tobytes()))], name
        assert n_rec == snp_check.GOLDENS[name][0 if min_mapq == 0 else 1]
        texts = f[5:]
        for k, w in enumerate([0] + WINDOWS):
            want = depth_check.text_of(contigs, diff, w)
            assert texts[3 * k:3 * k + 3] == ["w%d" % w if w else "base", str(len(want)), str(_wsum(want))], (name, w)
