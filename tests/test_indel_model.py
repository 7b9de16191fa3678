"""tools/indel_model.cc: the host twin of the indel table and its printer as a program of its own under AddressSanitizer + UBSan: the
goldens whole, block by block and line by line, the entries, every text and the header into buffers of exactly their size; the figures it
prints are the Python statement's (tests/indel_check.py).  No Python process loads the code that is checked, and nothing is preloaded."""
import os
import subprocess

import numpy as np
import pytest

import indel_check
from conftest import LAMBDA, ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
GOLDENS = ("expect_se_default.sam", "expect_pe_default.sam", "expect_span_default.sam", "expect_gap_se_lane.sam.gz", "expect_gap_se_mid.sam.gz", "expect_gap_se_long.sam.gz",
           "expect_gap_pe_short.sam.gz", "expect_gap_pe_long.sam.gz")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("indelmodel")
    exe = str(d / "indel_model.san")
    host = os.path.join(ROOT, "salt_amd", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tools", "indel_model.cc"), os.path.join(host, "salt_host.cc"), "-lz", "-lpthread"], check=True)
    return exe


def _fnv(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("floor", [0, 20, 255])
def test_the_twin_and_the_printer_over_the_goldens_under_sanitizers(floor, model):
    import snp_check
    genome = indel_check.Genome()
    p = subprocess.run([model, os.path.join(LAMBDA, "idx"), str(floor)] + [os.path.join(LAMBDA, n) for n in GOLDENS], capture_output=True, env=SAN_ENV, timeout=300)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-600:])
    out = p.stdout.decode().split("\n")
    assert out[len(GOLDENS)].startswith("refused ") and int(out[len(GOLDENS)].split()[1]) >= 15
    for name, line in zip(GOLDENS, out):
        table, stats, diff, n_rec = indel_check.add_sam(genome, snp_check.golden_sam(name), floor)
        pairs = indel_check.entries(table)
        f = line.split(" ")
        assert f[1:14] == ["records", str(n_rec), "stats"] + [str(x) for x in stats] + ["entries", str(len(pairs)), "efnv", str(_fnv(pairs.tobytes())), "dfnv", str(_fnv(diff.tobytes()))], name
        texts = [indel_check.text(genome, pairs, diff, a, p_) for a, p_ in ((1, 0), (2, 10), (3, 20))]
        head = indel_check.header(genome, floor, 3, 20, 0)
        assert f[14:] == [x for t in texts for x in ("text", str(len(t)), "tfnv", str(_fnv(t)))] + ["header", str(len(head)), "hfnv", str(_fnv(head))], name
        assert floor == 255 or (len(texts[0]) > 400 and np.asarray(pairs).size)      # (the smallest golden has seven alleles)
