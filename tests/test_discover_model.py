"""tools/discover_model.cc: the host twin of the SNP candidate arrays and its printer as a program of its own under AddressSanitizer +
UBSan: the goldens whole, block by block and line by line, every text into a buffer of exactly its size; the figures it prints are the
Python statement's (tests/disc_check.py)."""
import os
import subprocess

import pytest

import disc_check
import snp_check
from conftest import LAMBDA, ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("discmodel")
    exe = str(d / "discover_model.san")
    host = os.path.join(ROOT, "salt_amd", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tools", "discover_model.cc"), os.path.join(host, "salt_host.cc"), "-lz", "-lpthread"], check=True)
    return exe


def _fnv(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("floors", [(0, 0), (20, 20), (0, 30)])
def test_the_twin_and_the_printer_over_the_goldens_under_sanitizers(floors, model):
    genome = disc_check.Genome()
    names = sorted(snp_check.GOLDENS)
    p = subprocess.run([model, os.path.join(LAMBDA, "idx"), str(floors[0]), str(floors[1])] + [os.path.join(LAMBDA, n) for n in names], capture_output=True, env=SAN_ENV,
                       timeout=300)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-600:])
    out = p.stdout.decode().split("\n")
    assert out[len(names)].startswith("refused ") and int(out[len(names)].split()[1]) >= 12
    for name, line in zip(names, out):
        st = {}
        alt, diff, n_rec = disc_check.add_sam(genome, snp_check.golden_sam(name), floors[0], floors[1], st)
        f = line.split(" ")
        assert f[1:9] == ["records", str(n_rec), "events", str(st["counted"]), "afnv", str(_fnv(alt.tobytes())), "dfnv", str(_fnv(diff.tobytes()))], name
        texts = [disc_check.text(genome, alt, diff, a, p_, al) for a, p_ in ((1, 0), (2, 10), (3, 20)) for al in (False, True)]
        assert f[9:] == [x for t in texts for x in ("text", str(len(t)), "tfnv", str(_fnv(t)))], name
