"""The host twin of the SNP-site counts under AddressSanitizer + UBSan: tools/snp_counts_model.cc, a program of its own, built together with
salt_host.cc, runs salt_snp_sites and salt_snp_count_sam over the goldens -- whole, block by block and line by line, every
buffer ending where its text ends -- and over lines that are no SAM record.  Its tables must be the Python statement's (tests/snp_check.py)."""
import os
import subprocess

import pytest

import snp_check
from conftest import LAMBDA, ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("snpmodel")
    exe = str(d / "snp_counts_model.san")
    host = os.path.join(ROOT, "salt_amd", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tools", "snp_counts_model.cc"), os.path.join(host, "salt_host.cc"), "-lz", "-lpthread"], check=True)
    return exe


def _fnv(counts):
    h = 1469598103934665603
    for c in counts.reshape(-1):
        h = ((h ^ int(c)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("min_mapq", [0, 20])
def test_the_twin_over_the_goldens_under_sanitizers(min_mapq, model):
    names = sorted(snp_check.GOLDENS)
    p = subprocess.run([model, os.path.join(LAMBDA, "idx"), str(min_mapq)] + [os.path.join(LAMBDA, n) for n in names], capture_output=True, env=SAN_ENV, timeout=300)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-600:])
    out = p.stdout.decode().split("\n")
    assert out[len(names)] == "sites 3858" and out[len(names) + 1].startswith("refused ") and int(out[len(names) + 1].split()[1]) >= 10
    sites, _ = snp_check.sites_of_ref(os.path.join(LAMBDA, "idx.ref"))
    offsets = snp_check.contig_offsets(os.path.join(LAMBDA, "idx.C.ann"))
    for name, line in zip(names, out):
        want, n_rec = snp_check.count_sam(sites, offsets, snp_check.golden_sam(name), min_mapq)
        f = line.split(" ")
        got = dict(zip(f[1::2], map(int, f[2::2])))
        per_site = want.sum(axis=1)
        assert got == {"records": n_rec, "bases": int(want.sum()), "sites_hit": int((per_site > 0).sum()), "max": int(per_site.max()), "fnv": _fnv(want)}, name
        assert n_rec == snp_check.GOLDENS[name][0 if min_mapq == 0 else 1]
