"""The trimming rule's header (salt_amd/csrc/salt_trim_rule.h, what k_fq_trim and salt_trim_span compile) run by tools/trim_model.cc, plain
and under AddressSanitizer + UBSan, every read in an allocation of exactly its size: the spans and the sixteen counters equal the Python
statement of the rule (trim_check.py) on the edge-case set and a random block, and the run ends without a sanitizer report -- the proof of
the rule's bounds that a GPU cannot give.  (The kernel itself: test_gpu_trim.py.)"""
import os
import subprocess

import numpy as np
import pytest

import trim_check as tc
from conftest import ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("trimmodel")
    src = os.path.join(ROOT, "tools", "trim_model.cc")
    plain, san = str(d / "trim_model"), str(d / "trim_model.san")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", san, src], check=True)
    return plain, san, d


def _line(o, mate, seq, qual):
    return "\t".join([str(mate), o["adapter"] or "-", o["adapter2"] or "-", str(o["qual"]), str(o["front"]), str(o["tail"]),
                      str(o["min_overlap"] if o["adapter"] else 0), str(o["error_pct"] if o["adapter"] else 0), seq.hex(), qual.hex()]) + "\n"


def _run(exe, path):
    p = subprocess.run([exe, path], capture_output=True, env=SAN_ENV, timeout=300)
    for word in (b"runtime error", b"AddressSanitizer", b"LeakSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    return p


def _check(models, cases, name):
    plain, san, d = models
    path = str(d / name)
    with open(path, "w") as f:
        f.writelines(_line(*c) for c in cases)
    counts = np.zeros((2, 8), dtype=np.uint64)
    want = "".join("%d %d\n" % tc.model_span(o, mate, s, q, counts) for o, mate, s, q in cases) + " ".join(str(int(v)) for v in counts.reshape(-1)) + "\n"
    for exe in (plain, san):
        p = _run(exe, path)
        assert p.returncode == 0, p.stderr[-300:]
        got = p.stdout.decode()
        if got != want:
            g, w = got.split("\n"), want.split("\n")
            bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
            raise AssertionError("%s: %d lines differ, first at case %d: got %r, want %r (%r)" % (os.path.basename(exe), len(bad), bad[0], g[bad[0]], w[bad[0]],
                                                                                                    cases[bad[0]] if bad[0] < len(cases) else "counters"))


def test_the_edge_cases_give_the_models_spans_and_end_clean(models):
    _check(models, tc.edge_cases(), "edge.tsv")


def test_a_random_block_gives_the_models_spans_and_ends_clean(models):
    o, reads = tc.random_block(3000, seed=5)
    _check(models, [(o, i & 1, s, q) for i, (s, q) in enumerate(reads)], "random.tsv")


@pytest.mark.parametrize("line, word", [("0\tACGN\t-\t0\t0\t0\t5\t10\t41\t49\n", "adapter holds"), ("0\t-\t-\t94\t0\t0\t0\t0\t41\t49\n", "qual"),
                                        ("0\t-\t-\t20\t0\t0\t0\t0\t4141\t49\n", "sequence or quality"), ("2\t-\t-\t20\t0\t0\t0\t0\t41\t49\n", "mate"),
                                        ("0\t-\t-\t20\t0\t0\t0\t0\t\t\n", "sequence or quality"), ("0\t-\t-\t20\n", "fields")])
def test_what_is_no_case_is_refused(models, line, word):
    plain, san, d = models
    path = str(d / "bad.tsv")
    with open(path, "w") as f:
        f.write(line)
    for exe in (plain, san):
        p = _run(exe, path)
        assert p.returncode == 2 and word in p.stderr.decode()
