"""The pair form of the trimming rule's header (trim_pair_span of salt_amd/csrc/salt_trim_rule.h, what k_fq_trim_pair and
salt_trim_pair_span compile) run by the stand-alone tools/trim_pair_model.cc, plain and under AddressSanitizer + UBSan, every read in an
allocation of exactly its size: the spans and both counter arrays equal the Python statement of the rule (trim_pair_check.py) on the
edge-case set and on random pairs, and the run ends without a sanitizer report -- the proof of the rule's bounds that a GPU cannot give.
Nothing is loaded into Python under a sanitizer.  (The kernel itself: test_gpu_trim_pair.py.)"""
import os
import subprocess

import numpy as np
import pytest

import trim_pair_check as pc
from conftest import ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("trimpairmodel")
    src = os.path.join(ROOT, "tools", "trim_pair_model.cc")
    plain, san = str(d / "trim_pair_model"), str(d / "trim_pair_model.san")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", san, src], check=True)
    return plain, san, d


def _line(o, po, r1, r2):
    return "\t".join([o["adapter"] or "-", o["adapter2"] or "-", str(o["qual"]), str(o["front"]), str(o["tail"]), str(o["min_overlap"] if o["adapter"] else 0),
                      str(o["error_pct"] if o["adapter"] else 0), str(po["min_overlap"] if po else 0), str(po["error_pct"] if po else 0),
                      r1[0].hex(), r1[1].hex(), r2[0].hex(), r2[1].hex()]) + "\n"


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
    counts, pairs = np.zeros((2, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    want = "".join("%d %d %d %d\n" % pc.model_pair_span(o, po, r1, r2, counts, pairs) for o, po, r1, r2 in cases)
    want += " ".join(str(int(v)) for v in counts.reshape(-1)) + "\n" + " ".join(str(int(v)) for v in pairs) + "\n"
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
    _check(models, pc.edge_cases(), "edge.tsv")


def test_random_pairs_give_the_models_spans_and_end_clean(models):
    o, po, pairs = pc.random_pairs(2000, seed=5)
    _check(models, [(o, po, r1, r2) for r1, r2 in pairs], "random.tsv")


@pytest.mark.parametrize("line, word", [("-\t-\t0\t0\t0\t0\t0\t0\t5\t41\t49\t41\t49\n", "pair: min_overlap"), ("-\t-\t0\t0\t0\t0\t0\t513\t5\t41\t49\t41\t49\n", "pair: min_overlap"),
                                        ("-\t-\t0\t0\t0\t0\t0\t20\t51\t41\t49\t41\t49\n", "pair: error_pct"), ("-\t-\t94\t0\t0\t0\t0\t20\t10\t41\t49\t41\t49\n", "qual"),
                                        ("-\t-\t0\t0\t0\t0\t0\t20\t10\t4141\t49\t41\t49\n", "sequence or quality"), ("-\t-\t0\t0\t0\t0\t0\t20\t10\t41\t49\t\t\n", "sequence or quality"),
                                        ("-\t-\t0\t0\t0\n", "fields")])
def test_what_is_no_case_is_refused(models, line, word):
    plain, san, d = models
    path = str(d / "bad.tsv")
    with open(path, "w") as f:
        f.write(line)
    for exe in (plain, san):
        p = _run(exe, path)
        assert p.returncode == 2 and word in p.stderr.decode()
