"""The per-record rules of `polish` over SAM text (salt_amd/csrc/salt_polish_text.h, the source the kernels of salt_polish.hip compile) run
on the host by tools/polish_text_model.cc, plain and under AddressSanitizer + UBSan.  For every fixture input the model's dump -- flag,
l_seq, the read's codes, the sorted unique hits per strand, the items with their windows -- equals an independent restatement of the
reference's strtok rules written below; damaged records (every prefix of a 13-hit record, that record with each tab and each digit
replaced by a random byte) give a dump or a status, the same the restatement gives, and never a sanitizer report -- the proof of the
parser's bounds rules that a GPU cannot give.  (The kernels themselves: test_gpu_polish_text.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import polish_text_cases as ptc
from conftest import LAMBDA, ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
ANN, PAC = os.path.join(LAMBDA, "idx.C.ann"), os.path.join(LAMBDA, "idx.C.pac")
K, MAX_READ = 13, 512


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("polishmodel")
    src = os.path.join(ROOT, "tools", "polish_text_model.cc")
    plain, san = str(d / "polish_text_model"), str(d / "polish_text_model.san")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", plain, src], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", san, src], check=True)
    return plain, san


# ---- the restatement: the reference's rules (samParser.c:84-190; polish.c:84-92, 466) over Python bytes ----
def contigs():
    lines = open(ANN).read().split("\n")
    l_pac, n = int(lines[0].split()[0]), int(lines[0].split()[1])
    return l_pac, {lines[1 + 2 * i].split()[1].encode(): int(lines[2 + 2 * i].split()[0]) for i in range(n)}


def genome():
    l_pac, _ = contigs()
    b = np.frombuffer(open(PAC, "rb").read(), dtype=np.uint8)
    return np.stack([(b >> 6) & 3, (b >> 4) & 3, (b >> 2) & 3, b & 3], axis=1).reshape(-1)[:l_pac]


def strtok(s, delim):
    return [x for x in s.split(delim) if x]                     # leading and repeated delimiters vanish


def c_number(b, signed):
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?)([0-9]*)", b)
    v, neg = int(m.group(2) or b"0"), m.group(1) == b"-"
    if signed:                                                  # atoi: through a long, cut to int
        v = max(-2 ** 63, -v) if neg else min(2 ** 63 - 1, v)
        v &= 0xFFFFFFFF
        return v - 2 ** 32 if v >= 2 ** 31 else v
    if v > 2 ** 64 - 1:                                         # strtoul saturates, whatever the sign
        return 0xFFFFFFFF
    return (-v if neg else v) & 0xFFFFFFFF


CODE = {c: i for i, c in enumerate(b"ACGT")}
CODE.update({c: i for i, c in enumerate(b"acgt")})


def restate(text, use_sw=False):
    """the model's output for `text`, keep-going mode: a list of lines"""
    l_pac, ctg = contigs()
    g = genome()
    out, recno, in_header = [], 0, True
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                             # behind the last newline there is no line
    for line in lines:
        if in_header and line[:1] == b"@":
            continue
        in_header = False
        if not line:
            break
        status, f = 0, strtok(line, b"\t")
        hits = ([], [])
        if len(f) < 11:
            status = 1
        elif len(f[9]) > MAX_READ:
            status = 3
        else:
            flag, seq = c_number(f[1], True), f[9]
            raw = []
            if not (flag & 4) and f[2] != b"*":
                raw.append((1 if flag & 0x10 else 0, f[2], c_number(f[3], False)))
            xa = [o for o in f[11:] if b"XA" in o][:1]
            ct = strtok(xa[0], b":") if xa else []
            multi = ct[2] if len(ct) >= 3 else b""
            while multi:
                semi = multi.find(b";")
                item = multi if semi < 0 else multi[:semi]
                if not item:
                    break
                c2 = strtok(item, b",")
                if len(c2) < 2:
                    break
                raw.append((0, c2[0], c_number(c2[1], False)) if c2[1][:1] != b"-" else (1, c2[0], c_number(c2[1][1:], False)))
                if semi < 0:
                    break
                multi = multi[semi + 1:]
            n_parsed = [sum(1 for h in raw if h[0] == s) for s in (0, 1)]
            for s, chrom, pos in raw:
                if chrom not in ctg:
                    status = 2
                    break
                hits[s].append((ctg[chrom] + pos - 1) & 0xFFFFFFFF)
        items = []
        if not status:
            uniq = [sorted(set(h)) for h in hits]
            L = len(seq)
            l_ref, buf, prev_full, dirty = L, np.zeros(MAX_READ, dtype=np.uint8), None, False
            for s in (0, 1):
                for off in uniq[s]:
                    if off > l_pac:
                        status = 4
                        break
                    if off + l_ref > l_pac:
                        l_ref = l_pac - off
                    if use_sw and l_ref == 0:
                        status = 8
                        break
                    win = None
                    if l_ref < L and not use_sw:                # the reference's buffer: written in place, stale behind the clip
                        if not dirty and prev_full is not None:
                            buf[:L] = g[prev_full:prev_full + L]
                        buf[:l_ref] = g[off:off + l_ref]
                        win, dirty = buf[:L].copy(), True
                    elif l_ref == L:
                        prev_full = off
                    items.append((off, l_ref, s, win))
                if status:
                    break
        if status:
            out.append("status %d record %d" % (status, recno))
        else:
            codes = [CODE.get(c, 4) for c in seq]
            if flag & 0x10:
                codes = [3 - c if c < 4 else c for c in reversed(codes)]
            out.append("R %d flag %d l_seq %d hits %d %d unique %d %d codes %s" % (recno, flag, L, n_parsed[0], n_parsed[1], len(uniq[0]), len(uniq[1]), "".join(map(str, codes))))
            out += ["H %d %d" % (s, off) for s in (0, 1) for off in uniq[s]]
            out += ["I %d %d %d %d %s" % (off, tl, s, win is not None, "-" if win is None else "".join(map(str, win))) for off, tl, s, win in items]
        recno += 1
    return out


def run_model(exe, text, tmp_path, use_sw=False):
    path = tmp_path / "in.sam"
    path.write_bytes(text)
    p = subprocess.run([exe] + (["-s"] if use_sw else []) + ["-k", ANN, PAC, str(path)], capture_output=True, env=SAN_ENV, timeout=300)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode in (0, 3), (p.returncode, p.stderr[-300:])
    l_pac, ctg = contigs()
    lines = []
    for l in p.stdout.decode("latin-1").split("\n")[:-1]:
        if l.startswith("H "):                                  # H <strand> <offset> <contig> <pos>: the name and position must give the offset
            _, s, off, name, pos = l.split(" ")
            assert (ctg[name.encode("latin-1")] + int(pos) - 1) & 0xFFFFFFFF == int(off)
            l = "H %s %s" % (s, off)
        lines.append(l)
    return p.returncode, lines


def fixture_inputs():
    d = {exp: (data, "-s" in args) for exp, args, data in ptc.fixtures()}
    d["polish_edge_in"] = (open(os.path.join(LAMBDA, "polish_edge_in.sam"), "rb").read(), False)
    d["polish_edge_in_sw"] = (d["polish_edge_in"][0], True)
    for name, (args, data) in ptc.no_golden_cases().items():
        d[name] = (data, False)
    return d


@pytest.mark.parametrize("name", sorted(fixture_inputs()))
def test_the_model_equals_the_restatement_on_every_fixture_input(name, models, tmp_path):
    data, use_sw = fixture_inputs()[name]
    want = restate(data, use_sw)
    assert len(want) > 2 and not any(l.startswith("status") for l in want)
    for exe in models:
        rc, got = run_model(exe, data, tmp_path, use_sw)
        assert rc == 0 and got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]


def test_the_edge_set_has_clipped_windows_with_stale_bytes(models, tmp_path):
    """the explicit pool windows are exercised at all: some item of the edge set carries one, and its bytes behind the clip are not all zero"""
    rc, got = run_model(models[0], open(os.path.join(LAMBDA, "polish_edge_in.sam"), "rb").read(), tmp_path)
    wins = [l.split(" ") for l in got if l.startswith("I ") and l.split(" ")[4] == "1"]
    assert len(wins) > 20 and any(set(w[5][int(w[2]):]) - {"0"} for w in wins)


def thirteen_hit_record():
    for l in ptc.edge_lines():
        if l.count(b";") == 12 and int(l.split(b"\t")[3]) < 30000:
            return l
    raise AssertionError("no record with 13 hits in the edge set")


def damaged_inputs(seed=5):
    rec = thirteen_hit_record()
    rng = np.random.default_rng(seed)
    prefixes = [rec[:n] for n in range(1, len(rec))]
    swapped = []
    for i, c in enumerate(rec):
        if c == 9 or 48 <= c <= 57:
            swapped.append(rec[:i] + bytes([int(rng.integers(0, 256))]) + rec[i + 1:])
    return prefixes, swapped


def test_damaged_records_give_a_dump_or_a_status_and_no_sanitizer_report(models, tmp_path):
    prefixes, swapped = damaged_inputs()
    assert len(prefixes) > 400 and len(swapped) > 150
    seen = set()
    for batch in (prefixes, swapped):
        text = b"\n".join(batch) + b"\n"
        want = restate(text)
        seen |= {l.split(" ")[1] for l in want if l.startswith("status")}
        assert any(l.startswith("R ") for l in want)
        for exe in models:
            rc, got = run_model(exe, text, tmp_path)
            assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]
            assert rc == (3 if any(l.startswith("status") for l in want) else 0)
    assert {"1", "2"} <= seen                                    # the malformed-record status and the unknown contig both occur


def test_the_committed_inputs_are_what_the_generators_make():
    """the goldens belong to these inputs: the parser cases' file and the many-hits input are the generators' bytes"""
    import gzip
    import json
    parse = json.load(open(os.path.join(LAMBDA, ptc.PARSE)))
    assert {k: (v["args"], v["input"].encode("latin-1")) for k, v in parse.items()} == {k: (list(a), d) for k, (a, d) in ptc.parser_cases().items()}
    assert gzip.open(os.path.join(LAMBDA, ptc.MANY_IN + ".gz"), "rb").read() == ptc.many_hits_input()
