"""Inputs for `polish` over text (test data generators, no product or oracle code): records with very many XA items, one- and two-record
parser cases, and the inputs the reference itself cannot run.  Used by tests/golden/make_polish_text_fixture.py (which runs the real
`polish` on them) and by the tests alike."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDA = os.path.join(HERE, "golden", "lambda")
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_polish_fixture import polish_input            # noqa: E402

HDR = b"@HD\tVN:1\n"
CONTIGS = ((b"lambdaA", 48502), (b"lambdaB_div2pct", 48502))
MANY = (63, 64, 65, 150, 1000)


def edge_lines():
    return [l for l in open(os.path.join(LAMBDA, "polish_edge_in.sam"), "rb").read().split(b"\n") if l and not l.startswith(b"@")]


def many_hits_input(seed=11):
    """Four records of polish_edge_in.sam whose primaries lie below position 30 000, each with 63, 64, 65, 150 and 1 000 XA items spread
    over both contigs and both strands; every fifth item lies within +-4 of the primary, so the offset sort meets equal offsets."""
    rng = np.random.default_rng(seed)
    base = [l for l in edge_lines() if int(l.split(b"\t")[3]) < 30000][:4]
    assert len(base) == 4
    out = []
    for b in base:
        f = b.split(b"\t")
        for n in MANY:
            items = []
            for k in range(n):
                if k % 5 == 4:
                    items.append(b"%s,%s%d,100M,1;" % (f[2], b"+-"[int(rng.integers(0, 2)):][:1], max(1, int(f[3]) + int(rng.integers(-4, 5)))))
                else:
                    cn, cl = CONTIGS[int(rng.integers(0, 2))]
                    items.append(b"%s,%s%d,100M,%d;" % (cn, b"+-"[int(rng.integers(0, 2)):][:1], int(rng.integers(1, cl - 400)), int(rng.integers(0, 4))))
            g = list(f[:11]) + [b"XA:Z:" + b"".join(items), b"MD:Z:100", b"NM:i:0"]
            g[0] = f[0] + b"_x%d" % n
            out.append(b"\t".join(g))
    return HDR + b"\n".join(out) + b"\n"


def _with_xa(lines, k):
    """the k-th record of the edge set that has at least three XA items and a forward or reverse primary clear of the genome end"""
    pick = [l for l in lines if b"XA:Z:" in l and l.count(b";") >= 3 and int(l.split(b"\t")[3]) < 30000]
    return pick[k]


def parser_cases():
    """name -> (polish arguments, input bytes): one or two records (three under -p) behind @HD, each bending one rule of the parser"""
    lines = edge_lines()
    r1, r2, r3 = _with_xa(lines, 0), _with_xa(lines, 1), _with_xa(lines, 2)
    f1 = r1.split(b"\t")
    xa = [x for x in f1 if x.startswith(b"XA:Z:")][0]
    rest = [x for x in f1 if not x.startswith(b"XA:Z:")]
    c = {}
    c["double_tabs"] = ([], HDR + r1.replace(b"\t", b"\t\t") + b"\n")
    c["xa_last_no_semicolon"] = ([], HDR + b"\t".join(rest + [xa.rstrip(b";")]) + b"\n")
    c["at_name"] = ([], HDR + r1 + b"\n" + b"@" + r2 + b"\n")
    c["lower_case"] = ([], HDR + b"\t".join(f1[:9] + [f1[9].lower()] + f1[10:]) + b"\n")
    c["flag4_with_pos"] = ([], HDR + b"\t".join([f1[0], b"%d" % (int(f1[1]) | 4)] + f1[2:]) + b"\n")
    c["chrom_star"] = ([], HDR + b"\t".join(f1[:2] + [b"*", b"0"] + f1[4:]) + b"\n")
    c["no_optional"] = ([], HDR + b"\t".join(f1[:11]) + b"\n" + b"\t".join(r2.split(b"\t")[:11]) + b"\n")
    c["empty_line"] = ([], HDR + r1 + b"\n\n" + r2 + b"\n")
    c["no_trailing_newline"] = ([], HDR + r1 + b"\n" + r2)
    c["no_header"] = ([], r1 + b"\n" + r2 + b"\n")
    c["three_records_pe"] = (["-p"], HDR + r1 + b"\n" + r2 + b"\n" + r3 + b"\n")
    c["crlf"] = ([], HDR + r1 + b"\r\n" + r2 + b"\r\n")
    return c


def no_golden_cases():
    """Inputs the reference itself dies on (segmentation fault), plus reads with N: the yardstick for these is the product's own host path."""
    lines = edge_lines()
    r1, r2 = _with_xa(lines, 0), _with_xa(lines, 1)
    f1 = r1.split(b"\t")
    xa = [x for x in f1 if x.startswith(b"XA:Z:")][0]
    rest = [x for x in f1 if not x.startswith(b"XA:Z:")]
    c = {}
    c["earlier_field_with_xa"] = ([], HDR + b"\t".join(f1[:11] + [b"RG:Z:XA1"] + f1[11:]) + b"\n" + r2 + b"\n")
    c["xa_no_semicolon_then_field"] = ([], HDR + b"\t".join(rest[:11] + [xa.rstrip(b";")] + rest[11:]) + b"\n" + r2 + b"\n")
    c["reads_with_n"] = ([], open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read())
    return c


RAGGED = (("polish_text_ragged_default_lv.sam", [], "expect_ragged_default.sam"), ("polish_text_ragged_default_sw.sam", ["-s"], "expect_ragged_default.sam"),
          ("polish_text_ragged_pe_lv.sam", ["-p"], "expect_ragged_pe.sam"), ("polish_text_ragged_pe_sw.sam", ["-p", "-s"], "expect_ragged_pe.sam"),
          ("polish_text_se_r5_s4_m16_lv.sam", [], "expect_se_r5_s4_m16.sam"))
MANY_RUNS = (("polish_text_manyhits_se.sam", []), ("polish_text_manyhits_sw.sam", ["-s"]), ("polish_text_manyhits_pe.sam", ["-p"]))
MANY_IN = "polish_text_manyhits_in.sam"
PARSE = "polish_text_parse.json"          # {case: {"args", "input", "expect"}}, bytes as latin-1 text: the inputs hold CR, empty lines, no final newline


def write_gz(name, data):
    """<name>.gz under tests/golden/lambda, the same bytes whenever it is written (no time stamp, no file name)"""
    with open(os.path.join(LAMBDA, name + ".gz"), "wb") as f, gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=f, mtime=0) as z:
        z.write(data)


def expected(name):
    """the committed bytes of the real `polish` for the fixture `name`: plain, gzipped, or an entry of the parser cases' one file"""
    m = name[len("polish_text_parse_"):-len(".sam")] if name.startswith("polish_text_parse_") else None
    if m is not None:
        return json.load(open(os.path.join(LAMBDA, PARSE)))[m]["expect"].encode("latin-1")
    path = os.path.join(LAMBDA, name)
    return open(path, "rb").read() if os.path.exists(path) else gzip.open(path + ".gz", "rb").read()


def fixtures():
    """[(name of the expected output, polish arguments, input bytes)] of every new golden; expected(name) has the committed bytes"""
    out = [(exp, args, polish_input(os.path.join(LAMBDA, src), "-p" in args)) for exp, args, src in RAGGED]
    many = gzip.open(os.path.join(LAMBDA, MANY_IN + ".gz"), "rb").read() if os.path.exists(os.path.join(LAMBDA, MANY_IN + ".gz")) else many_hits_input()
    out += [(exp, args, many) for exp, args in MANY_RUNS]
    out += [("polish_text_parse_%s.sam" % name, args, data) for name, (args, data) in sorted(parser_cases().items())]
    return out
