#!/usr/bin/env python3
"""Golden outputs of the reference's `polish` for the text entry point (run in the BUILD container only): oracle/_ref/polish on the inputs
of tests/polish_text_cases.py -- ragged read lengths, records with up to 1 000 XA items, one-rule parser cases.  Every input is run twice
(the outputs must agree) and must end with exit status 0.

  polish_text_ragged_*.sam.gz, polish_text_se_r5_s4_m16_lv.sam.gz   polish_input() of committed `salt` outputs
  polish_text_manyhits_in.sam.gz -> polish_text_manyhits_{se,sw,pe}.sam.gz
  polish_text_parse.json                                            the parser cases: arguments, input and output of each
(gzip without a time stamp: the same bytes whenever this runs)
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
POLISH = os.path.join(ROOT, "oracle", "_ref", "polish")
L = os.path.join(HERE, "lambda")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import polish_text_cases as ptc          # noqa: E402


def run(args, data):
    with tempfile.NamedTemporaryFile("wb", suffix=".sam", delete=False) as t:
        t.write(data)
    try:
        outs = []
        for _ in range(2):
            p = subprocess.run([POLISH] + list(args) + [os.path.join(L, "idx"), t.name], capture_output=True)
            assert p.returncode == 0, (args, p.returncode, p.stderr[-300:])
            outs.append(p.stdout)
        assert outs[0] == outs[1], "the reference's output changes from run to run"
        return outs[0]
    finally:
        os.unlink(t.name)


def main():
    for f in os.listdir(L):
        if f.startswith("polish_text_"):
            os.unlink(os.path.join(L, f))
    ptc.write_gz(ptc.MANY_IN, ptc.many_hits_input())
    parse = {}
    for exp, args, data in ptc.fixtures():
        out = run(args, data)
        if exp.startswith("polish_text_parse_"):
            parse[exp[len("polish_text_parse_"):-len(".sam")]] = {"args": list(args), "input": data.decode("latin-1"), "expect": out.decode("latin-1")}
        else:
            ptc.write_gz(exp, out)
        print(exp, args, len(data), "->", len(out), "bytes,", out.count(b"\n"), "records, NUL bytes", out.count(b"\0"))
    with open(os.path.join(L, ptc.PARSE), "w") as f:
        json.dump(parse, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
