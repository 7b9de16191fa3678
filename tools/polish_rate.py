#!/usr/bin/env python3
"""Rate of `polish` and `polish -p`: another build's binary (--parent, e.g. the parent commit's) against this tree's device path, the same
input file through both, three runs each, alternating, output to /dev/null and once into a file, the two outputs compared with cmp (a
difference fails the run); then this binary's host path once, and `salt`'s own end-to-end rate in the same session for scale.
Input: the committed lambda inputs (polish_input of expect_se_default.sam / expect_pe_default.sam) repeated to --records records.
Writes --log (profiles/r10/polish_text.log).

  python tools/polish_rate.py --parent /path/to/parent/salt_amd/bin/polish
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_polish_fixture import polish_input          # noqa: E402

L = os.path.join(ROOT, "tests", "golden", "lambda")
BIN = os.path.join(ROOT, "salt_amd", "bin")


class Run:
    def __init__(self, args):
        self.a = args
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        self.logf = open(args.log, "w")
        self.dir = tempfile.mkdtemp()
        self.idx = os.path.join(self.dir, "idx")

    def log(self, *a):
        s = " ".join(str(x) for x in a)
        print(s, flush=True)
        self.logf.write(s + "\n")
        self.logf.flush()

    def make_input(self, src, paired, name):
        data = polish_input(os.path.join(L, src), paired)
        lines = data.split(b"\n")
        hdr = b"\n".join(l for l in lines if l.startswith(b"@")) + b"\n"
        body = b"\n".join(l for l in lines if l and not l.startswith(b"@")) + b"\n"
        n = body.count(b"\n")
        rep = (self.a.records + n - 1) // n
        path = os.path.join(self.dir, name)
        with open(path, "wb") as f:
            f.write(hdr)
            blob = body * 100
            for _ in range(rep // 100):
                f.write(blob)
            f.write(body * (rep % 100))
        return path, n * rep

    def timed(self, exe, args, path, env, out=None):
        t0 = time.perf_counter()
        with open(out or "/dev/null", "wb") as f:
            p = subprocess.run(["timeout", "-k", "10", "600", exe] + args + [self.idx, path], stdout=f, stderr=subprocess.PIPE, env=dict(os.environ, **env))
        dt = time.perf_counter() - t0
        if p.returncode != 0:
            self.log("STOP", exe, args, "rc", p.returncode, p.stderr[-400:])
            sys.exit(2)
        return dt, p.stderr.decode()[-300:].strip()

    def mode(self, name, args, src):
        new, old, log = os.path.join(BIN, "polish"), self.a.parent, self.log
        path, n = self.make_input(src, bool(args), "in_%d.sam" % len(args))
        log("== %s: %d records, %.1f MB" % (name, n, os.path.getsize(path) / 1e6))
        res = {"parent": [], "device": []}
        for r in range(3):
            for who, exe, env in (("parent", old, {}), ("device", new, {"SALT_POLISH_DEVICE": "1"})):
                dt, err = self.timed(exe, args, path, env)
                res[who].append(n / dt)
                log("  run %d %-7s %.2f s  %.3f Mrecords/s   %s" % (r, who, dt, n / dt / 1e6, err.split("\n")[-1][:200] if who == "device" and r == 0 else ""))
        dt, _ = self.timed(new, args, path, {"SALT_POLISH_HOST": "1"})
        log("  this binary, SALT_POLISH_HOST=1: %.2f s  %.3f Mrecords/s" % (dt, n / dt / 1e6))
        for who, v in res.items():
            log("  %-7s min %.3f median %.3f max %.3f Mrecords/s (spread %.3f)" % (who, min(v) / 1e6, sorted(v)[1] / 1e6, max(v) / 1e6, (max(v) - min(v)) / 1e6))
        fo, fn = os.path.join(self.dir, "old.out"), os.path.join(self.dir, "new.out")
        dto, _ = self.timed(old, args, path, {}, fo)
        dtn, _ = self.timed(new, args, path, {"SALT_POLISH_DEVICE": "1"}, fn)
        same = subprocess.run(["cmp", fo, fn]).returncode == 0
        log("  into a file: parent %.2f s (%.3f Mrecords/s), device %.2f s (%.3f Mrecords/s); cmp of the two outputs (%d bytes): %s"
            % (dto, n / dto / 1e6, dtn, n / dtn / 1e6, os.path.getsize(fn), "identical" if same else "DIFFERENT"))
        for f in (fo, fn, path):
            os.unlink(f)
        if not same:
            sys.exit(3)

    def salt_rate(self):
        """salt's own end-to-end rate in the same session: the lambda reads repeated, SAM to /dev/null"""
        fq = open(os.path.join(L, "reads_se.fq"), "rb").read()
        nr = fq.count(b"\n") // 4
        rep = (self.a.records + nr - 1) // nr
        fqp = os.path.join(self.dir, "reads.fq")
        with open(fqp, "wb") as f:
            for _ in range(rep):
                f.write(fq)
        t0 = time.perf_counter()
        p = subprocess.run(["timeout", "-k", "10", "600", os.path.join(BIN, "salt"), "-d", "-c", self.idx, fqp], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        dt = time.perf_counter() - t0
        self.log("== salt -d -c on %d lambda reads, SAM to /dev/null: rc %d, %.2f s wall, %.3f Mreads/s (start-up and index attach included)"
                 % (nr * rep, p.returncode, dt, nr * rep / dt / 1e6))
        self.log(p.stderr.decode()[-400:])
        os.unlink(fqp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the other build's polish binary")
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r10", "polish_text.log"))
    run = Run(ap.parse_args())
    p = subprocess.run(["timeout", "-k", "10", "120", os.path.join(BIN, "salt-idx"), "-k", "19", os.path.join(L, "genome.fa"), os.path.join(L, "snps.txt"), run.idx],
                       capture_output=True)
    if p.returncode:
        run.log("salt-idx failed", p.returncode)
        sys.exit(1)
    run.log("input: the committed lambda inputs (polish_input of expect_se_default.sam / expect_pe_default.sam) repeated to >= %d records; one GPU, 32-MiB blocks"
            % run.a.records)
    run.mode("polish", [], "expect_se_default.sam")
    run.mode("polish -p", ["-p"], "expect_pe_default.sam")
    run.salt_rate()


if __name__ == "__main__":
    main()
