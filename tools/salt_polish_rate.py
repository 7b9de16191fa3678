#!/usr/bin/env python3
"""Rate of the align-and-polish pipeline: the two-step run of another build (--parent, e.g. the parent commit's salt_amd/bin) -- `salt` into
a SAM file, then `polish` on that file, for pairs with the empty lines of `salt -p` filtered out in between, the filter's time counted --
against this tree's `salt --polish`, which prints the same records without the file.  Three runs each, alternating, output into a file and
once to /dev/null; the outputs of the two compared with cmp at the end (a difference fails the run).
Input: the committed lambda reads repeated to --reads reads (single end) and --reads / 2 pairs.  Writes --log (profiles/r11/salt_polish.log).

  python tools/salt_polish_rate.py --parent /path/to/parent/salt_amd/bin
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = os.path.join(ROOT, "tests", "golden", "lambda")
BIN = os.path.join(ROOT, "salt_amd", "bin")
LIMIT = ["timeout", "-k", "10", "300"]


class Run:
    def __init__(self, args):
        self.a = args
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        self.logf = open(args.log, "w")
        self.dir = tempfile.mkdtemp(dir=args.tmp)
        self.idx = os.path.join(self.dir, "idx")

    def log(self, *a):
        s = " ".join(str(x) for x in a)
        print(s, flush=True)
        self.logf.write(s + "\n")
        self.logf.flush()

    def repeat(self, src, n_reads, name):
        fq = open(os.path.join(L, src), "rb").read()
        nr = fq.count(b"\n") // 4
        rep = (n_reads + nr - 1) // nr
        path = os.path.join(self.dir, name)
        with open(path, "wb") as f:
            blob = fq * 20
            for _ in range(rep // 20):
                f.write(blob)
            f.write(fq * (rep % 20))
        return path, nr * rep

    def step(self, cmd, out, stdin=None):
        """one program of a pipeline step, under its own time limit; a failure ends the whole run"""
        t0 = time.perf_counter()
        with open(out, "wb") as f:
            p = subprocess.run(LIMIT + cmd, stdout=f, stderr=subprocess.PIPE, stdin=stdin)
        dt = time.perf_counter() - t0
        if p.returncode != 0:
            self.log("STOP", cmd, "rc", p.returncode, p.stderr[-400:])
            sys.exit(2)
        return dt

    def two_step(self, args, files, paired, out):
        sam, flt = os.path.join(self.dir, "f.sam"), os.path.join(self.dir, "f.flt.sam")
        t = [self.step([os.path.join(self.a.parent, "salt")] + args + [self.idx] + files, sam)]
        src = sam
        if paired:                                               # `polish` ends its input at the first empty line: they have to go
            t.append(self.step(["grep", "-v", "^$", sam], flt))
            src = flt
        t.append(self.step([os.path.join(self.a.parent, "polish")] + (["-p"] if paired else []) + [self.idx, src], out))
        size = os.path.getsize(sam)
        for f in (sam, flt):
            if os.path.exists(f):
                os.unlink(f)
        return t, size

    def mode(self, name, args, files, n, paired):
        log = self.log
        log("== %s: %d reads, %.1f MB of FASTQ" % (name, n, sum(os.path.getsize(f) for f in files) / 1e6))
        fo, fn = os.path.join(self.dir, "two_step.out"), os.path.join(self.dir, "fused.out")
        res = {"two-step": [], "fused": []}
        for r in range(3):
            t, size = self.two_step(args, files, paired, fo)
            res["two-step"].append(n / sum(t))
            log("  run %d two-step %.2f s = %s  %.3f Mreads/s  (SAM in between: %.1f MB)" % (r, sum(t), " + ".join("%.2f" % x for x in t), n / sum(t) / 1e6, size / 1e6))
            dt = self.step([os.path.join(BIN, "salt"), "--polish"] + args + [self.idx] + files, fn)
            res["fused"].append(n / dt)
            log("  run %d fused    %.2f s  %.3f Mreads/s" % (r, dt, n / dt / 1e6))
        for who, v in res.items():
            log("  %-8s min %.3f median %.3f max %.3f Mreads/s (spread %.3f)" % (who, min(v) / 1e6, sorted(v)[1] / 1e6, max(v) / 1e6, (max(v) - min(v)) / 1e6))
        lo, hi = sorted(res["two-step"]), sorted(res["fused"])
        log("  the ranges %s" % ("overlap: the difference is inside the spread of the three runs" if lo[0] <= hi[2] and hi[0] <= lo[2] else "do not overlap"))
        dt = self.step([os.path.join(BIN, "salt"), "--polish"] + args + [self.idx] + files, "/dev/null")
        log("  fused, output to /dev/null: %.2f s  %.3f Mreads/s" % (dt, n / dt / 1e6))
        same = subprocess.run(["cmp", fo, fn]).returncode == 0
        log("  cmp of the two outputs (%d bytes): %s" % (os.path.getsize(fn), "identical" if same else "DIFFERENT"))
        for f in (fo, fn):
            os.unlink(f)
        if not same:
            sys.exit(3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the other build's salt_amd/bin directory (salt and polish)")
    ap.add_argument("--reads", type=int, default=4000000)
    ap.add_argument("--tmp", default=None, help="where the inputs and the SAM file in between are written")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "r11", "salt_polish.log"))
    run = Run(ap.parse_args())
    p = subprocess.run(LIMIT + [os.path.join(BIN, "salt-idx"), "-k", "19", os.path.join(L, "genome.fa"), os.path.join(L, "snps.txt"), run.idx], capture_output=True)
    if p.returncode:
        run.log("salt-idx failed", p.returncode)
        sys.exit(1)
    run.log("input: the committed lambda reads repeated; one GPU; wall time of whole programs, start-up and index attach included in every one")
    se, n = run.repeat("reads_se.fq", run.a.reads, "reads.fq")
    run.mode("single end", [], [se], n, False)
    os.unlink(se)
    m1, n1 = run.repeat("reads_pe_1.fq", run.a.reads // 2, "reads_1.fq")
    m2, _ = run.repeat("reads_pe_2.fq", run.a.reads // 2, "reads_2.fq")
    run.mode("paired end", ["-p", "-a", "350", "-b", "650"], [m1, m2], 2 * n1, True)


if __name__ == "__main__":
    main()
