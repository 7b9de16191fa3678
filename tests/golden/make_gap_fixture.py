#!/usr/bin/env python3
"""Adds the gapped-pass fixture to tests/golden/lambda/ (run in the BUILD container only, after make_fixtures.py).

The other fixtures put their indels somewhere in the middle of 100-base reads.  Here every read has no gap-free hit by design and
the grid walks what the gapped pass of the aligner switches on: the read length (the Landau-Vishkin bound is L/10, the text window
L+4 bases of nibble-packed masks), the indel's size against that bound, and its position against the 8-base words of the windows.

Single end (-d -c): LENS x {insertion, deletion} x sizes {1, 2, 3, L/10-1, L/10, L/10+1} x POSITIONS, strands alternating from
read to read (both strands at every point for L < 64); every tenth read carries one extra (EXTRAS, in turn).  End reads: a 2-base deletion in the middle of a read whose
LV window pos+L+4 ends at the contig's / the genome's end -1, +0, +1 (the LV guard and the candidate rule's range filter differ
by one there), and reads starting at bases 0..2 of each contig.
Paired end (-d -p -c -a 300 -b 700): PE_LENS x {mate 1, mate 2, both} x {insertion, deletion} x sizes 1..4 x PE_POSITIONS (the
paired-end bound is 3: size 4 is left to the Smith-Waterman rescue).

Read names: g<i>_L<len>_<ins|del><size>_p<position>_<strand>_<contig>_<origin, 1-based>_<extra>.
Outputs, @PG line stripped, cut by length so that no file (before compression) outgrows the largest one the directory already
had, and gzipped like the directory's polish fixtures:
  reads_gap_se_{lane,mid,long}.fq.gz      expect_gap_se_{lane,mid,long}.sam.gz       L <= 129 / 130..168 / >= 170
  reads_gap_pe_{short,long}_[12].fq.gz    expect_gap_pe_{short,long}.sam.gz          mates <= 164 / >= 165
and tests/golden/lv_vectors_shapes.txt.gz: the unit vectors of `lvharness --shapes` (oracle/ref_harness.c), gzipped without a time stamp.
The script refuses to write unless the reference prints the same bytes under two MALLOC_PERTURB_ values and the fixture
holds the gapped records it is for (MIN_GAPPED per length, MIN_XA in all).
"""
import gzip
import os
import random
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import REF_BIN, OUT, K, revcomp, strip_pg      # noqa: E402
from make_span_fixture import contigs                             # noqa: E402

LENS = [40, 99, 100, 101, 119, 120, 128, 129, 130, 131, 139, 140, 160, 164, 165, 168, 170, 200, 300, 512]
SE_BANDS = (("se_lane", 0, 129), ("se_mid", 130, 168), ("se_long", 170, 512))
PE_LENS = [100, 150, 160, 164, 165, 168, 200, 250]
PE_BANDS = (("pe_short", 0, 164), ("pe_long", 165, 250))
PE_POSITIONS = lambda L: [1, 8, L // 2, L - 9, L - 2]             # noqa: E731
EXTRAS = ("sub", "snp", "insdel", "N")
SE_ARGS = ["-d", "-c"]
PE_ARGS = ["-d", "-p", "-c", "-a", "300", "-b", "700"]
MAX_FILE = 614911                 # the largest file of tests/golden/lambda before this fixture (expect_pe_default.sam)
MIN_GAPPED, MIN_XA = 40, 100
LV_SHAPES = (3000, 1)             # lvharness --shapes N SEED


def positions(L):
    return [0, 1, 2, 3, 7, 8, 9, L // 2, L - 9, L - 8, L - 3, L - 2, L - 1]


def sizes(L):
    out = []
    for s in (1, 2, 3, L // 10 - 1, L // 10, L // 10 + 1):
        if s >= 1 and s not in out:
            out.append(s)
    return out


class Sim:
    def __init__(self, rng):
        self.rng = rng
        self.genome = contigs(os.path.join(OUT, "genome.fa"))
        names = [n for n, _ in self.genome]
        self.snp = {}
        for line in open(os.path.join(OUT, "snps.txt")):
            c, p, al, ref = line.split()
            self.snp[(names.index(c), int(p) - 1)] = [a for a in al.split("/") if a != ref]

    def source(self, ci, pos, n, alt=False):
        """n bases of contig ci from pos: the reference's own bases (N replaced), or the listed other allele at every SNP site"""
        s = self.genome[ci][1]
        out = []
        for i in range(pos, pos + n):
            c = s[i] if 0 <= i < len(s) else "N"
            if alt and (ci, i) in self.snp:
                c = self.rng.choice(self.snp[(ci, i)])
            out.append(c if c in "ACGT" else self.rng.choice("ACGT"))
        return out

    def other(self, c):
        return self.rng.choice([x for x in "ACGT" if x != c])

    def edit(self, src, L, kind, size, p):
        """the read of L bases: src with `size` bases inserted before / deleted from read position p"""
        r = list(src)
        if kind == "ins":
            ins = [self.rng.choice("ACGT") for _ in range(size)]
            if p < len(r):
                ins[-1] = self.other(r[p])            # so the insertion cannot slide into a shorter one
            r[p:p] = ins
        else:
            del r[p:p + size]
        return r[:L]

    def read(self, L, kind, size, p, strand, extra, ci=None, pos=None):
        rng = self.rng
        if ci is None:
            ci = rng.randrange(len(self.genome))
        n_src = L + 2 * size + 8
        if pos is None:
            pos = rng.randrange(40, len(self.genome[ci][1]) - n_src - 40)
        src = self.source(ci, pos, n_src, alt=(extra == "snp"))
        r = self.edit(src, L, kind, size, p)
        if extra == "insdel":                          # the opposite edit of the same size 20 bases on: the diagonal returns
            q = p + 20 if p + 20 + size < L - 2 else p - 20
            if q >= 1:
                r = self.edit(r + src[L:L + size], L, "del" if kind == "ins" else "ins", size, q)
        if extra == "sub":                             # up to the bound where 1-3 substitutions reach it
            room = L // 10 - size
            for q in rng.sample(range(L), room if 1 <= room <= 3 else rng.randrange(1, 4)):
                r[q] = self.other(r[q])
        if extra == "N":
            r[rng.randrange(L)] = "N"
        r = "".join(r)
        name = "L%d_%s%d_p%d_%s_%s_%d_%s" % (L, kind, size, p, "-" if strand else "+", self.genome[ci][0], pos + 1, extra or "plain")
        return name, (revcomp(r) if strand else r)


def single_end(sim):
    reads = []                                         # (L, name, sequence)
    n = 0
    for L in LENS:
        for kind in ("ins", "del"):
            for size in sizes(L):
                for p in positions(L):
                    for strand in ((0, 1) if L < 64 else (n & 1,)):       # short reads: their size list collapses, so both strands
                        extra = EXTRAS[(n // 10) % 4] if n % 10 == 9 else None
                        name, r = sim.read(L, kind, size, p, strand, extra)
                        reads.append((L, "g%d_%s" % (n, name), r))
                        n += 1
    # end reads: the LV window [pos, pos+L+4) of a read with a 2-base deletion in the middle against the end of each contig (the
    # second one's is the genome's); and reads from bases 0..2 of each contig
    for ci, (_, s) in enumerate(sim.genome):
        for L in (100, 130, 170):
            for strand in (0, 1):
                for d in (-1, 0, 1):
                    pos = len(s) + d - (L + 4)
                    name, r = sim.read(L, "del", 2, L // 2, strand, None, ci, pos)
                    reads.append((L, "g%d_end%+d_%s" % (n, d, name), r))
                    n += 1
                for pos in (0, 1, 2):
                    name, r = sim.read(L, "del", 2, L // 2, strand, None, ci, pos)
                    reads.append((L, "g%d_start%d_%s" % (n, pos, name), r))
                    n += 1
    return reads


def paired_end(sim):
    rng = sim.rng
    pairs = []                                         # (L, name, mate 1, mate 2)
    n = 0
    for L in PE_LENS:
        for which in (1, 2, 3):
            for kind in ("ins", "del"):
                for size in (1, 2, 3, 4):
                    for p in PE_POSITIONS(L):
                        ci = rng.randrange(len(sim.genome))
                        s = sim.genome[ci][1]
                        isz = max(2 * L + 10, int(rng.gauss(500, 50)))
                        pos = rng.randrange(40, len(s) - isz - 60)
                        src1 = sim.source(ci, pos, L + 16)
                        src2 = sim.source(ci, pos + isz - L, L + 16)
                        m1 = sim.edit(src1, L, kind, size, p) if which & 1 else src1[:L]
                        m2 = sim.edit(src2, L, kind, size, p) if which & 2 else src2[:L]
                        r1, r2 = "".join(m1), revcomp("".join(m2))
                        if n & 1:
                            r1, r2 = r2, r1
                        name = "q%d_L%d_%s%d_p%d_m%d_%s_%s_%d_%d" % (n, L, kind, size, p, which, "-" if n & 1 else "+", sim.genome[ci][0], pos + 1, isz)
                        pairs.append((L, name, r1, r2))
                        n += 1
    return pairs


def reference_sam(idx, args, files, tmp):
    """the reference's SAM for these files, printed twice under two allocator fill patterns: equal or no fixture"""
    outs = []
    for perturb in ("165", "77"):
        sam = os.path.join(tmp, "o.sam")
        with open(sam, "w") as g:
            subprocess.run([os.path.join(REF_BIN, "salt")] + args + [idx] + files, check=True, stdout=g, stderr=subprocess.DEVNULL,
                           env=dict(os.environ, MALLOC_PERTURB_=perturb))
        strip_pg(sam, sam + ".nopg")
        outs.append(open(sam + ".nopg", "rb").read())
    if outs[0] != outs[1]:
        sys.exit("the reference's output for %s depends on uninitialised memory: no fixture written" % files)
    return outs[0]


def gapped_by_length(sam):
    """records of a SAM text whose own CIGAR has an I or D, counted by read length; and the records with an XA tag"""
    by_len, xa = {}, 0
    for line in sam.decode().split("\n"):
        if not line or line[0] == "@":
            continue
        t = line.split("\t")
        by_len.setdefault(len(t[9]), 0)
        if re.search("[ID]", t[5]):
            by_len[len(t[9])] += 1
        xa += any(x.startswith("XA:Z:") for x in t[11:])
    return by_len, xa


def lv_shapes():
    """oracle/_ref/lvharness --shapes (oracle/ref_harness.c on the reference's own Landau-Vishkin units), printed twice like the SAM"""
    cmd = [os.path.join(REF_BIN, "lvharness"), "--shapes"] + [str(x) for x in LV_SHAPES]
    outs = [subprocess.run(cmd, check=True, stdout=subprocess.PIPE, env=dict(os.environ, MALLOC_PERTURB_=p)).stdout for p in ("165", "77")]
    if outs[0] != outs[1]:
        sys.exit("lvharness --shapes depends on uninitialised memory: no fixture written")
    return gzip.compress(outs[0], compresslevel=9, mtime=0)


def main():
    sim = Sim(random.Random(20261018))
    se, pe = single_end(sim), paired_end(sim)
    files = {}                                         # file name -> bytes
    jobs = []                                          # (case, args, FASTQ names)
    for band, lo, hi in SE_BANDS:
        files["reads_gap_%s.fq" % band] = "".join("@%s\n%s\n+\n%s\n" % (nm, r, "I" * L) for L, nm, r in se if lo <= L <= hi).encode()
        jobs.append(("gap_" + band, SE_ARGS, ["reads_gap_%s.fq" % band]))
    for band, lo, hi in PE_BANDS:
        for m in (1, 2):
            files["reads_gap_%s_%d.fq" % (band, m)] = "".join("@%s/%d\n%s\n+\n%s\n" % (p[1], m, p[1 + m], "I" * p[0])
                                                              for p in pe if lo <= p[0] <= hi).encode()
        jobs.append(("gap_" + band, PE_ARGS, ["reads_gap_%s_%d.fq" % (band, m) for m in (1, 2)]))
    gapped, xa_total = {"se": {}, "pe": {}}, 0
    with tempfile.TemporaryDirectory() as tmp:
        idx = os.path.join(tmp, "idx")
        subprocess.run([os.path.join(REF_BIN, "salt-idx"), "-k", str(K), os.path.join(OUT, "genome.fa"), os.path.join(OUT, "snps.txt"), idx],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        for case, args, fqs in jobs:
            paths = []
            for f in fqs:
                paths.append(os.path.join(tmp, f))
                with open(paths[-1], "wb") as g:
                    g.write(files[f])
            sam = reference_sam(idx, args, paths, tmp)
            files["expect_%s.sam" % case] = sam
            by_len, xa = gapped_by_length(sam)
            for L, c in by_len.items():
                d = gapped["pe" if "-p" in args else "se"]
                d[L] = d.get(L, 0) + c
            xa_total += xa
            print("%-14s %5d records, %4d with an I or D, %4d with XA" % (case, sum(1 for l in sam.split(b"\n") if l and l[:1] != b"@"),
                                                                         sum(by_len.values()), xa))
    print("gapped records by length, single end:", sorted(gapped["se"].items()))
    print("gapped records by mate length, paired end:", sorted(gapped["pe"].items()))
    thin = [L for L in LENS if gapped["se"].get(L, 0) < MIN_GAPPED] + [L for L in PE_LENS if gapped["pe"].get(L, 0) < MIN_GAPPED]
    if thin:
        sys.exit("fewer than %d gapped records at lengths %s: no fixture written" % (MIN_GAPPED, thin))
    if xa_total < MIN_XA:
        sys.exit("only %d records with XA: no fixture written" % xa_total)
    files[os.path.join("..", "lv_vectors_shapes.txt.gz")] = lv_shapes()
    big = [f for f, b in files.items() if len(b) > MAX_FILE]
    if big:
        sys.exit("files over %d bytes: %s: no fixture written" % (MAX_FILE, big))
    for f, b in files.items():                         # gzipped without a time stamp: the same bytes from every run
        with open(os.path.join(OUT, f if f.endswith(".gz") else f + ".gz"), "wb") as g:
            g.write(b if f.endswith(".gz") else gzip.compress(b, compresslevel=9, mtime=0))
    print("wrote %d files, largest %d bytes" % (len(files), max(len(b) for b in files.values())))


if __name__ == "__main__":
    main()
