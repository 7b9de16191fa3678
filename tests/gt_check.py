"""Genotypes at the SNP sites: the third statement of the definition in include/salt_gpu.h, in Python, next to the device kernels
(salt_gt.hip) and the host twin (salt_gt_add_sam, salt_gt_text).  The penalty table from its formula, the events of a SAM text, the call
and the VCF record; Python integers throughout, so nothing here can wrap.  The tests compare the other two with it."""
import math
import os
import re

import numpy as np

import snp_check
from conftest import LAMBDA

Q_NONE = 20


def table():
    """(94, 3) penalties M, X, H per quality 0 .. 93 in 1 / 4096 Phred, from the formula"""
    rows = []
    for q in range(94):
        e = 10.0 ** (-min(max(q, 2), 60) / 10.0)
        rows.append([int(math.floor(-10.0 * math.log10(x) * 4096.0 + 0.5)) for x in (1.0 - e, e / 3.0, (1.0 - e) / 2.0 + e / 6.0)])
    return rows


def tie_margin():
    """how close any entry comes to a rounding tie"""
    worst = 1.0
    for q in range(94):
        e = 10.0 ** (-min(max(q, 2), 60) / 10.0)
        for x in (1.0 - e, e / 3.0, (1.0 - e) / 2.0 + e / 6.0):
            worst = min(worst, abs((-10.0 * math.log10(x) * 4096.0) % 1.0 - 0.5))
    return worst


TABLE = table()


class Genome:
    """what the call needs of an index prefix: the sites, their masks, the 2-bit genome and the contigs"""
    def __init__(self, prefix=os.path.join(LAMBDA, "idx")):
        self.sites, self.masks = snp_check.sites_of_ref(prefix + ".ref")
        lines = open(prefix + ".C.ann").read().split("\n")
        n = int(lines[0].split()[1])
        self.contigs = [(lines[1 + 2 * i].split()[1], int(lines[2 + 2 * i].split()[0]), int(lines[2 + 2 * i].split()[1])) for i in range(n)]      # name, offset, length
        self.offsets = {name: off for name, off, _ in self.contigs}
        pac = np.fromfile(prefix + ".C.pac", dtype=np.uint8)
        self.bases = ((pac[:, None] >> np.array([6, 4, 2, 0], dtype=np.uint8)) & 3).reshape(-1)      # base l = (pac[l >> 2] >> ((~l & 3) << 1)) & 3

    def contig_of(self, g):
        """the last contig that begins at or in front of g"""
        c = 0
        for k, (_, off, _) in enumerate(self.contigs):
            if off <= g:
                c = k
        return c


def add_sam(genome, sam, min_mapq=0, sums=None):
    """sums[site][base] = [n, sm, sx, sh] (Python integers) of the record lines of a SAM text, and the records that contributed"""
    site_of = {int(g): i for i, g in enumerate(genome.sites)}
    if sums is None:
        sums = [[[0, 0, 0, 0] for _ in range(4)] for _ in range(len(genome.sites))]
    n_rec = 0
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        if int(f[1]) & 4 or int(f[4]) < min_mapq:
            continue
        n_rec += 1
        g, s, seq, qual = genome.offsets[f[2].decode()] + int(f[3]) - 1, 0, f[9], f[10]
        no_qual = qual == b"*" and len(seq) != 1
        for n, op in re.findall(rb"(\d+)([MIDS])", f[5]):
            n = int(n)
            if op == b"M":
                for k in range(n):
                    b = b"ACGT".find(seq[s + k:s + k + 1])
                    if g + k in site_of and b >= 0:
                        byte = 0 if no_qual else qual[s + k]
                        q = byte - 33 if 33 <= byte <= 126 else Q_NONE
                        w = sums[site_of[g + k]][b]
                        w[0] += 1
                        for x in range(3):
                            w[1 + x] += TABLE[q][x]
                g, s = g + n, s + n
            elif op == b"D":
                g += n
            else:
                s += n
    return sums, n_rec


def as_array(sums):
    return np.array(sums, dtype=np.uint64).reshape(-1, 4, 4)


def call(mask, r, site):
    """the call of one site from its sums [base][n, sm, sx, sh]: dict with alleles, gt (i, j), pl list, gq, ad, dp, qual, raw"""
    alleles = [r] + [b for b in range(4) if (mask >> b) & 1 and b != r]
    n, sm, sx, sh = ([int(site[b][k]) for b in range(4)] for k in range(4))
    raw = []
    for j in range(len(alleles)):
        for i in range(j + 1):                                             # VCF order: j (j + 1) / 2 + i
            a, b = alleles[i], alleles[j]
            if i == j:
                raw.append(sm[a] + sum(sx[c] for c in range(4) if c != a))
            else:
                raw.append(sh[a] + sh[b] + sum(sx[c] for c in range(4) if c not in (a, b)))
    low = min(raw)
    k = raw.index(low)                                                     # the first of the smallest
    pl = [(x - low + 2048) >> 12 for x in raw]
    pairs = [(i, j) for j in range(len(alleles)) for i in range(j + 1)]
    return dict(alleles=alleles, gt=pairs[k], k=k, pl=pl, gq=min(99, min(p for x, p in enumerate(pl) if x != k)), ad=[n[a] for a in alleles], dp=sum(n),
                qual=pl[0], raw=raw)


def text(genome, sums, first=0):
    """the VCF records of sites [first, first + len(sums))"""
    out = []
    for i, site in enumerate(sums):
        g = int(genome.sites[first + i])
        c = call(int(genome.masks[g]), int(genome.bases[g]), site)
        name, off, _ = genome.contigs[genome.contig_of(g)]
        head = "%s\t%d\t.\t%s\t%s\t" % (name, g - off + 1, "ACGT"[c["alleles"][0]], ",".join("ACGT"[a] for a in c["alleles"][1:]))
        if c["dp"] == 0:
            out.append(head + ".\t.\tDP=0\tGT:AD:DP:GQ:PL\t./.:%s:0:.:.\n" % ",".join("0" for _ in c["alleles"]))
        else:
            out.append(head + "%d\t.\tDP=%d\tGT:AD:DP:GQ:PL\t%d/%d:%s:%d:%d:%s\n" % (c["qual"], c["dp"], c["gt"][0], c["gt"][1], ",".join(map(str, c["ad"])), c["dp"], c["gq"],
                                                                                 ",".join(map(str, c["pl"]))))
    return "".join(out).encode()


def header(genome, sample="sample"):
    lines = ["##fileformat=VCFv4.2", "##source=salt --genotype"]
    lines += ["##contig=<ID=%s,length=%d>" % (name, length) for name, _, length in genome.contigs]
    lines += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Bases of counted reads at the site (A, C, G, T)">',
              '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
              '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Bases that show each allele">',
              '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Bases of counted reads at the site (A, C, G, T)">',
              '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality: the smallest PL of another genotype, at most 99">',
              '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, flat priors, uncapped">',
              "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample]
    return ("\n".join(lines) + "\n").encode()


def hand_made(genome):
    """A sums table over all sites of an index that holds every case the call rule has, and what it holds: (sums as Python lists,
    census dict).  Site 0, the last site and the sites on both sides of every contig boundary carry sums; the rest is filled by a seeded
    pattern with sites of no depth in between."""
    n_sites = len(genome.sites)
    rng = np.random.RandomState(20261020)
    sums = [[[0, 0, 0, 0] for _ in range(4)] for _ in range(n_sites)]

    def events(site, base, q, times=1):
        w = sums[site][base]
        w[0] += times
        for x in range(3):
            w[1 + x] += TABLE[q][x] * times

    def info(s):
        g = int(genome.sites[s])
        return int(genome.masks[g]), int(genome.bases[g])

    for s in range(n_sites):                                               # the seeded body: depth 0 .. 40, mixed qualities, every base now and then
        if rng.randint(0, 8) == 0:
            continue
        mask, r = info(s)
        listed = [b for b in range(4) if (mask >> b) & 1]
        for _ in range(rng.randint(1, 41)):
            b = listed[rng.randint(0, len(listed))] if rng.randint(0, 10) else int(rng.randint(0, 4))
            events(s, b, int(rng.randint(0, 94)))
    by_alleles = {}
    for s in range(n_sites):
        mask, r = info(s)
        by_alleles.setdefault(len([r] + [b for b in range(4) if (mask >> b) & 1 and b != r]), []).append(s)
    edge = {0, n_sites - 1}
    for _, off, _ in genome.contigs[1:]:                                   # the sites on both sides of every contig boundary
        k = int(np.searchsorted(genome.sites, off))
        edge |= {max(k - 1, 0), min(k, n_sites - 1)}
    free = [s for s in by_alleles[2] if s not in edge]

    def clear(s):
        sums[s] = [[0, 0, 0, 0] for _ in range(4)]
        return info(s)

    def two(s):
        mask, r = clear(s)
        return r, [b for b in range(4) if (mask >> b) & 1 and b != r][0]

    it = iter(free)
    s_tie = next(it); r, a = two(s_tie)                                    # a tie: the same events on both alleles make 0/0 and 1/1 equal; 0/0 wins
    events(s_tie, r, 30, 3); events(s_tie, a, 30, 3)
    sums[s_tie][r][3] += 10 ** 7; sums[s_tie][a][3] += 10 ** 7             # (the het is out of the way)
    s_2047 = next(it); r, a = two(s_2047)                                  # raw differences of exactly 2047 and 2048 above the minimum: PL 0 and 1
    sums[s_2047][r] = [5, 1000, 50000, 40000]; sums[s_2047][a] = [5, 1000 + 2047, 50000, 40000]
    s_2048 = next(it); r, a = two(s_2048)
    sums[s_2048][r] = [5, 1000, 50000, 40000]; sums[s_2048][a] = [5, 1000 + 2048, 50000, 40000]
    s_gq = []
    for want in (98, 99, 100):                                             # GQ below, at and above 99: the runner-up's PL is `want`
        s = next(it); r, a = two(s)
        sums[s][r] = [9, 0, 10 ** 6, want * 4096]; sums[s][a] = [0, 10 ** 7, 0, 0]      # 0/0 raw 0, 0/1 raw want * 4096, 1/1 far off
        s_gq.append(s)
    s_zero = next(it); clear(s_zero)                                       # DP == 0
    s_out = next(it); r, a = two(s_out)                                    # bases outside the allele set
    outside = [b for b in range(4) if b not in (r, a)]
    events(s_out, r, 35, 12); events(s_out, outside[0], 20, 3); events(s_out, outside[1], 11, 2)
    s_big = next(it); r, a = two(s_big)                                    # sums above 2^32 (and a difference above 2^32)
    events(s_big, r, 2, 400000); events(s_big, a, 40, 300000)
    for s in sorted(edge):                                                 # the edges carry sums whatever the seed said
        if sum(sums[s][b][0] for b in range(4)) == 0:
            mask, r = info(s)
            events(s, r, 30, 7)
    census = dict(tie=s_tie, d2047=s_2047, d2048=s_2048, gq=s_gq, zero=s_zero, outside=s_out, big=s_big, edge=sorted(edge), by_alleles=by_alleles)
    return sums, census


def synth_index(directory):
    """A small index of three contigs whose sites have two, three and four alleles, with sites at position 0, at the genome's last
    position and on both sides of both contig boundaries: what the lambda index lacks for the call rule.  Returns the prefix."""
    import salt_amd
    from salt_amd import workload
    genome = workload.make_genome(6000, seed=9)
    rng = np.random.RandomState(9)
    bounds = workload.contig_bounds(len(genome), 3)
    pos = set(int(p) for p in rng.choice(len(genome), size=330, replace=False))
    pos |= {0, len(genome) - 1, bounds[1] - 1, bounds[1], bounds[2] - 1, bounds[2]}
    pos = np.array(sorted(pos), dtype=np.int64)
    ref = genome[pos].astype(np.int64)
    mask = (1 << ref) | (1 << ((ref + rng.randint(1, 4, size=len(pos))) & 3))
    kind = rng.randint(0, 10, size=len(pos))
    mask = np.where(kind == 0, mask | (1 << ((ref + rng.randint(1, 4, size=len(pos))) & 3)), mask)      # some of these are tri-allelic
    mask = np.where(kind == 1, 15, mask).astype(np.uint8)                                              # all four letters
    contigs, groups = workload.as_builder_input(genome, pos, mask, 3, name="gt")
    prefix = os.path.join(str(directory), "idx")
    salt_amd.idx_build_mem(contigs, groups, prefix, 20, flags=salt_amd.IDX_NO_LP)
    return prefix
