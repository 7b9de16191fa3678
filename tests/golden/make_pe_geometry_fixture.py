#!/usr/bin/env python3
"""Adds the designed paired-end fixture to tests/golden/lambda/ (run in the BUILD container only, after make_fixtures.py).

The other paired-end fixtures hold one kind of pair: an FR fragment drawn inside one contig, insert sizes normal around the middle of the
window.  Here every pair is designed for a branch or a clamp of pairing2 / pairing_singleton / the SW rescue / alnpe_sam, and the real
reference (oracle/_ref/salt, `make -C oracle ref`) answers them under two option rows (tests/pe_geometry.py ROWS):
  edge_<row>_<l1>x<l2>  FR pairs of template length min_tlen-1, min_tlen, min_tlen+1, max_tlen-1, max_tlen, max_tlen+1 of that row;
                        mates of 100+100, 75+150 and 150+75 bases (forward + reverse mate)
  FF, RR, RF, far       both mates forward / both reverse / outward facing at a distance inside both windows; FR 5000 bases apart
  overlap1/50/full      mates overlapping by 1, by 50, completely (row a100: min_tlen below the mates' total length, min_isize 0)
  start0/1/7            fragment starting at base 0, 1, 7 of the genome, forward mate damaged: the reverse mate anchors a rescue whose window
                        start clamps to 0
  start_column          fragment of 200 bases at base 0, forward mate damaged: under row a350 the reverse anchor lies within min_isize of the
                        genome's start and the rescue window is the single column 0
  end0/1/7_damaged      fragment ending on the genome's last base, 1 and 7 before it, reverse mate damaged: the forward mate anchors a rescue
  end0/1/7_random       whose window end clamps (singleton branch: l_pac - 1); _random: the reverse mate is random bases
  boundary_split        one mate in lambdaA's last 300 bases, the other in lambdaB's first 300
  boundary_span_fwd/rev the forward / the reverse mate spans the contig boundary
  boundary_rescue       a damaged reverse mate whose rescue window spans the boundary
  cross_AB / cross_BA   forward mate cut from one copy, reverse mate from the matching place of the other: the primaries can lie 48 502 apart
  chimeric_same/other   both mates clean, 20 kb apart in one contig / in different contigs: the both-mapped rescue, both anchors tried
  clip_<head|tail>_<fwd|rev>  a damaged forward / reverse mate whose first / last 15 bases (genome orientation) are random: the rescue clips
  unmapped_both, unmapped_fwd_anchor, unmapped_rev_anchor   both mates random; one mate random beside a forward / a reverse anchor
  altpair               mates whose primaries cannot pair and whose alternative hits (in the other copy) are an FR pair inside both windows
  end_cross             the forward mate cut from lambdaB's last 440 bases (ending on the last base, 1 and 7 before it), the reverse mate from the
                        matching end of lambdaA: both map, in different copies, and the SNP-aware rescue finds the reverse mate at lambdaB's end,
                        in a both-mapped window whose end clamps to l_pac
  end_elsewhere         a clean forward mate 300 / 440 bases before the genome's end whose mate maps elsewhere: the both-mapped rescue window
                        (which finds nothing) has its end clamped to l_pac
  endchim               a clean forward mate within 250 bases of the genome's end whose mate maps 30 kb away.  pairing2 exit(1)s on a rescue
                        window that starts at or past l_pac (alnpe.c:266): a pair on which the reference exits under either row has no
                        golden, goes to reads_pe_geom_noref_[12].fq and is listed in the class table as noref_<class>: all twelve do
Damage is make_pairs' (9 % substitutions and a 2-base deletion; the mate keeps its length and its outer end by taking two more bases at its
inner end).  The 8 bases at a genome end are spared so that the rescued alignment can reach POS 1 / the last base.  Of several damaged
candidates the generator keeps the first that the reference leaves unmapped when its mate is random bases: a designed damaged mate is
unmapped on its own, so its pair takes pairing_singleton with exactly one rescue window (tests/pe_geometry.py WINDOWS_OF_CLASS).
Every design is written in both file orders (name suffix _a: the forward mate in file 1; _b: in file 2) at several positions.

Before anything is written the script asserts that the reference exits 0 on the golden pairs under both rows (each pair of a class that
can reach alnpe.c:266 is also run alone; one that makes the reference exit moves to the noref files) and the census of
tests/pe_geometry.py: per row and file order at least 4 pairs showing each property the classes are for, and at least one per mate
shape of every window-edge property.

What the reference cannot be made to show (tests/pe_geometry.py UNREACHABLE; the census does not ask for it):
  * TLEN 0 for template length max_tlen+1 with the forward mate in file 2 (both rows).  The pair is out of range, so pairing2 rescues from
    q[0], here the reverse mate: its window starts at pos - max_isize - l, one base inside the forward mate, the rescue returns 1S99M in
    place of the clean 100M, and alnpe_sam's template (sam.c:355-356, from the clipped row) is max_tlen - 1 or max_tlen: a proper pair.
    With the forward mate in file 1 the window's inclusive end covers the whole reverse mate and TLEN is 0 wherever the rescue returns it
    whole.
  * A result that depends on the order of a hit list: the alternative-hit loops `break` at the first hit past the window, which matters
    only for a mate with two alternative hits on one strand, i.e. a sequence with three copies.  The lambda genome has two.
  * Under row a100, TLEN 0 at template length 99 of 100-base mates: alnpe_sam prints 101 there (sam.c:356's arm for pos[0] >= pos[1]) and the
    pair is proper.  The 150+75 and 75+150 shapes show TLEN 0 at 99.
  * Under row a100, the low edge (99, 100, 101) of the 75+150 shape with the forward mate in file 2: q[0] is then the 150-base reverse mate,
    which the rescue returns as 125S25M, and sam.c:356 adds q[0].seq_end (149, an index into the read) without taking its seq_start off: 225.
  * The SNP-aware rescue in a window clamped to l_pac (end_cross) with the forward mate in file 2: pairing2 tries q[0]'s window first, here
    the reverse mate's in lambdaA, and finds the forward mate's copy there.  (The kernels still queue and run the clamped window.)
One thing the census counts differently from the design, because the reference does: under row a100 the low edge lies below the mates'
total length, min_isize is 0 and CHECK_IN_RANGE never accepts overlapping mates, so these pairs are all rescued or left as they are, and
TLEN comes from alnpe_sam alone -- template length 100 of 100-base mates prints -100 on both records (equal POS, `>=`), which the census
takes as |TLEN| = 100.
A both-mapped rescue window that ends at l_pac reads the allele mask at l_pac.  That nibble, like the three behind it in the last word of
<P>.ref, was never initialised: the index builder reallocs the array, clears and sets only the nibbles below l and writes the whole last
word (Index_src/mixRef.c:131-145; Align_src/metaref.c loads it as it is), so they hold whatever the heap held when the index was built: in
the committed idx.ref 0, 0, 0, 1, in the index this script builds something else.  Before
the goldens are made the script therefore answers every pair under both rows with each of the 16 values in those nibbles
(with_pad_nibbles); a pair whose records differ under any value moves to the noref files.  None does: the goldens do not depend on it.

Outputs: reads_pe_geom_[12].fq.gz, expect_pe_geom_a350.sam.gz, expect_pe_geom_a100.sam.gz (@PG stripped; gzipped like the gap fixture),
         reads_pe_geom_noref_[12].fq,
         pe_geom_classes.tsv (pair name, class, designed template length; 0 where the design has none).
"""
import gzip
import os
import random
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_fixtures import REF_BIN, OUT, K, revcomp, strip_pg               # noqa: E402
from make_span_fixture import contigs                                      # noqa: E402
import pe_geometry as pg                                                   # noqa: E402

N_CAND = 8                                         # damaged candidates per design
RISKY = ("end", "chimeric")               # classes whose pairs are also run alone (a forward anchor near the genome's end)


class Maker:
    def __init__(self, rng, genome):
        self.rng = rng
        self.cat = "".join(s for _, s in genome)
        self.la = len(genome[0][1])
        assert (self.la, len(self.cat)) == (pg.LEN_A, pg.L_PAC)
        self.snp = {}
        names = [n for n, _ in genome]
        for line in open(os.path.join(OUT, "snps.txt")):
            c, p, al, _ = line.split()
            self.snp[(self.la if names.index(c) else 0) + int(p) - 1] = al.split("/")
        self.pairs = []                            # [class, T, forward-design mate, other mate, order]  (reads as they go into the files)
        self.damaged = []                          # (index into pairs, which mate 0/1, [candidates])

    def cut(self, pos, n):
        """n genome bases from pos (forward strand) as a list: a SNP site takes one of its alleles, an N a random base."""
        assert 0 <= pos and pos + n <= len(self.cat), (pos, n)
        out = []
        for j in range(pos, pos + n):
            c = self.rng.choice(self.snp[j]) if j in self.snp else self.cat[j]
            out.append(c if c in "ACGT" else self.rng.choice("ACGT"))
        return out

    def junk(self, n):
        return [self.rng.choice("ACGT") for _ in range(n)]

    def damage(self, pos, n, inner_right, spare_head=0, spare_tail=0, clip=None):
        """The n bases at pos with 9 % substitutions and a 2-base deletion; two more bases come in at the inner end (the right end of a forward
        mate, the left end of a reverse mate), so the mate still covers pos .. pos+n-1 at its outer end.  clip: 'head' / 'tail' = 15 random bases."""
        rng = self.rng
        src = self.cut(pos, n + 2) if inner_right else self.cut(pos - 2, n + 2)
        for j in range(spare_head, len(src) - spare_tail):
            if rng.random() < 0.09:
                src[j] = rng.choice([c for c in "ACGT" if c != src[j]])
        p = rng.randrange(20, n - 20)
        del src[p:p + 2]
        first = pos if inner_right else pos - 2 + 2                    # after the deletion src[0] is pos (inner_right) or, at its tail, src[-1] is pos+n-1
        for j in range(spare_head):                                    # spared bases are the reference's own: no alternative allele either
            src[j] = self.cat[first + j]
        for j in range(spare_tail):
            src[-1 - j] = self.cat[pos + n - 1 - j]
        if clip == "head":
            src[:15] = self.junk(15)
        if clip == "tail":
            src[-15:] = self.junk(15)
        return src

    def add(self, cls, t, fwd, other, damaged=None):
        """fwd / other: base lists in read orientation; damaged = (which mate, function that draws a candidate in read orientation)."""
        for order in "ab":
            k = len(self.pairs)
            self.pairs.append([cls, t, "".join(fwd), "".join(other), order])
            if damaged is not None:
                which, draw = damaged
                self.damaged.append((k, which, ["".join(draw()) for _ in range(N_CAND)]))

    def fr(self, cls, pos, t, lf=100, lr=100):
        self.add(cls, t, self.cut(pos, lf), revcomp("".join(self.cut(pos + t - lr, lr))))


def design(m):
    la, lp, rng = m.la, pg.L_PAC, m.rng
    spots = [5000, 31000, la + 9000, la + 41000, 17000]               # fragment starts; clear of lambdaB's N hole (20000) and inversion (30000)
    for row in pg.ROWS:
        for lf, lr, n_spots in ((100, 100, 4), (75, 150, 4), (150, 75, 4)):
            for t in sorted(pg.edge_lengths(row)):
                for pos in spots[:n_spots]:
                    m.fr("edge_%s_%dx%d" % (row, lf, lr), pos + rng.randrange(50), t, lf, lr)
    for pos in spots:
        p, t = pos + 2000, 400
        a, b = m.cut(p, 100), m.cut(p + t - 100, 100)
        m.add("FF", t, a, b)
        m.add("RR", t, list(revcomp("".join(a))), list(revcomp("".join(b))))
        m.add("RF", t, list(revcomp("".join(a))), b)
        m.fr("far", pos - 3000, 5000)
        for cls, t in (("overlap1", 199), ("overlap50", 150), ("overlapfull", 100)):
            m.fr(cls, pos + 3000 + rng.randrange(50), t)
    t = 440
    for k in (0, 1, 7):
        for _ in range(8 if k == 0 else 4):
            rev = revcomp("".join(m.cut(k + t - 100, 100)))
            draw = lambda k=k: m.damage(k, 100, True, spare_head=8)
            m.add("start%d" % k, t, draw(), rev, damaged=(0, draw))
            e = lp - k
            fwd = m.cut(e - t, 100)
            draw = lambda e=e: list(revcomp("".join(m.damage(e - 100, 100, False, spare_tail=8))))
            m.add("end%d_damaged" % k, t, fwd, draw(), damaged=(1, draw))
            m.add("end%d_random" % k, t, m.cut(e - t, 100), m.junk(100))
    for _ in range(4):                                                 # the reverse anchor within min_isize (row a350) of base 0: a window of one column
        draw = lambda: m.damage(0, 100, True, spare_head=8)
        m.add("start_column", 200, draw(), revcomp("".join(m.cut(100, 100))), damaged=(0, draw))
    for d in (-40, -20, 0, 20, 40):
        m.fr("boundary_split", la - 250 + d, t)
        m.fr("boundary_span_fwd", la - 50 + d // 2, t)
        m.fr("boundary_span_rev", la - 450 + d // 2, t)
        pos = la - 400 + d
        draw = lambda pos=pos: list(revcomp("".join(m.damage(pos + t - 100, 100, False))))
        m.add("boundary_rescue", t, m.cut(pos, 100), draw(), damaged=(1, draw))
    for p in (5000, 12000, 25000, 36000, 44000):
        m.add("cross_AB", t, m.cut(p, 100), list(revcomp("".join(m.cut(la + p + t - 100, 100)))))
        m.add("cross_BA", t, m.cut(la + p, 100), list(revcomp("".join(m.cut(p + t - 100, 100)))))
    for p in (3000, 8000, 22000, la + 2000, la + 7000):                # forward anchors far more than max_tlen from the genome's end
        m.add("chimeric_same", 20100, m.cut(p, 100), list(revcomp("".join(m.cut(p + 20000, 100)))))
        q = p + 15000 + la if p < la else p + 15000 - la
        m.add("chimeric_other", 0, m.cut(p, 100), list(revcomp("".join(m.cut(q, 100)))))
    for pos in spots:
        p = pos + 6000
        for clip in ("head", "tail"):
            draw = lambda p=p, clip=clip: m.damage(p, 100, True, clip=clip)
            m.add("clip_%s_fwd" % clip, t, draw(), list(revcomp("".join(m.cut(p + t - 100, 100)))), damaged=(0, draw))
            draw = lambda p=p, clip=clip: list(revcomp("".join(m.damage(p + t - 100, 100, False, clip=clip))))
            m.add("clip_%s_rev" % clip, t, m.cut(p, 100), draw(), damaged=(1, draw))
        m.add("unmapped_both", 0, m.junk(100), m.junk(100))
        m.add("unmapped_fwd_anchor", 0, m.cut(p + 700, 100), m.junk(100))
        m.add("unmapped_rev_anchor", 0, m.junk(100), list(revcomp("".join(m.cut(p + 900, 100)))))
    # altpair: the only way into pairing2's alternative-hit loops that ends in a pair.  A hit list holds only hits as good as the primary, the
    # primary itself left out, so the 2 % copy is an alternative hit only where a read has the same number of differences in both copies; on a
    # tie the reverse-strand hit becomes the primary, then the lower position.  Mate 1 is a reverse read of a lambdaA window inside the stretch
    # that lambdaB holds inverted, free of differences: primary lambdaA reverse, alternative lambdaB forward.  Mate 2 is a reverse read of the
    # window that ends T bases downstream of that forward hit, with a third base wherever the copies differ: the same differences in both,
    # primary lambdaA reverse, alternative lambdaB reverse.  The primaries are both reverse and cannot pair; the alternatives are an FR pair of
    # template length T in lambdaB.  File order a pairs in the loops' first pass, b in the second.
    a_, b_ = m.cat[:la], m.cat[la:]
    for x in (30058, 30070, 30085, 30100, 30105):
        y = 60200 - x                                                  # lambdaB[30000:30300] is the reverse complement of the diverged copy
        assert revcomp(a_[x:x + 100]) == b_[y:y + 100]
        for t in range(360, 451):                                      # a template length inside both windows at which mate 2 can be made
            w = y + t - 100
            differ = [j for j in range(w, w + 100) if a_[j] != b_[j]]
            if w >= 30300 and len(differ) <= 2 and not any(j in m.snp or la + j in m.snp for j in differ):
                break
        else:
            raise AssertionError("no window for mate 2 of altpair at %d" % x)
        other = "".join(a_[j] if a_[j] == b_[j] else [c for c in "ACGT" if c not in (a_[j], b_[j])][0] for j in range(w, w + 100))
        m.add("altpair", t, list(revcomp(a_[x:x + 100])), list(revcomp(other)))
    for i, k in enumerate((0, 1, 7)):                                   # both mates map, the forward one at the genome's end: the both-mapped window clamps to l_pac
        m.add("end_elsewhere", 0, m.cut(lp - 440 - k, 100), list(revcomp("".join(m.cut(la + 12000 + 1000 * i, 100)))))
        m.add("end_elsewhere", 0, m.cut(lp - 300 - k, 100), list(revcomp("".join(m.cut(3000 + 1000 * i, 100)))))
    for k in (0, 0, 0, 0, 1, 7):                                       # the reverse mate from lambdaA's end: it maps there, and the rescue finds it in lambdaB
        m.add("end_cross", 440, m.cut(lp - 440 - k, 100), list(revcomp("".join(m.cut(la - 100 - k, 100)))))
    for i, k in enumerate((0, 1, 7, 60, 120, 149)):                    # mates at lambdaB 21000 .. 26000, clear of the N hole at 20000
        m.add("endchim", 0, m.cut(lp - 100 - k, 100), list(revcomp("".join(m.cut(la + 21000 + 1000 * i, 100)))))


def write_fastq(rng, pairs, names, p1, p2):
    with open(p1, "w") as f1, open(p2, "w") as f2:
        for (cls, t, fwd, other, order), name in zip(pairs, names):
            r1, r2 = (fwd, other) if order == "a" else (other, fwd)
            for f, r, k in ((f1, r1, 1), (f2, r2, 2)):
                f.write("@%s/%d\n%s\n+\n%s\n" % (name, k, r, "".join(chr(33 + rng.randrange(20, 41)) for _ in r)))


def run_ref(idx, args, p1, p2, out=None):
    with open(out or os.devnull, "w") as g:
        return subprocess.run([os.path.join(REF_BIN, "salt")] + args + [idx, p1, p2], stdout=g, stderr=subprocess.DEVNULL).returncode


def with_pad_nibbles(tmp, idx, v):
    """A copy of the index whose <P>.ref has the value v in the four nibbles behind the genome's last base (positions l_pac .. l_pac + 3 of the
    last word): the index builder never clears them (mixRef.c:131-143 clears below l and writes the whole last word), so they hold whatever
    the heap held, and a both-mapped rescue window that ends at l_pac reads the first of them."""
    d = os.path.join(tmp, "pad%d" % v)
    os.makedirs(d)
    for f in os.listdir(tmp):
        if f.startswith("idx.") and f != "idx.ref":
            os.symlink(os.path.join(tmp, f), os.path.join(d, f))
    words = bytearray(open(idx + ".ref", "rb").read())
    assert int.from_bytes(words[:4], "little") == pg.L_PAC and pg.L_PAC % 8 == 4 and len(words) == 4 * (1 + (pg.L_PAC + 7) // 8)
    last = int.from_bytes(words[-4:], "little") & 0xFFFF
    words[-4:] = (last | (v * 0x1111) << 16).to_bytes(4, "little")
    open(os.path.join(d, "idx.ref"), "wb").write(bytes(words))
    return os.path.join(d, "idx")


def main():
    rng = random.Random(20261019)
    genome = contigs(os.path.join(OUT, "genome.fa"))
    m = Maker(rng, genome)
    design(m)
    with tempfile.TemporaryDirectory() as tmp:
        idx = os.path.join(tmp, "idx")
        subprocess.run([os.path.join(REF_BIN, "salt-idx"), "-k", str(K), os.path.join(OUT, "genome.fa"), os.path.join(OUT, "snps.txt"), idx],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        a350 = pg.ROWS["a350"][0]
        # 1. of each damaged mate's candidates, the first that the reference leaves unmapped beside a random mate
        cand = [(k, which, c) for k, which, cs in m.damaged for c in cs]
        c1, c2, sam = (os.path.join(tmp, f) for f in ("c_1.fq", "c_2.fq", "c.sam"))
        write_fastq(rng, [["cand", 0, c, "".join(m.junk(100)), "a"] for _, _, c in cand], ["c%d" % i for i in range(len(cand))], c1, c2)
        assert run_ref(idx, a350, c1, c2, sam) == 0
        recs = pg.records(open(sam, "rb").read())
        assert len(recs) == len(cand)
        chosen = {}
        for (k, which, c), (_, r1, r2) in zip(cand, recs):
            if k not in chosen and int(r1[1]) & 4:
                assert int(r2[1]) & 4, "a random mate mapped"
                chosen[k] = (which, c)
        assert len(chosen) == len(m.damaged), "%d damaged mates map on their own in every candidate" % (len(m.damaged) - len(chosen))
        for k, (which, c) in chosen.items():
            m.pairs[k][2 + which] = c
        names = ["g%d_%s_%d_%s" % (i, p[0], p[1], p[4]) for i, p in enumerate(m.pairs)]
        # 2. pairs on which the reference exits (alnpe.c:266) have no golden
        def alone(i):
            if not m.pairs[i][0].startswith(RISKY):
                return True
            q1, q2 = os.path.join(tmp, "one_%d_1.fq" % i), os.path.join(tmp, "one_%d_2.fq" % i)
            write_fastq(random.Random(i), [m.pairs[i]], [names[i]], q1, q2)
            return all(run_ref(idx, pg.ROWS[row][0], q1, q2) == 0 for row in pg.ROWS)
        with ThreadPoolExecutor(8) as ex:
            ok = list(ex.map(alone, range(len(m.pairs))))
        for i, fine in enumerate(ok):
            if not fine:
                m.pairs[i][0] = "noref_" + m.pairs[i][0]
        # 3. pairs whose answer depends on the nibbles behind the genome's last base have none either: all 16 values are tried
        pads = [with_pad_nibbles(tmp, idx, v) for v in range(16)]
        g1, g2 = (os.path.join(tmp, f) for f in pg.READS)

        def answers(index, members):
            write_fastq(random.Random(7), [m.pairs[i] for i in members], [names[i] for i in members], g1, g2)
            out = []
            for row, (args, _, _) in pg.ROWS.items():
                raw = os.path.join(tmp, "pad_%s.sam" % row)
                assert run_ref(index, args, g1, g2, raw) == 0
                out.append({name: (r1, r2) for name, r1, r2 in pg.records(open(raw, "rb").read())})
            return out
        keep = [i for i, fine in enumerate(ok) if fine]
        for attempt in range(2):
            base = answers(pads[0], keep)
            fragile = set()
            for index in pads[1:]:
                for got, want in zip(answers(index, keep), base):
                    fragile |= {name for name in want if got[name] != want[name]}
            if not fragile:
                break
            assert attempt == 0, fragile
            print("depend on the nibbles behind the last base: %s" % sorted(fragile), file=sys.stderr)
            for i in keep:
                if names[i] in fragile:
                    ok[i] = False
                    m.pairs[i][0] = "noref_" + m.pairs[i][0]
            keep = [i for i in keep if ok[i]]
        gone = [i for i, fine in enumerate(ok) if not fine]
        assert len(gone) >= 2 * pg.MIN_PER_ORDER
        table = {names[i]: (m.pairs[i][0], m.pairs[i][1]) for i in range(len(names))}
        write_fastq(rng, [m.pairs[i] for i in keep], [names[i] for i in keep], g1, g2)
        sams = {}
        for row, (args, _, _) in pg.ROWS.items():
            raw = os.path.join(tmp, "raw_%s.sam" % row)
            assert run_ref(idx, args, g1, g2, raw) == 0, "the reference did not exit 0 under %s" % row
            strip_pg(raw, os.path.join(tmp, "expect_%s.sam" % row))
            sams[row] = open(os.path.join(tmp, "expect_%s.sam" % row), "rb").read()
            assert len(pg.records(sams[row])) == len(keep)
            c = pg.census(sams[row], table, row)
            for key in sorted(set(k for k, _ in c)):
                print("%s %-28s a %3d  b %3d" % (row, key, c[(key, "a")], c[(key, "b")]), file=sys.stderr)
        if sys.argv[1:]:                                               # a directory to look at the SAM in when the census fails
            for row in pg.ROWS:
                open(os.path.join(sys.argv[1], "raw_%s.sam" % row), "wb").write(sams[row])
        for row in pg.ROWS:
            pg.check_census(sams[row], table, row)
        # 4. all asserted: write
        for f, src in zip(pg.READS, (g1, g2)):                         # gzipped without a time stamp: the same bytes from every run
            with open(os.path.join(OUT, f + ".gz"), "wb") as g:
                g.write(gzip.compress(open(src, "rb").read(), compresslevel=9, mtime=0))
        write_fastq(rng, [m.pairs[i] for i in gone], [names[i] for i in gone], *(os.path.join(OUT, f) for f in pg.NOREF))
        for row in pg.ROWS:
            with open(os.path.join(OUT, "expect_pe_geom_%s.sam.gz" % row), "wb") as g:
                g.write(gzip.compress(sams[row], compresslevel=9, mtime=0))
        with open(os.path.join(OUT, pg.CLASSES), "w") as g:
            for i in keep + gone:
                g.write("%s\t%s\t%d\n" % (names[i], m.pairs[i][0], m.pairs[i][1]))
        for cls, n in sorted(pg.class_counts(sams["a350"], table).items()):
            print("%-28s %d pairs" % (cls, n), file=sys.stderr)
        print("noref: %d pairs" % len(gone), file=sys.stderr)


if __name__ == "__main__":
    main()
