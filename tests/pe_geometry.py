"""The designed paired-end fixture (tests/golden/make_pe_geometry_fixture.py): its files, its option rows, its class table, and the
census of the reference's SAM that the generator asserts before it writes and tests/test_pe_geometry_golden.py asserts again from the
committed files.  No GPU and no reference needed here."""
import collections
import gzip
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDA = os.path.join(HERE, "golden", "lambda")

# option row -> (salt arguments, min_tlen, max_tlen)
ROWS = {
    "a350": (["-d", "-p", "-c", "-a", "350", "-b", "650"], 350, 650),
    "a100": (["-d", "-p", "-c", "-a", "100", "-b", "460"], 100, 460),
}
READS = ["reads_pe_geom_1.fq", "reads_pe_geom_2.fq"]                # stored as <name>.gz, like the goldens (expect_pe_geom_<row>.sam.gz)
NOREF = ["reads_pe_geom_noref_1.fq", "reads_pe_geom_noref_2.fq"]
CLASSES = "pe_geom_classes.tsv"
LEN_A, LEN_B = 48502, 48502                       # lambdaA, lambdaB_div2pct
L_PAC = LEN_A + LEN_B
MIN_PER_ORDER = 4                                 # pairs of each class that must show the class's property, in either file order


def edge_lengths(row):
    """{designed template length: inside the window?} of a row's window-edge pairs."""
    _, lo, hi = ROWS[row]
    return {lo - 1: False, lo: True, lo + 1: True, hi - 1: True, hi: True, hi + 1: False}


# Rescue windows k_pair queues for a pair whose mates are, before pairing, as the class designs them: a random mate is unmapped, a
# damaged mate is unmapped on its own (the generator keeps only such damage), the other mate maps.  pairing_singleton tries one window
# per mapped mate, so such a pair has one; a pair of two random mates has none.  Classes that are absent here (two clean mates) queue
# zero or two windows depending on the alternative hits, which the class table does not say: test (d) leaves them out of its count.
WINDOWS_OF_CLASS = {"unmapped_both": 0}
for _c in (["start%d" % k for k in (0, 1, 7)] + ["end%d_%s" % (k, w) for k in (0, 1, 7) for w in ("damaged", "random")] +
           ["start_column", "boundary_rescue", "clip_head_fwd", "clip_tail_fwd", "clip_head_rev", "clip_tail_rev", "unmapped_fwd_anchor", "unmapped_rev_anchor"]):
    WINDOWS_OF_CLASS[_c] = 1


def golden(row):
    with gzip.open(os.path.join(LAMBDA, "expect_pe_geom_%s.sam.gz" % row), "rb") as f:
        return f.read()


def read_paths():
    """the gzipped FASTQ files (salt_amd.read_fastq reads them as they are)"""
    return [os.path.join(LAMBDA, f + ".gz") for f in READS]


def plain_reads(tmp_dir):
    """the FASTQ files unpacked into tmp_dir, for the command-line tools"""
    out = []
    for f, src in zip(READS, read_paths()):
        out.append(os.path.join(str(tmp_dir), f))
        with gzip.open(src, "rb") as g, open(out[-1], "wb") as dst:
            dst.write(g.read())
    return out


def class_table(path=None):
    """{pair name: (class, designed template length)}; noref pairs are listed too (their class starts with 'noref_')."""
    out = collections.OrderedDict()
    with open(path or os.path.join(LAMBDA, CLASSES)) as f:
        for line in f:
            name, cls, t = line.rstrip("\n").split("\t")
            out[name] = (cls, int(t))
    return out


def records(sam):
    """[(name, [fields of mate 1], [fields of mate 2])] of a paired SAM stream (bytes), headers and blank lines dropped."""
    rows = [l.split("\t") for l in sam.decode().split("\n") if l and not l.startswith("@")]
    assert len(rows) % 2 == 0
    out = []
    for i in range(0, len(rows), 2):
        assert rows[i][0] == rows[i + 1][0], (rows[i][0], rows[i + 1][0])
        out.append((rows[i][0], rows[i], rows[i + 1]))
    return out


def ref_span(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", cigar) if op in "MD")


def census(sam, table, row):
    """Counter of (property, file order) over the pairs of one golden SAM.  A pair name ends in _a (forward mate in file 1) or _b."""
    c = collections.Counter()
    edges = edge_lengths(row)
    for name, r1, r2 in records(sam):
        cls, t = table[name]
        order = name[-1]
        assert order in "ab", name
        f1, f2 = int(r1[1]), int(r2[1])
        mapped = not (f1 & 4) and not (f2 & 4)
        tl1, tl2 = int(r1[8]), int(r2[8])
        if cls.startswith("edge_") and cls.split("_")[1] == row and t in edges:
            shape = cls.split("_", 2)[2]
            if edges[t]:
                if mapped and (f1 & 2) and (f2 & 2) and abs(tl1) == t and abs(tl2) == t:
                    c[("tlen_%d" % t, order)] += 1
                    c[("tlen_%d_%s" % (t, shape), order)] += 1
            elif tl1 == 0 and tl2 == 0 and not (f1 & 2) and not (f2 & 2):
                c[("tlen0_%d" % t, order)] += 1
                c[("tlen0_%d_%s" % (t, shape), order)] += 1
        if cls == "altpair" and mapped and (f1 & 2) and r1[2] == r2[2] == "lambdaB_div2pct" and abs(tl1) == t and abs(tl2) == t:
            c[("paired_by_alternative_hits", order)] += 1
        if cls == "end_cross" and mapped and (f1 & 2) and any(int(r[4]) > 0 and r[2] == "lambdaB_div2pct" and
                                                               int(r[3]) - 1 + ref_span(r[5]) >= LEN_B - 1 for r in (r1, r2)):
            c[("rescued_at_the_genomes_end", order)] += 1               # the SNP-aware rescue (MAPQ from its scores) in a window clamped to l_pac
        if cls in ("FF", "RR") and mapped and (f1 & 2) and bool(f1 & 0x10) == bool(f1 & 0x20):
            c[("proper_same_strand", order)] += 1
        if any(r[6] not in ("=", "*") for r in (r1, r2)):
            c[("rnext_other_contig", order)] += 1
        if cls.startswith("clip_") and any("S" in r[5] for r in (r1, r2)):
            c[("soft_clip_rescued", order)] += 1
        for r, f in ((r1, f1), (r2, f2)):
            if f & 4:
                continue
            if r[2] == "lambdaA" and r[3] == "1":
                c[("pos_1", order)] += 1
            if r[2] == "lambdaB_div2pct" and int(r[3]) - 1 + ref_span(r[5]) == LEN_B:
                c[("last_base", order)] += 1
        if any((f & 0x18) == 0x18 for f in (f1, f2)):
            c[("mate_unmapped_self_reverse", order)] += 1
    return c


SHAPES = ("100x100", "75x150", "150x75")            # forward x reverse mate of the window-edge classes

# What the reference cannot be made to show (make_pe_geometry_fixture.py's docstring gives the reasons): (property, file order) pairs that
# the census does not ask for.
UNREACHABLE = {
    "a350": {("rescued_at_the_genomes_end", "b"), ("tlen0_651", "b")} | {("tlen0_651_%s" % s, "b") for s in SHAPES},
    "a100": {("rescued_at_the_genomes_end", "b"), ("tlen0_461", "b")} | {("tlen0_461_%s" % s, "b") for s in SHAPES} |
            {("tlen0_99_100x100", "a"), ("tlen0_99_100x100", "b"), ("tlen0_99_75x150", "b"), ("tlen_100_75x150", "b"), ("tlen_101_75x150", "b")},
}


def required(row):
    """[(property, file order, least count)]: MIN_PER_ORDER pairs per property, and of the window-edge properties at least one per mate shape
    as well (in_range uses the forward mate's length, the windows both)."""
    edge = ["tlen_%d" % t if inside else "tlen0_%d" % t for t, inside in sorted(edge_lengths(row).items())]
    keys = edge + ["paired_by_alternative_hits", "proper_same_strand", "rnext_other_contig", "soft_clip_rescued", "pos_1", "last_base",
                   "rescued_at_the_genomes_end", "mate_unmapped_self_reverse"]
    want = [(k, o, MIN_PER_ORDER) for k in keys for o in "ab"] + [("%s_%s" % (k, s), o, 1) for k in edge for s in SHAPES for o in "ab"]
    return [(k, o, n) for k, o, n in want if (k, o) not in UNREACHABLE[row]]


def check_census(sam, table, row):
    c = census(sam, table, row)
    short = {(k, o): c[(k, o)] for k, o, n in required(row) if c[(k, o)] < n}
    assert not short, (row, short)
    return c


def class_counts(sam, table):
    """{class: pairs in the SAM}"""
    return collections.Counter(table[name][0] for name, _, _ in records(sam))
