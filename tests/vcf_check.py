"""The rule of DESIGN.md 2.2 (SNP sites from a VCF) stated in Python, independently of the C++ per-line function the device's kernel and the
host twin share, and a builder of noisy VCF texts from a list of SNPs.  Shared by test_vcf_host.py and test_gpu_vcf.py."""
import hashlib
import os
import random
import struct
import zlib

import numpy as np

from conftest import GOLDEN, LAMBDA, ROOT

COUNTERS = ("lines", "kept", "sites", "unknown_contig", "out_of_range", "not_snv", "ref_mismatch", "filtered")
FIXTURES = {"lambda": LAMBDA}
for _c in ("two_contigs", "gap_short", "all_snp_contigs", "dense"):
    FIXTURES[_c] = os.path.join(GOLDEN, "index_cases", _c)
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
SEED_LEN = 19                   # what test_index_builder.py builds every fixture with
BIT = {65: 1, 67: 2, 71: 4, 84: 8}        # A C G T -> the mask bit
CODE = {65: 0, 67: 1, 71: 2, 84: 3}


class Malformed(Exception):
    def __init__(self, line):
        Exception.__init__(self, "line %d" % line)
        self.line = line


def read_fasta(path):
    """[(name up to the first white space, bytes of the bases)]"""
    out = []
    for l in open(path, "rb").read().splitlines():
        if l.startswith(b">"):
            out.append([l[1:].split()[0].decode(), bytearray()])
        elif out:
            out[-1][1] += l.strip()
    return [(n, bytes(s)) for n, s in out]


def read_snps(path):
    """the four-column SNP file: [(contig, 1-based pos, 'A/G', ref letter)]"""
    out = []
    for l in open(path).read().splitlines():
        c, p, al, r = l.split("\t")
        out.append((c, int(p), al, r))
    return out


def api_contigs(contigs):
    return [(n, np.frombuffer(s, dtype=np.uint8)) for n, s in contigs]


def model(contigs, text, pass_only=False, rename=None):
    """(groups, counters) of a VCF text under the rule: groups[i] = (name, positions, masks, ref codes) of contig i, ascending.
    Raises Malformed with the smallest 1-based number of a malformed line."""
    first = {}
    for i, (n, _) in enumerate(contigs):
        first.setdefault(n.encode(), i)
    rename = {a.encode(): b.encode() for a, b in (rename.items() if isinstance(rename, dict) else (rename or []))}
    sites = [dict() for _ in contigs]
    ct = dict.fromkeys(COUNTERS + ("first_unknown_line",), 0)
    bad = 0
    lines = bytes(text).split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                     # the text ended with its newline
    for no, l in enumerate(lines, 1):
        if l.endswith(b"\r"):
            l = l[:-1]
        if not l or l.startswith(b"#"):
            continue
        f = l.split(b"\t")
        if len(f) < 5 or not 1 <= len(f[1]) <= 10 or any(not 48 <= ch <= 57 for ch in f[1]):
            bad = bad or no
            continue
        ct["lines"] += 1
        chrom, pos, ref, alt = f[0], int(f[1]), f[3].upper(), f[4].upper()
        ci = first.get(rename.get(chrom, chrom))
        if ci is None:
            ct["unknown_contig"] += 1
            ct["first_unknown_line"] = ct["first_unknown_line"] or no
            continue
        seq = contigs[ci][1]
        if not 1 <= pos <= len(seq):
            ct["out_of_range"] += 1
            continue
        if len(ref) != 1 or ref[0] not in BIT:
            ct["not_snv"] += 1
            continue
        bits = 0
        for a in alt.split(b","):
            if len(a) == 1 and a[0] in BIT and a != ref:
                bits |= BIT[a[0]]
        if not bits:
            ct["not_snv"] += 1
            continue
        if seq[pos - 1:pos].upper() != ref:
            ct["ref_mismatch"] += 1
            continue
        if pass_only and len(f) >= 7 and f[6] not in (b"PASS", b"."):
            ct["filtered"] += 1
            continue
        ct["kept"] += 1
        sites[ci][pos - 1] = sites[ci].get(pos - 1, 0) | bits | BIT[ref[0]]
    if bad:
        raise Malformed(bad)
    groups = []
    for (n, seq), s in zip(contigs, sites):
        pos = sorted(s)
        groups.append((n, np.array(pos, dtype=np.uint32), np.array([s[p] for p in pos], dtype=np.uint8),
                       np.array([CODE[seq[p:p + 1].upper()[0]] for p in pos], dtype=np.uint8)))
        ct["sites"] += len(pos)
    return groups, ct


def same(a, b):
    """two (groups, counters) results are equal"""
    (ga, ca), (gb, cb) = a, b
    assert {k: ca[k] for k in cb} == cb and len(ga) == len(gb)
    for x, y in zip(ga, gb):
        assert x[0] == y[0]
        for u, v in zip(x[1:], y[1:]):
            assert np.array_equal(np.asarray(u), np.asarray(v)), x[0]
    return True


def snp_groups(contigs, snps):
    """what the SNP file says, as groups BY NAME: the expectation for a VCF built from it"""
    names = [n for n, _ in contigs]
    s = [dict() for _ in contigs]
    for c, p, al, r in snps:
        s[names.index(c)][p - 1] = (sum(BIT[ord(a)] for a in al.split("/")), CODE[ord(r)])
    return [(n, np.array(sorted(d), dtype=np.uint32), np.array([d[p][0] for p in sorted(d)], dtype=np.uint8),
             np.array([d[p][1] for p in sorted(d)], dtype=np.uint8)) for n, d in zip(names, s)]


def build_vcf(contigs, snps, seed=1, vcf_names=None, contig_order=None, extra_filtered=False):
    """A VCF text that holds exactly the sites of `snps` under the rule, with noise around them: header lines, shuffled lines, multi-allelic
    sites both split over lines and joined with commas, indel / MNP / <DEL> / * / . records, lower-case alleles, unknown contigs (one a prefix
    of a real name, one that a real name is a prefix of), a CRLF line, lines of 5 and 6 fields, an ALT of 5 000 bytes, a non-PASS FILTER, and a
    last line without its newline.  vcf_names: FASTA name -> the name the VCF uses.  contig_order: the records contig by contig in that
    order instead of shuffled.  extra_filtered: also non-PASS records at positions that are NO sites (for --vcf-pass-only tests)."""
    rnd = random.Random(seed)
    name = lambda c: (vcf_names or {}).get(c, c)
    seqs = dict(contigs)
    tail = "\t.\tPASS\tRS=1;VC=SNV"
    recs = []                                           # (FASTA contig, line without newline)
    for k, (c, p, al, r) in enumerate(snps):
        alts = [a for a in al.split("/") if a != r]
        assert alts and r in al.split("/") and seqs[c][p - 1:p].upper() == r.encode()
        low = (lambda x: x.lower()) if k % 5 == 0 else (lambda x: x)
        if len(alts) > 1 and k % 2 == 0:
            for a in alts:
                recs.append((c, "%s\t%d\trs%d\t%s\t%s%s" % (name(c), p, k, low(r), low(a), tail)))
        else:
            junk = ["", ",<DEL>", ",*", ",%sT" % r, ",N", ",."][k % 6]
            end = [tail, "", "\t50", "\t.\t.\tX", "\t9\tq10\tX"][k % 5]
            recs.append((c, "%s\t%d\t.\t%s\t%s%s%s" % (name(c), p, low(r), ",".join(low(a) for a in alts), junk, end)))
        if k % 7 == 0:                                  # noise beside it, all dropped: an indel, an MNP, symbolic and missing alleles, wrong names
            b = seqs[c][p - 1:p + 1].decode().upper()
            recs.append((c, "%s\t%d\t.\t%s\t%s%s" % (name(c), p, b, b[0], tail)))
            recs.append((c, "%s\t%d\t.\t%s\tAC,GT%s" % (name(c), p, b, tail)))
            recs.append((c, "%s\t%d\t.\t%s\t%s%s" % (name(c), p, r, ["<DEL>", "*", ".", "N", r][k // 7 % 5], tail)))
            recs.append((c, "%s1\t%d\t.\t%s\t%s%s" % (name(c), p, r, alts[0], tail)))
            if len(name(c)) > 1:
                recs.append((c, "%s\t%d\t.\t%s\t%s%s" % (name(c)[:-1], p, r, alts[0], tail)))
            recs.append((c, "chrUn_x\t%d\t.\t%s\t%s%s" % (p, r, alts[0], tail)))
    c, p, al, r = snps[0]
    a0 = [a for a in al.split("/") if a != r][0]
    recs.append((c, "%s\t%d\tlong\t%s\t%s,%s%s" % (name(c), p, r, a0 * 5000, a0, tail)))
    recs.append((c, "%s\t%d\tcrlf\t%s\t%s%s\r" % (name(c), p, r, a0, tail)))
    recs.append((c, "%s\t%d\tnotpass\t%s\t%s\t.\tq10;s50\tX" % (name(c), p, r, a0)))
    if extra_filtered:
        taken = {(c, p) for c, p, _, _ in snps}
        for c, seq in contigs:
            for p in range(1, len(seq) + 1, max(1, len(seq) // 7)):
                b = seq[p - 1:p].upper().decode()
                if (c, p) not in taken and b in "ACGT":
                    recs.append((c, "%s\t%d\t.\t%s\t%s\t3\tLowQual\tX" % (name(c), p, b, "ACGT"[("ACGT".index(b) + 1) % 4])))
    if contig_order:
        recs = [x for c in contig_order for x in recs if x[0] == c]
    else:
        rnd.shuffle(recs)
    head = "##fileformat=VCFv4.2\n##contig=<ID=%s>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" % name(contigs[0][0])
    lines = [x for _, x in recs]
    lines.insert(len(lines) // 2, "")                   # an empty line and a comment in the middle
    lines.insert(len(lines) // 3, "#late comment")
    return (head + "\n".join(lines)).encode()           # no newline behind the last line


def fixture(case):
    """(contigs, snps) of a committed genome.fa / snps.txt pair"""
    d = FIXTURES[case]
    return read_fasta(os.path.join(d, "genome.fa")), read_snps(os.path.join(d, "snps.txt"))


EDGE_CONTIGS = [("a", b"ACGTACGTNACGTACGTTGCA"), ("ab", b"GATTACAGATTACA"), ("b", b"C")]


def edge_texts():
    """name -> (text, the malformed line's number or None), all over EDGE_CONTIGS"""
    la = len(EDGE_CONTIGS[0][1])
    ok = "a\t2\t.\tC\tT\n"
    t = {
        "pos_1": ("a\t1\t.\tA\tG\n", None),
        "pos_len": ("a\t%d\t.\tA\tC\n" % la, None),
        "pos_len_plus_1": ("a\t%d\t.\tA\tC\n" % (la + 1), None),
        "pos_0": ("a\t0\t.\tA\tC\n" + ok, None),
        "pos_wraps_to_1": ("a\t4294967297\t.\tA\tG\n", None),
        "pos_ten_digits": ("a\t9999999999\t.\tA\tG\n" + ok, None),
        "pos_eleven_digits_and_12a": ("#h\n" + ok + "a\t12a\t.\tA\tG\n" + ok + "a\t12345678901\t.\tA\tG\n", 3),
        "pos_eleven_digits_first": (ok + ok + "a\t12345678901\t.\tA\tG\n" + "a\t12a\t.\tA\tG\n", 3),
        "pos_empty": ("a\t\t.\tA\tG\n", 1),
        "pos_signed": ("a\t+2\t.\tC\tT\n", 1),
        "four_fields": (ok + "\n" + "a\t3\t.\tG\n", 3),
        "four_fields_unknown_contig": ("zz\t3\t.\tG", 1),
        "ref_disagrees": ("a\t2\t.\tG\tT\n" + ok, None),
        "site_on_N": ("a\t9\t.\tA\tG\na\t9\t.\tN\tG\n", None),
        "contig_borders": ("a\t%d\t.\tA\tT\nab\t1\t.\tG\tC\nab\t14\t.\ta\tc,g,t\nb\t1\t.\tC\tA\n" % la, None),
        "prefix_names": ("ab\t2\t.\tA\tC\na\t2\t.\tC\tA\nabc\t2\t.\tA\tC\n\t2\t.\tA\tC\n", None),
        "empty": ("", None),
        "header_only": ("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n", None),
        "newlines_only": ("\n\r\n\n", None),
        "or_of_lines": ("a\t2\t.\tC\tT\na\t2\t.\tc\tg\na\t2\t.\tC\tA,C,<X>\n", None),
        "alt_shapes": ("a\t2\t.\tC\t\na\t2\t.\tC\t,\na\t3\t.\tG\t,A,\na\t4\t.\tT\tTA,*,.\na\t5\t.\tA\tC,\r\n", None),
        "filters": ("a\t2\t.\tC\tT\t.\tq10\na\t3\t.\tG\tT\t.\tPASS\na\t4\t.\tT\tA\t.\t.\na\t5\t.\tA\tC\t.\na\t6\t.\tC\tA\na\t7\t.\tG\tA\t.\t\tX\na\t8\t.\tT\tA\t.\tPASSED", None),
        "no_final_newline": (ok + "a\t3\t.\tG\tA", None),
    }
    return {k: (v[0].encode(), v[1]) for k, v in t.items()}


def bgzf(text, block=4000):
    """the text as BGZF blocks with the end-of-file block (SAM spec 4.1), made with zlib"""
    out = b""
    for at in range(0, len(text), block):
        t = text[at:at + block]
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        d = c.compress(t) + c.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(t), len(t))
    return out + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def same_index(prefix, d, sa_slack=1):
    """the comparison of test_index_builder.py: every file the reference wrote, except the spots where it writes memory it does not own"""
    for sfx in (".R.seedLen", ".C.pac", ".C.ann", ".C.amb", ".C.bwt", ".C.sa", ".lp", ".R.backward.bwt", ".R.backward.occ"):
        assert open(prefix + sfx, "rb").read() == open(os.path.join(d, "idx" + sfx), "rb").read(), sfx
    got, want = np.fromfile(prefix + ".R.backward.sa", dtype=np.uint32), np.fromfile(os.path.join(d, "idx.R.backward.sa"), dtype=np.uint32)
    assert len(got) == len(want) and int((got != want).sum()) <= sa_slack, int((got != want).sum())
    got, want = np.fromfile(prefix + ".ref", dtype=np.uint32), np.fromfile(os.path.join(d, "idx.ref"), dtype=np.uint32)
    assert len(got) == len(want) and got[0] == want[0] and (got[1:-1] == want[1:-1]).all()
    l = int(got[0])
    live = (1 << (4 * (l % 8))) - 1 if l % 8 else 0xFFFFFFFF
    assert (int(got[-1]) & live) == (int(want[-1]) & live)
    assert hashlib.sha256(open(prefix + ".C.lkt", "rb").read()).hexdigest() == open(os.path.join(d, "idx.C.lkt.sha256")).read().strip()


def same_dirs(a, b):
    for sfx in (".R.seedLen", ".C.pac", ".C.ann", ".C.amb", ".C.bwt", ".C.sa", ".C.lkt", ".lp", ".R.backward.bwt", ".R.backward.occ", ".R.backward.sa", ".ref"):
        assert open(a + sfx, "rb").read() == open(b + sfx, "rb").read(), sfx
