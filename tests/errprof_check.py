"""The error profile: the third statement of the rule, in Python, next to the device kernel (salt_errprof.hip) and the host twin
(salt_errprof_add_sam, salt_errprof_text).  Written from the definition in include/salt_gpu.h: the .ref file decoded, the SAM parsed, the
CIGAR walked, the file printed.  The tests compare the other two with it, use census() to show that a golden exercises what it is said
to, and read `salt --error-profile`'s file back with parse_file()."""
import math
import os
import re

import numpy as np

import snp_check
from conftest import LAMBDA

SHAPE = (2, 512, 95, 4, 4)                  # E[mate][cycle][q][ref][read]
NONE = 94
NT = "ACGT"


def lambda_masks():
    """the 4-bit mixRef masks of the lambda index, one per genome position"""
    return snp_check.sites_of_ref(os.path.join(LAMBDA, "idx.ref"))[1]


def lambda_offsets():
    return snp_check.contig_offsets(os.path.join(LAMBDA, "idx.C.ann"))


def tables_of_sam(masks, offsets, sam, min_mapq=0, tables=None, stats=None):
    """(E, R, records that counted) of the record lines of a SAM text.  stats (a dict) gets the census: base events, mismatches, M
    columns masked (site or genome N), M columns with a read N, the set of q seen, the largest cycle."""
    E, R = tables if tables is not None else (np.zeros(SHAPE, dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64))
    ref_len = len(masks)
    n_rec = 0
    st = stats if stats is not None else {}
    for k in ("events", "mismatches", "masked", "read_n", "max_cycle"):
        st.setdefault(k, 0)
    st.setdefault("q", set())
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        flag, mapq = int(f[1]), int(f[4])
        mate = 1 if flag & 0x80 else 0
        R[mate, 0] += 1
        if flag & 4:
            R[mate, 2] += 1
            continue
        if mapq < min_mapq:
            R[mate, 3] += 1
            continue
        n_rec += 1
        rev = bool(flag & 0x10)
        seq, qual = f[9], f[10]
        L = len(seq)
        no_qual = qual == b"*" and L != 1
        R[mate, 4] += 1
        R[mate, 5] += rev
        R[mate, 6] += bool(re.search(rb"[IDS]", f[5]))
        g, s = offsets[f[2].decode()] + int(f[3]) - 1, 0
        for n, op in re.findall(rb"(\d+)([MIDS])", f[5]):
            n = int(n)
            if op == b"D":
                g += n
            elif op != b"M":
                s += n
            else:
                for _ in range(n):
                    if g < ref_len and s < L:
                        m = int(masks[g])
                        b = NT.find(chr(seq[s]))
                        if b < 0:
                            st["read_n"] += 1
                        elif m == 0 or m & (m - 1):
                            st["masked"] += 1
                        else:
                            c = m.bit_length() - 1
                            q = NONE if no_qual or not 33 <= qual[s] <= 126 else qual[s] - 33
                            cycle = L - 1 - s if rev else s
                            E[mate, cycle, q, 3 - c if rev else c, 3 - b if rev else b] += 1
                            st["events"] += 1
                            st["mismatches"] += b != c
                            st["q"].add(q)
                            st["max_cycle"] = max(st["max_cycle"], cycle)
                    g, s = g + 1, s + 1
    return E, R, n_rec


def margins(E):
    """(Q[mate][q] = (bases, mismatches), C[mate][cycle] = (bases, mismatches), S[mate][ref][read]) as integer arrays"""
    off = np.ones((4, 4), dtype=bool) & ~np.eye(4, dtype=bool)
    mm = E * off
    Q = np.stack([E.sum(axis=(1, 3, 4)), mm.sum(axis=(1, 3, 4))], axis=-1)
    C = np.stack([E.sum(axis=(2, 3, 4)), mm.sum(axis=(2, 3, 4))], axis=-1)
    return Q, C, E.sum(axis=(1, 2))


def text_of(E, R, min_mapq=0, full=False):
    """the file's bytes, from the format's description"""
    Q, C, S = margins(E)
    mates = [m for m in (0, 1) if R[m, 0]]
    qn = lambda q: "none" if q == NONE else str(q)
    out = ["#salt-error-profile\tv1\tmin_mapq=%d\n" % min_mapq, "#R\tmate\tseen\tskipped\tunmapped\tlow_mapq\tcounted\treverse\tgapped\n"]
    out += ["R\t%d\t%s\n" % (m, "\t".join(str(int(x)) for x in R[m, :7])) for m in mates]
    out.append("#Q\tmate\tq\tbases\tmismatches\tempirical\n")
    for m in mates:
        for q in range(95):
            b, x = int(Q[m, q, 0]), int(Q[m, q, 1])
            if b:
                out.append("Q\t%d\t%s\t%d\t%d\t%.2f\n" % (m, qn(q), b, x, -10.0 * math.log10((x + 1.0) / (b + 2.0))))
    out.append("#C\tmate\tcycle\tbases\tmismatches\n")
    for m in mates:
        out += ["C\t%d\t%d\t%d\t%d\n" % (m, c + 1, int(C[m, c, 0]), int(C[m, c, 1])) for c in range(512) if C[m, c, 0]]
    out.append("#S\tmate\tref\tread\tcount\n")
    for m in mates:
        out += ["S\t%d\t%s\t%s\t%d\n" % (m, NT[a], NT[b], int(S[m, a, b])) for a in range(4) for b in range(4)]
    if full:
        out.append("#E\tmate\tcycle\tq\tref\tread\tcount\n")
        for m in mates:
            for c, q, a, b in zip(*np.nonzero(E[m])):
                out.append("E\t%d\t%d\t%s\t%s\t%s\t%d\n" % (m, c + 1, qn(q), NT[a], NT[b], int(E[m, c, q, a, b])))
    return "".join(out).encode()


def parse_file(data):
    """the file -> dict(min_mapq, R (2, 8), Q {(mate, q): (bases, mismatches, empirical text)}, C {(mate, cycle0): (bases, mismatches)},
    S (2, 4, 4), E (the full table, or None without the E section)); every line is checked for its shape"""
    assert data.endswith(b"\n")
    lines = data.decode().split("\n")[:-1]
    head = lines[0].split("\t")
    assert head[:2] == ["#salt-error-profile", "v1"] and head[2].startswith("min_mapq=") and len(head) == 3
    out = {"min_mapq": int(head[2][9:]), "R": np.zeros((2, 8), dtype=np.uint64), "Q": {}, "C": {}, "S": np.zeros((2, 4, 4), dtype=np.uint64), "E": None}
    heads = {"R": "#R\tmate\tseen\tskipped\tunmapped\tlow_mapq\tcounted\treverse\tgapped", "Q": "#Q\tmate\tq\tbases\tmismatches\tempirical",
             "C": "#C\tmate\tcycle\tbases\tmismatches", "S": "#S\tmate\tref\tread\tcount", "E": "#E\tmate\tcycle\tq\tref\tread\tcount"}
    seen, order, keys = [], "RQCSE", {}
    qv = lambda t: NONE if t == "none" else int(t)
    for line in lines[1:]:
        if line.startswith("#"):
            tag = line[1]
            assert heads[tag] == line and tag not in seen
            seen.append(tag)
            if tag == "E":
                out["E"] = np.zeros(SHAPE, dtype=np.uint64)
            continue
        f = line.split("\t")
        tag, m = f[0], int(f[1])
        assert tag == seen[-1] and m in (0, 1)
        if tag == "R":
            assert len(f) == 9
            out["R"][m, :7] = [int(x) for x in f[2:]]
            key = (m,)
        elif tag == "Q":
            assert len(f) == 6 and re.fullmatch(r"\d+\.\d\d", f[5])
            key = (m, qv(f[2]))
            out["Q"][key] = (int(f[3]), int(f[4]), f[5])
        elif tag == "C":
            assert len(f) == 5 and int(f[2]) >= 1
            key = (m, int(f[2]) - 1)
            out["C"][key] = (int(f[3]), int(f[4]))
        elif tag == "S":
            assert len(f) == 5
            key = (m, NT.index(f[2]), NT.index(f[3]))
            out["S"][key] = int(f[4])
        else:
            assert len(f) == 7 and int(f[6]) > 0
            key = (m, int(f[2]) - 1, qv(f[3]), NT.index(f[4]), NT.index(f[5]))
            out["E"][key] = int(f[6])
        assert tag not in keys or keys[tag] < key, "section %s is not ascending at %r" % (tag, key)
        keys[tag] = key
    assert "".join(seen) in (order, order[:4])
    return out


def requalify(sam, qual_of):
    """the SAM text with every record's QUAL replaced by qual_of(record index, L) (bytes of length L, in SAM order)"""
    out, k = [], 0
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if len(f) >= 11 and not line.startswith(b"@"):
            f[10] = qual_of(k, len(f[9]))
            k += 1
            line = b"\t".join(f)
        out.append(line)
    return b"\n".join(out)
