"""The run's summary (`salt --stats`): the third statement of the rule, in Python, next to the device kernel (salt_stats.hip) and the host
twin (salt_stats_add_sam, salt_stats_text).  Written from the definition of the tables and of the file, not from the C: the SAM parsed,
the CIGAR walked, the file printed and read back.  The tests compare the other two with it."""
import os
import re

import numpy as np

from conftest import LAMBDA

# name -> (offset in the fixed cells, shape); CT stands apart, (contigs, 8)
TABLES = {"SN": (0, (2, 16)), "MQ": (32, (2, 256)), "RL": (544, (2, 513)), "GC": (1570, (2, 102)), "XA": (1774, (2, 8)), "IS": (1790, (4097,)),
          "OR": (5887, (4,)), "ID": (5891, (2, 65))}
CELLS = 6021
SN_KEYS = ["seen", "skipped", "unmapped", "low_mapq", "counted", "reverse", "gapped", "with_xa", "proper", "mate_unmapped", "mate_other_contig",
           "bases", "m_bases", "i_bases", "d_bases", "s_bases"]
HEAD = "#salt-stats\tv1\tmin_mapq=%d\tISQ mean: hundredths, the >=4096 bin left out\n"


def split(cells):
    """the fixed cells as a dict of views"""
    assert cells.shape == (CELLS,)
    return {k: cells[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in TABLES.items()}


def contigs_of_ann(ann_path):
    """[(name, offset, length)] of <P>.C.ann (a count line, then two lines per sequence: "gi name comment" and "offset len n_ambs")"""
    lines = open(ann_path).read().split("\n")
    n = int(lines[0].split()[1])
    return [(lines[1 + 2 * i].split()[1], int(lines[2 + 2 * i].split()[0]), int(lines[2 + 2 * i].split()[1])) for i in range(n)]


def lambda_contigs():
    return contigs_of_ann(os.path.join(LAMBDA, "idx.C.ann"))


def gc_bin(seq):
    gc, n = sum(seq.count(c) for c in b"CG"), sum(seq.count(c) for c in b"ACGT")
    return (200 * gc + n) // (2 * n) if n else 101


def tables_of_sam(contigs, sam, min_mapq=0, tables=None):
    """(cells, ct, records that counted) of the record lines of a SAM text; ref_len is the end of the last contig"""
    cells, ct = tables if tables is not None else (np.zeros(CELLS, dtype=np.uint64), np.zeros((len(contigs), 8), dtype=np.uint64))
    T = split(cells)
    rid_of = {name: i for i, (name, _, _) in enumerate(contigs)}
    ref_len = contigs[-1][1] + contigs[-1][2]
    n_rec = 0
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        flag, pos, mapq, cigar, rnext, pnext, tlen, seq = int(f[1]), int(f[3]), int(f[4]), f[5], f[6], int(f[7]), int(f[8]), f[9]
        mate = 1 if flag & 0x80 else 0
        SN = T["SN"][mate]
        SN[0] += 1
        T["RL"][mate, len(seq)] += 1
        T["GC"][mate, gc_bin(seq)] += 1
        SN[11] += len(seq)
        if flag & 4:
            SN[2] += 1
            continue
        rid = rid_of[f[2].decode()]
        T["MQ"][mate, mapq] += 1
        ct[rid, mate] += 1
        if mapq < min_mapq:
            SN[3] += 1
            continue
        n_rec += 1
        rev = bool(flag & 0x10)
        SN[4] += 1
        ct[rid, 2 + mate] += 1
        if rev:
            SN[5] += 1
            ct[rid, 4] += 1
        if re.search(rb"[IDS]", cigar):
            SN[6] += 1
        g = contigs[rid][1] + pos - 1
        for n, op in re.findall(rb"(\d+)([MIDS])", cigar):
            n = int(n)
            if op == b"M":
                cols = max(0, min(g + n, ref_len) - g)
                SN[12] += cols
                ct[rid, 5] += cols
                g += n
            elif op == b"I":
                SN[13] += n
                T["ID"][0, min(n, 64)] += 1
            elif op == b"D":
                SN[14] += n
                T["ID"][1, min(n, 64)] += 1
                g += n
            else:
                SN[15] += n
        xa = [t for t in f[11:] if t.startswith(b"XA:Z:")]
        n_xa = xa[0].count(b";") if xa else 0
        SN[7] += n_xa > 0
        T["XA"][mate, min(n_xa, 7)] += 1
        SN[8] += bool(flag & 2)
        if not flag & 1:
            continue
        if flag & 8:
            SN[9] += 1
            continue
        if rnext != b"=" and rnext != f[2]:
            SN[10] += 1
            continue
        if mate == 0:
            if tlen:
                T["IS"][min(abs(tlen), 4096)] += 1
            rev_ot = bool(flag & 0x20)
            if rev == rev_ot:
                T["OR"][2] += 1
            else:
                fwd, back = (pnext, pos) if rev else (pos, pnext)
                T["OR"][0 if fwd <= back else 1] += 1
    return cells, ct, n_rec


def isq(IS):
    """(pairs, [q25, q50, q75] as bin indices or None, mean in hundredths or None) of the insert-size histogram"""
    IS = [int(x) for x in IS]
    pairs = sum(IS)
    qs = []
    for k in (1, 2, 3):
        cum, at = 0, None
        for t, v in enumerate(IS):
            cum += v
            if pairs and 4 * cum >= k * pairs:
                at = t
                break
        qs.append(at)
    n, s = sum(IS[:4096]), sum(t * v for t, v in enumerate(IS[:4096]))
    return pairs, qs, (100 * s + n // 2) // n if n else None


def text_of(contigs, cells, ct, min_mapq=0):
    """the file's bytes, from the format's description"""
    T = split(np.asarray(cells))
    mates = [0, 1] if T["SN"][1, 0] else [0]
    out = [HEAD % min_mapq]
    out += ["SN\t%d\t%s\t%d\n" % (m, SN_KEYS[k], int(T["SN"][m, k])) for m in mates for k in range(16)]
    for tag in ("MQ", "RL", "GC", "XA"):
        for m in mates:
            for k, v in enumerate(T[tag][m]):
                if v:
                    out.append("%s\t%d\t%s\t%d\n" % (tag, m, "none" if (tag, k) == ("GC", 101) else str(k), int(v)))
    tl = lambda t: ">=4096" if t == 4096 else str(t)
    out += ["IS\t%s\t%d\n" % (tl(t), int(v)) for t, v in enumerate(T["IS"]) if v]
    pairs, qs, mean = isq(T["IS"])
    out.append("ISQ\t%d\t%s\t%s\n" % (pairs, "\t".join("." if q is None else tl(q) for q in qs), "." if mean is None else "%d.%02d" % (mean // 100, mean % 100)))
    out.append("OR\t%d\t%d\t%d\n" % tuple(int(x) for x in T["OR"][:3]))
    out += ["ID\t%s\t%d\t%d\n" % (">=64" if k == 64 else str(k), int(T["ID"][0, k]), int(T["ID"][1, k])) for k in range(65) if T["ID"][0, k] or T["ID"][1, k]]
    out += ["CT\t%s\t%d\t%s\n" % (name, length, "\t".join(str(int(x)) for x in ct[i][:6])) for i, (name, _, length) in enumerate(contigs)]
    return "".join(out).encode()


def parse_file(data):
    """the file -> dict(min_mapq, cells, ct, names, lengths, isq (the ISQ line's fields as text)); every line is checked for its shape, the
    order of the sections and of the keys inside each"""
    assert data.endswith(b"\n")
    lines = data.decode().split("\n")[:-1]
    head = lines[0].split("\t")
    assert head[:2] == ["#salt-stats", "v1"] and head[2].startswith("min_mapq=") and len(head) == 4 and ">=4096" in head[3]
    cells = np.zeros(CELLS, dtype=np.uint64)
    T = split(cells)
    out = {"min_mapq": int(head[2][9:]), "cells": cells, "names": [], "lengths": [], "isq": None}
    ct, order, last = [], ["SN", "MQ", "RL", "GC", "XA", "IS", "ISQ", "OR", "ID", "CT"], {}
    seen = []
    for line in lines[1:]:
        f = line.split("\t")
        tag = f[0]
        assert tag in order and (not seen or order.index(seen[-1]) <= order.index(tag)), line
        if not seen or seen[-1] != tag:
            seen.append(tag)
        if tag == "SN":
            assert len(f) == 4 and f[2] in SN_KEYS
            key = (int(f[1]), SN_KEYS.index(f[2]))
            T["SN"][key] = int(f[3])
        elif tag in ("MQ", "RL", "GC", "XA"):
            assert len(f) == 4 and int(f[3]) > 0
            key = (int(f[1]), 101 if f[2] == "none" else int(f[2]))
            assert tag == "GC" or f[2] != "none"
            T[tag][key] = int(f[3])
        elif tag == "IS":
            assert len(f) == 3 and int(f[2]) > 0
            key = (4096 if f[1] == ">=4096" else int(f[1]),)
            assert key[0] < 4096 or f[1] == ">=4096"
            T["IS"][key] = int(f[2])
        elif tag == "ISQ":
            assert len(f) == 6 and out["isq"] is None
            out["isq"], key = f[1:], ()
        elif tag == "OR":
            assert len(f) == 4
            T["OR"][:3], key = [int(x) for x in f[1:]], ()
        elif tag == "ID":
            assert len(f) == 4 and (int(f[2]) or int(f[3]))
            key = (64 if f[1] == ">=64" else int(f[1]),)
            assert key[0] < 64 or f[1] == ">=64"
            T["ID"][0, key[0]], T["ID"][1, key[0]] = int(f[2]), int(f[3])
        else:
            assert len(f) == 9
            out["names"].append(f[1]); out["lengths"].append(int(f[2]))
            ct.append([int(x) for x in f[3:]] + [0, 0])
            key = (len(ct),)
        assert tag not in last or last[tag] < key, "section %s is not ascending at %r" % (tag, key)
        last[tag] = key
    assert [t for t in seen if t in ("SN", "ISQ", "OR", "CT")] == ["SN", "ISQ", "OR", "CT"]
    out["ct"] = np.array(ct, dtype=np.uint64).reshape(len(ct), 8)
    return out
