"""Allele counts at the SNP sites: the third statement of the rule, in Python, next to the device kernel (salt_snp.hip) and the host twin
(salt_snp_count_sam).  Written from the definition in include/salt_gpu.h: the .ref file decoded, the SAM parsed, the CIGAR walked.  The
tests compare the other two with it, and use census() to show that a golden exercises what it is said to."""
import gzip
import os
import re

import numpy as np

from conftest import LAMBDA

# golden -> (contributing records at min_mapq 0, at 20), as counted when the fixtures were made
GOLDENS = {
    "expect_se_default.sam": (1907, 882), "expect_pe_default.sam": (1929, 779), "expect_ragged_pe.sam": (573, 255),
    "expect_gap_se_mid.sam.gz": (1216, 1046), "expect_gap_pe_short.sam.gz": (902, 527), "expect_span_default.sam": (40, 19),
}


def golden_sam(name):
    data = open(os.path.join(LAMBDA, name), "rb").read()
    return gzip.decompress(data) if name.endswith(".gz") else data


def sites_of_ref(ref_path):
    """ascending genome positions whose 4-bit mask has two or more bits set; <P>.ref = ref_len, then 8 masks per 32-bit word, low nibble first"""
    words = np.fromfile(ref_path, dtype="<u4")
    ref_len = int(words[0])
    masks = ((words[1:, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).reshape(-1)[:ref_len]
    return np.flatnonzero((masks & (masks - 1)) != 0).astype(np.uint32), masks


def contig_offsets(ann_path):
    """{name: offset in the concatenated genome} of <P>.C.ann (bns_dump's text: a count line, then two lines per sequence)"""
    lines = open(ann_path).read().split("\n")
    n = int(lines[0].split()[1])
    return {lines[1 + 2 * i].split()[1]: int(lines[2 + 2 * i].split()[0]) for i in range(n)}


def count_sam(sites, offsets, sam, min_mapq=0):
    """counts[(site, base)] of the record lines of a SAM text, and the records that contributed"""
    site_of = {int(g): i for i, g in enumerate(sites)}
    counts = np.zeros((len(sites), 4), dtype=np.uint32)
    n_rec = 0
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        if int(f[1]) & 4 or int(f[4]) < min_mapq:
            continue
        n_rec += 1
        g, s, seq = offsets[f[2].decode()] + int(f[3]) - 1, 0, f[9]
        for n, op in re.findall(rb"(\d+)([MIDS])", f[5]):
            n = int(n)
            if op == b"M":
                for k in range(n):
                    b = b"ACGT".find(seq[s + k:s + k + 1])
                    if g + k in site_of and b >= 0:
                        counts[site_of[g + k], b] += 1
                g, s = g + n, s + n
            elif op == b"D":
                g += n
            else:
                s += n
    return counts, n_rec


def census(sam, min_mapq=0):
    """(indel ops, soft-clip ops) among the CIGARs of the records that contribute"""
    indel = clip = 0
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if len(f) < 11 or line.startswith(b"@") or int(f[1]) & 4 or int(f[4]) < min_mapq:
            continue
        indel += len(re.findall(rb"\d+[ID]", f[5]))
        clip += len(re.findall(rb"\d+S", f[5]))
    return indel, clip


def parse_counts_file(data):
    """--snp-counts FILE -> ([(contig, pos1, ref, alleles)], counts (n, 4) uint64)"""
    lines = data.decode().split("\n")
    assert lines[0] == "#contig\tpos\tref\talleles\tA\tC\tG\tT" and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert all(len(r) == 8 for r in rows)
    return [(r[0], int(r[1]), r[2], r[3]) for r in rows], np.array([[int(x) for x in r[4:]] for r in rows], dtype=np.uint64).reshape(-1, 4)
