"""Coverage: the third statement of the rule, in Python, next to the device kernels (salt_depth.hip) and the host twins (salt_depth_add_sam,
salt_depth_text).  Written from the definition in include/salt_gpu.h: the SAM parsed, the CIGAR walked, the difference array summed, the
lines printed from integers.  The tests compare the other two with it."""
import os
import re

import numpy as np

from conftest import LAMBDA


def contigs_of_ann(ann_path):
    """[(name, offset, length)] of <P>.C.ann (bns_dump's text: a count line, then two lines per sequence)"""
    lines = open(ann_path).read().split("\n")
    n = int(lines[0].split()[1])
    return [(lines[1 + 2 * i].split()[1], int(lines[2 + 2 * i].split()[0]), int(lines[2 + 2 * i].split()[1])) for i in range(n)]


def lambda_contigs():
    return contigs_of_ann(os.path.join(LAMBDA, "idx.C.ann"))


def ref_len_of(contigs):
    return contigs[-1][1] + contigs[-1][2]


def diff_of_sam(contigs, sam, min_mapq=0):
    """(diff uint32[ref_len + 1], contributing records) of the record lines of a SAM text"""
    ref_len = ref_len_of(contigs)
    offsets = {name: off for name, off, _ in contigs}
    diff = np.zeros(ref_len + 1, dtype=np.int64)
    n_rec = 0
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        if int(f[1]) & 4 or int(f[4]) < min_mapq:
            continue
        n_rec += 1
        g = offsets[f[2].decode()] + int(f[3]) - 1
        for n, op in re.findall(rb"(\d+)([MIDS])", f[5]):
            n = int(n)
            if op == b"M":
                end = min(g + n, ref_len)
                if g < end:
                    diff[g] += 1
                    diff[end] -= 1
                g += n
            elif op == b"D":
                g += n
    return (diff % (1 << 32)).astype(np.uint32), n_rec


def max_m_end(contigs, sam):
    """the largest global position at which an M run of a mapped record ends (exclusive)"""
    offsets = {name: off for name, off, _ in contigs}
    top = 0
    for line in sam.split(b"\n"):
        f = line.split(b"\t")
        if len(f) < 11 or line.startswith(b"@") or int(f[1]) & 4:
            continue
        g = offsets[f[2].decode()] + int(f[3]) - 1
        for n, op in re.findall(rb"(\d+)([MIDS])", f[5]):
            if op in b"MD":
                g += int(n)
            if op == b"M":
                top = max(top, g)
    return top


def depth_of(diff):
    """depth[g], 0 <= g < ref_len, mod 2^32"""
    return (np.cumsum(diff[:-1].astype(np.uint64)) % (1 << 32)).astype(np.uint32)


def text_of(contigs, diff, window=0):
    """the per-base bedGraph (window 0) or the window means of a difference array, as bytes"""
    depth = depth_of(diff)
    out = []
    for name, off, length in contigs:
        d = depth[off:off + length]
        if window == 0:
            cuts = np.flatnonzero(d[1:] != d[:-1]) + 1
            starts = np.concatenate([[0], cuts])
            ends = np.concatenate([cuts, [length]])
            out += ["%s\t%d\t%d\t%d\n" % (name, a, b, d[a]) for a, b in zip(starts.tolist(), ends.tolist())]
        else:
            for a in range(0, length, window):
                b = min(a + window, length)
                s, n = int(d[a:b].astype(np.uint64).sum(dtype=np.uint64)), b - a
                h = (100 * s + n // 2) // n
                out.append("%s\t%d\t%d\t%d.%02d\n" % (name, a, b, h // 100, h % 100))
    return "".join(out).encode()


def parse_per_base(data):
    """[(contig, start, end, depth)] of a per-base text"""
    assert data.endswith(b"\n")
    rows = [l.split("\t") for l in data.decode().split("\n")[:-1]]
    assert all(len(r) == 4 for r in rows)
    return [(r[0], int(r[1]), int(r[2]), int(r[3])) for r in rows]
