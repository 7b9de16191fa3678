"""SNP candidates off the index's sites: the third statement of the definition in include/salt_gpu.h, in Python, next to the device kernels
(salt_discover.hip) and the host twin (salt_disc_add_sam, salt_disc_text).  The arrays of a SAM text, the call, the file's bytes and a
parser for the file; Python integers for the fields, so nothing here can wrap.  The tests compare the other two with it."""
import re

import numpy as np

from gt_check import Genome  # noqa: F401  (masks, 2-bit bases and contigs of an index prefix)

DEFAULTS = dict(min_mapq=20, min_baseq=20, min_alt=3, min_pct=20)
BITS, FIELD = 21, (1 << 21) - 1


def add_sam(genome, sam, min_mapq=20, min_baseq=20, stats=None):
    """(alt uint64[ref_len], diff uint32[ref_len + 1], records that contributed) of the record lines of a SAM text.  stats (a dict) gets
    the census: events, events that counted, events at known sites, events with a usable quality below / at or above the floor."""
    ref_len = len(genome.masks)
    alt, diff, n_rec = [0] * ref_len, np.zeros(ref_len + 1, dtype=np.int64), 0
    st = dict(events=0, counted=0, at_sites=0, below=0, passed=0, unusable=0, cut=0)
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
                end = min(g + n, ref_len)
                st["cut"] += end < g + n
                if g < end:
                    diff[g] += 1
                    diff[end] -= 1
                for p in range(g, end):
                    b, m = b"ACGT".find(seq[s + p - g:s + p - g + 1]), int(genome.masks[p])
                    if b < 0 or m == 0 or (m >> b) & 1:
                        continue
                    st["events"] += 1
                    st["at_sites"] += (m & (m - 1)) != 0
                    byte = 0 if no_qual else qual[s + p - g]
                    usable = 33 <= byte <= 126
                    st["unusable"] += not usable
                    if usable and byte - 33 < min_baseq:
                        st["below"] += 1
                        continue
                    st["passed"] += usable
                    st["counted"] += 1
                    alt[p] += 1 << (BITS * bin(~m & 15 & ((1 << b) - 1)).count("1"))
                g, s = g + n, s + n
            elif op == b"D":
                g += n
            else:
                s += n
    if stats is not None:
        stats.update(st)
    return np.array([a & (2 ** 64 - 1) for a in alt], dtype=np.uint64), (diff % (1 << 32)).astype(np.uint32), n_rec


def counts(word, mask):
    """{base: count} of the bases outside the mask"""
    out = [b for b in range(4) if not (mask >> b) & 1]
    return {b: (int(word) >> (BITS * k)) & FIELD for k, b in enumerate(out)}


def called(word, mask, depth, min_alt=3, min_pct=20):
    return [b for b, n in counts(word, mask).items() if mask and n >= min_alt and 100 * n >= min_pct * depth]


def text(genome, alt, diff, min_alt=3, min_pct=20, all_sites=False):
    """the file's bytes"""
    depth = np.cumsum(np.asarray(diff, dtype=np.uint64)[:-1]) % (1 << 32)
    masks = genome.masks
    where = np.arange(len(alt)) if all_sites else np.flatnonzero(alt)
    out = []
    for g in where:
        m, d = int(masks[g]), int(depth[g])
        cs = called(alt[g], m, d, min_alt, min_pct)
        if m == 0 or not (cs or (all_sites and m & (m - 1))):
            continue
        name, off, _ = genome.contigs[genome.contig_of(int(g))]
        n = counts(alt[g], m)
        out.append("%s\t%d\t%s\t%s\t%d\t%s\n" % (name, g - off + 1, "/".join("ACGT"[b] for b in range(4) if (m >> b) & 1 or b in cs), "ACGT"[int(genome.bases[g])], d,
                                                 ",".join(str(n[b]) if b in n else "." for b in range(4))))
    return "".join(out).encode()


def parse(data):
    """[(contig, pos1, alleles, ref, depth, [cA, cC, cG, cT] with None for '.')]"""
    rows = [l.split("\t") for l in data.decode().split("\n")[:-1]]
    assert data == b"" or data.endswith(b"\n")
    assert all(len(r) == 6 for r in rows)
    return [(r[0], int(r[1]), r[2], r[3], int(r[4]), [None if x == "." else int(x) for x in r[5].split(",")]) for r in rows]
