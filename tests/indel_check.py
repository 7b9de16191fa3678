"""Indel candidates: the third statement of the definition in include/salt_gpu.h, in Python, next to the device kernels (salt_indel.hip)
and the host twin (salt_indel_add_sam, salt_indel_text).  The table of a SAM text as a dict, the four counters, the difference array, the
call, the file's bytes and a parser for them; Python integers and lists of letters, so nothing here can wrap or shift a bit field wrongly
the way the other two could.  The tests compare the other two with it."""
import re

import numpy as np

from gt_check import Genome  # noqa: F401  (2-bit bases and contigs of an index prefix)

DEFAULTS = dict(min_mapq=20, min_alt=3, min_pct=20, log2_slots=24)
MAX_INS, MAX_DEL, MAX_SHIFT, PROBE = 12, 63, 4096, 128
GOLD = 0x9E3779B97F4A7C15


def letter(genome, x):
    """the 2-bit genome's base at x, A beyond it"""
    return int(genome.bases[x]) if x < len(genome.masks) and x < len(genome.bases) else 0


def contig_of(genome, x):
    """(first position, end) of the last contig that begins at or in front of x; the last contig ends at ref_len"""
    c = genome.contig_of(x)
    ref_len = len(genome.masks)
    end = genome.contigs[c + 1][1] if c + 1 < len(genome.contigs) else ref_len
    return genome.contigs[c][1], min(end, ref_len)


def key_of(g, is_del, n, bases=()):
    k = 1 << 63 | g << 31 | (1 << 30 if is_del else 0) | n << 24
    for j, b in enumerate(bases):
        k |= b << (22 - 2 * j)
    return k


def key_parts(key):
    """(g, is_del, n, bases) of a well-formed key"""
    n = (key >> 24) & 63
    return (key >> 31) & 0xFFFFFFFF, bool((key >> 30) & 1), n, [] if (key >> 30) & 1 else [(key >> (22 - 2 * j)) & 3 for j in range(n)]


def well_formed(key, ref_len):
    g, is_del, n = (key >> 31) & 0xFFFFFFFF, (key >> 30) & 1, (key >> 24) & 63
    low = key & 0xFFFFFF
    if not key >> 63 or g < 1 or g > ref_len or n < 1:
        return False
    return low == 0 if is_del else n <= MAX_INS and low & ((1 << (24 - 2 * n)) - 1) == 0


def home(key, log2_slots):
    return ((key * GOLD) & (2 ** 64 - 1)) >> (64 - log2_slots)


def normalise(genome, g, is_del, n, bases):
    """(g, bases, steps) after the left shift"""
    first, _ = contig_of(genome, g - 1)
    bases, steps = list(bases), 0
    while steps < MAX_SHIFT and g - 1 > first:
        a = letter(genome, g - 1)
        if is_del:
            if a != letter(genome, g + n - 1):
                break
        else:
            if a != bases[-1]:
                break
            bases = [a] + bases[:-1]
        g, steps = g - 1, steps + 1
    return g, bases, steps


def add_sam(genome, sam, min_mapq=20, census=None):
    """(table {key: [fwd, rev]}, stats [tabled, dropped, long, unanchored], diff uint32[ref_len + 1], records that contributed) of the
    record lines of a SAM text.  census (a dict) gets: ops (the I and D ops of the counted records), moved (events the shift moved),
    moved_ins / moved_del, max_steps."""
    ref_len = len(genome.masks)
    table, stats, diff, n_rec = {}, [0, 0, 0, 0], np.zeros(ref_len + 1, dtype=np.int64), 0
    cs = dict(ops=0, moved=0, moved_ins=0, moved_del=0, max_steps=0)
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        flag = int(f[1])
        if flag & 4 or int(f[4]) < min_mapq:
            continue
        n_rec += 1
        g, s, seq = genome.offsets[f[2].decode()] + int(f[3]) - 1, 0, f[9]
        ops = []                                                       # the ops without the soft clips, with where they are met
        for n, op in re.findall(rb"(\d+)([MIDS])", f[5]):
            n = int(n)
            if op != b"S":
                ops.append((op, n, g, s))
            if op == b"M":
                end = min(g + n, ref_len)
                if g < end:
                    diff[g] += 1
                    diff[end] -= 1
                g, s = g + n, s + n
            elif op == b"D":
                g += n
            else:
                s += n
        for k, (op, n, g, s) in enumerate(ops):
            if op == b"M":
                continue
            cs["ops"] += 1
            is_del = op == b"D"
            if not 1 <= n <= (MAX_DEL if is_del else MAX_INS):
                stats[2] += 1
                continue
            ok = 0 < k < len(ops) - 1 and ops[k - 1][0] == b"M" and ops[k - 1][1] >= 1 and ops[k + 1][0] == b"M" and ops[k + 1][1] >= 1 and g >= 1
            bases = []
            if ok:
                _, end = contig_of(genome, g - 1)
                ok = g < end and (not is_del or g + n <= end)
            if ok and not is_del:
                bases = [b"ACGT".find(seq[s + j:s + j + 1]) for j in range(n)]
                ok = s + n <= len(seq) and min(bases) >= 0
            if not ok:
                stats[3] += 1
                continue
            g2, bases, steps = normalise(genome, g, is_del, n, bases)
            cs["moved"] += steps > 0
            cs["moved_del" if is_del else "moved_ins"] += steps > 0
            cs["max_steps"] = max(cs["max_steps"], steps)
            table.setdefault(key_of(g2, is_del, n, bases), [0, 0])[1 if flag & 16 else 0] += 1
            stats[0] += 1
    if census is not None:
        census.update(cs)
    return table, stats, (diff % (1 << 32)).astype(np.uint32), n_rec


def entries(table):
    """the table as the uint64 (n, 2) array of (key, value) pairs in key order that the other two hand out"""
    rows = [(k, (v[0] + (v[1] << 32)) & (2 ** 64 - 1)) for k, v in sorted(table.items())]
    return np.array([r for r in rows if r[1]], dtype=np.uint64).reshape(-1, 2)


def table_of(pairs):
    return {int(k): [int(v) & 0xFFFFFFFF, int(v) >> 32] for k, v in np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)}


def text(genome, pairs, diff, min_alt=3, min_pct=20):
    """the file's records (no header) of (key, value) pairs in key order"""
    ref_len = len(genome.masks)
    depth = np.cumsum(np.asarray(diff, dtype=np.uint64)[:-1]) % (1 << 32)
    out = []
    for key, v in np.asarray(pairs, dtype=np.uint64).reshape(-1, 2):
        key, v = int(key), int(v)
        if not well_formed(key, ref_len) or v == 0:
            continue
        g, is_del, n, bases = key_parts(key)
        fwd, rev, d = v & 0xFFFFFFFF, v >> 32, int(depth[g - 1])
        if fwd + rev < min_alt or 100 * (fwd + rev) < min_pct * d:
            continue
        name, off, _ = genome.contigs[genome.contig_of(g - 1)]
        anchor = "ACGT"[letter(genome, g - 1)]
        ref = anchor + ("".join("ACGT"[letter(genome, g + k)] for k in range(n)) if is_del else "")
        alt = anchor + ("" if is_del else "".join("ACGT"[b] for b in bases))
        out.append("%s\t%d\t.\t%s\t%s\t.\t.\tTYPE=%s;LEN=%d;DP=%d;AO=%d;AOF=%d;AOR=%d\n" % (name, g - off, ref, alt, "DEL" if is_del else "INS", n, d, fwd + rev, fwd, rev))
    return "".join(out).encode()


def header(genome, min_mapq=20, min_alt=3, min_pct=20, dropped=0):
    h = "##fileformat=VCFv4.2\n##source=salt --indels\n"
    h += "".join("##contig=<ID=%s,length=%d>\n" % (name, length) for name, _, length in genome.contigs)
    h += ('##INFO=<ID=TYPE,Number=1,Type=String,Description="INS or DEL">\n'
          '##INFO=<ID=LEN,Number=1,Type=Integer,Description="Inserted or deleted bases">\n'
          '##INFO=<ID=DP,Number=1,Type=Integer,Description="Counted reads whose M runs cover the anchor base">\n'
          '##INFO=<ID=AO,Number=1,Type=Integer,Description="Counted reads that show the allele, left-normalised">\n'
          '##INFO=<ID=AOF,Number=1,Type=Integer,Description="... on the forward strand">\n'
          '##INFO=<ID=AOR,Number=1,Type=Integer,Description="... on the reverse strand">\n')
    h += "##salt_indels_parameters=<min_mapq=%d,min_alt=%d,min_pct=%d>\n##salt_indels_dropped=%d\n" % (min_mapq, min_alt, min_pct, dropped)
    return (h + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n").encode()


def parse(data):
    """[(contig, pos1, ref, alt, {INFO})] of the records of a file (header lines skipped)"""
    assert data == b"" or data.endswith(b"\n")
    rows = [l.split("\t") for l in data.decode().split("\n")[:-1] if not l.startswith("#")]
    assert all(len(r) == 8 and r[2] == r[5] == r[6] == "." for r in rows)
    out = []
    for r in rows:
        info = dict(x.split("=") for x in r[7].split(";"))
        out.append((r[0], int(r[1]), r[3], r[4], {k: (v if k == "TYPE" else int(v)) for k, v in info.items()}))
    return out
