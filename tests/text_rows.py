"""Built rows for the text kernels (salt_amd/csrc/salt_text.hip) and the bytes they must give.

GpuAligner.text_from_rows / text_from_rows_pe hand the FASTQ scan, k_pack's records and the SAM / BAM record kernels result rows of our
choosing.  This module builds those rows and their FASTQ blocks, states the 4-line FASTQ rules in plain Python (fq_parse), gets the expected
bytes from the host twins (Index.samse / Index.sampe per record, salt_amd.bam_from_sam of that text), and counts -- from the expected bytes,
the rows and the blocks alone, never from device output -- that every class of record the kernels treat differently is there (census).
No GPU here: tests/test_text_rows_model.py builds and counts everything on the CPU, tests/test_gpu_text_rows.py compares the device.

Two indexes: the committed dense one (3 000 bases, 434 SNPs) for MD / NM / XV, and one built here from memory with three contigs (names of
1, 40 and 74 characters; the first long enough for positions that straddle 2^14, 2^17 and 2^20) for RNAME, POS, XA, bins and the slot edges."""
import os
import time

import numpy as np

from conftest import GOLDEN

UNMAPPED = 0xFFFFFFFF
NT = b"ACGTN"
SPACE = b" \t\n\v\f\r"
CODE = np.full(256, 4, dtype=np.uint8)
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    CODE[_c] = _v
LETTER = np.frombuffer(NT, dtype=np.uint8)
SE_UNMAPPED_HEAD = b"\t4\t*\t0\t0\t*\t*\t0\t0\t"
HEAD_CAP, TAIL_CAP = 96, 224                   # the record slot of k_sam_len: SAM_HEAD_CAP, SAM_TAIL_CAP
BAM_HEAD_WORDS = (HEAD_CAP - 36) // 4          # CIGAR words that fit the head part beside BAM's 36 fixed bytes
XV_CAP = 64                                    # sam.c:246-328 lists at most 64 offsets
L_SEED = 19
MAX_READS = 8192                               # records of the largest block a test hands over: the GPU tests' workspaces hold as many
BIG_CONTIG = 1_100_000                         # the built index's first contig: passes 2^20
NAMES = ("q", "contig_two_of_the_built_index_40_chars__", "c" * 74)
LENS = (BIG_CONTIG, 60, 3000)


# ---- the 4-line FASTQ rules (query.c:146-239 with trim_readno, query.c:139-143) ----
def fq_parse(block):
    """[(name, codes, quality)] of a block of whole 4-line records: the name runs up to the first white space and loses a trailing /digit
    when it is longer than 2; carriage returns in front of the newline are no part of a sequence or quality; A0 C1 G2 T3, anything else 4."""
    lines = block.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    out = []
    for i in range(0, len(lines) - 1, 4):
        head, seq, plus, qual = lines[i:i + 4]
        assert head[:1] == b"@" and plus[:1] == b"+"
        k = 1
        while k < len(head) and head[k] not in SPACE:
            k += 1
        name = head[1:k]
        if len(name) > 2 and name[-2:-1] == b"/" and name[-1:].isdigit():
            name = name[:-2]
        seq, qual = seq.rstrip(b"\r"), qual.rstrip(b"\r")
        assert len(seq) == len(qual) > 0
        out.append((name, CODE[np.frombuffer(seq, dtype=np.uint8)], qual))
    return out


# ---- an index with its bases and masks as arrays ----
class Ref:
    def __init__(self, prefix):
        import salt_amd
        self.ix = salt_amd.Index.reload(prefix)
        w = np.fromfile(prefix + ".ref", dtype="<u4")
        self.ref_len = int(w[0])
        at = np.arange(self.ref_len)
        self.mask = ((w[1:][at >> 3] >> (4 * (at & 7))) & 15).astype(np.uint8)
        pac = np.fromfile(prefix + ".C.pac", dtype=np.uint8)
        self.base = ((pac[at >> 2] >> ((~at & 3) << 1)) & 3).astype(np.uint8)
        self.contigs = self.ix.contigs()                         # (offset, length, name)

    def alt(self, g, listed, salt=0):
        """a base that differs from the genome's at g: one the mask lists if `listed` and there is one, else one it does not list if there is"""
        b, m = int(self.base[g]), int(self.mask[g])
        yes = [c for c in range(4) if c != b and (m >> c) & 1]
        no = [c for c in range(4) if c != b and not (m >> c) & 1]
        pick = (yes or no) if listed else (no or yes)
        return pick[(g + salt) % len(pick)]


def dense_ref():
    return Ref(os.path.join(GOLDEN, "index_cases", "dense", "idx"))


def built_genome():
    rng = np.random.Generator(np.random.PCG64(4242))
    return [LETTER[rng.integers(0, 4, size=n)] for n in LENS]


def build_index(prefix):
    """the three-contig index, from memory, on the host; returns the build's seconds"""
    import salt_amd
    contigs = list(zip(NAMES, built_genome()))
    groups = []
    for (name, seq), at in zip(contigs, ((7, 16380, 16390, 131070, 131080, 1048570, 1048580, BIG_CONTIG - 1), (0, 30, 59), (0, 9, 99, 999, 2999))):
        pos = np.array(at, dtype=np.uint32)
        ref = CODE[seq[pos]]
        groups.append((name, pos, ((1 << ref) | (1 << ((ref + 1 + pos % 3) & 3))).astype(np.uint8), ref))
    t0 = time.perf_counter()
    salt_amd.idx_build_mem(contigs, groups, prefix, L_SEED)
    return time.perf_counter() - t0


# ---- rows ----
def new_rows(n):
    import salt_amd
    rows = np.zeros(n, dtype=salt_amd.RESULT_DTYPE)
    rows["pos"] = UNMAPPED
    rows["strand"] = 3
    rows["n_diff"] = rows["is_gap"] = 255
    return rows


def ops(*pairs):
    """("M", 20), ("I", 1), ... -> binary operations"""
    return [(n << 4) | "MID".index(o) for o, n in pairs]


def cigar_spans(cig):
    on_ref = sum(c >> 4 for c in cig if c & 15 in (0, 2))
    on_read = sum(c >> 4 for c in cig if c & 15 in (0, 1))
    return on_ref, on_read


def set_mapped(rows, i, pos, strand, cig, seq_start=0, mapq=37, n_diff=0):
    r = rows[i]
    r["pos"], r["strand"], r["mapq"], r["n_diff"] = pos, strand, mapq, n_diff
    r["is_gap"] = 0 if len(cig) == 1 else 1
    r["seq_start"], r["seq_end"] = seq_start, seq_start + cigar_spans(cig)[1] - 1
    r["n_cigar"] = len(cig)
    r["cigar"][:len(cig)] = cig


def set_hits(rows, i, hits):
    """hits: [(strand, pos, n_diff, cigar or None)] in strand order"""
    r = rows[i]
    k = [0, 0]
    for h, (s, pos, nd, cig) in enumerate(hits):
        assert h == 0 or s >= hits[h - 1][0]
        x = r["hits"][s][k[s]]
        x["pos"], x["n_diff"], x["is_gap"], x["strand"] = pos, nd, 0 if cig is None else 1, s
        if cig is not None:
            r["hit_n_cigar"][h] = len(cig)
            r["hit_cigar"][h][:len(cig)] = cig
        k[s] += 1
    r["n_hits"][0], r["n_hits"][1] = k


# ---- reads ----
def revcomp(codes):
    c = np.asarray(codes, dtype=np.uint8)[::-1]
    return np.where(c < 4, 3 - c, c).astype(np.uint8)


def filler(n, salt):
    return ((np.arange(n) * 7 + salt * 3 + (np.arange(n) >> 2)) & 3).astype(np.uint8)


def aligned_read(ref, pos, cig, flips=(), listed=True, clip5=0, clip3=0, salt=0):
    """the bases of a read as aligned: clip5 bases, the CIGAR walked over the genome from pos (M copies, I inserts, D skips), clip3 bases;
    flips: read offsets (from the first aligned base, I counted) inside M operations that get another base than the genome's"""
    out, g, s, flips = [filler(clip5, salt)], pos, 0, set(flips)
    for c in cig:
        n, op = c >> 4, c & 15
        if op == 0:
            run = ref.base[g:g + n].copy()
            for k in range(n):
                if s + k in flips:
                    run[k] = ref.alt(g + k, listed, salt)
            out.append(run)
            g += n
            s += n
        elif op == 1:
            out.append(filler(n, salt + 1))
            s += n
        else:
            g += n
    out.append(filler(clip3, salt + 2))
    return np.concatenate(out).astype(np.uint8)


def quality(n, salt):
    return (((np.arange(n) * 13 + salt * 7) % 94) + 33).astype(np.uint8).tobytes()


class Block:
    """One device call: the FASTQ block(s), the rows, the options."""

    def __init__(self, name, ref, paired=False, c=1, d=1, rg=None, direct=False, eol=b"\n", min_tlen=250, max_tlen=550):
        self.name, self.ref, self.paired, self.c, self.d, self.rg, self.direct, self.eol = name, ref, paired, c, d, rg, direct, eol
        self.min_tlen, self.max_tlen = min_tlen, max_tlen
        self.recs, self.fill = [], []                             # (header behind '@', sequence letters, third line, quality); row setters
        self.fq1 = self.fq2 = self.rows = None

    def opt(self, ref):
        import salt_amd
        return salt_amd.AlnOpt(l_seed=ref.ix.l_seed, print_xa_cigar=self.c, print_nm_md=self.d, rg_id=self.rg, paired=int(self.paired),
                               min_tlen=self.min_tlen, max_tlen=self.max_tlen)

    def add(self, header, letters, qual=None, plus=b"+", setter=None):
        i = len(self.recs)
        self.recs.append((header, bytes(letters), plus, quality(len(letters), i) if qual is None else qual))
        self.fill.append(setter)
        return i

    def add_read(self, codes, strand=0, setter=None, header=None):
        """a read given as aligned: the FASTQ holds the reverse complement for strand 1"""
        i = len(self.recs)
        codes = np.asarray(codes, dtype=np.uint8)
        return self.add(b"r%d" % i if header is None else header, LETTER[revcomp(codes) if strand == 1 else codes].tobytes(), setter=setter)

    def text(self, recs):
        e = self.eol
        return b"".join(b"@" + h + e + s + e + p + e + q + e for h, s, p, q in recs)

    def finish(self):
        self.rows = new_rows(len(self.recs))
        for i, f in enumerate(self.fill):
            if f is not None:
                f(self.rows, i)
        if self.paired:
            assert len(self.recs) % 2 == 0
            self.fq1, self.fq2 = self.text(self.recs[0::2]), self.text(self.recs[1::2])
        else:
            self.fq1, self.fq2 = self.text(self.recs), b""
        return self

    def reads(self):
        """[(name, codes, quality)] in row order, by the Python parse"""
        if not self.paired:
            return fq_parse(self.fq1)
        a, b = fq_parse(self.fq1), fq_parse(self.fq2)
        return [x for pair in zip(a, b) for x in pair]


def mapped(pos, strand, cig, **kw):
    return lambda rows, i: set_mapped(rows, i, pos, strand, cig, **kw)


def skipped(rows, i):
    rows[i]["skipped"] = 1


# ---- the case sets ----
EDGE_COLS = (0, 15, 16, 17, 31, 32)
PATTERNS = ("none", "all_listed", "all_unlisted", "edges_listed", "edges_unlisted")


def flips_of(pattern, n):
    if pattern == "none":
        return ()
    if pattern.startswith("all"):
        return range(n)
    return sorted({c for c in EDGE_COLS + (n - 1,) if 0 <= c < n})


def md_words_se(ref, strand):
    """one M over the whole read: pos & 15 x n = 1 .. 48 x the mismatch patterns; then runs that end on the genome's last base"""
    b = Block("md_words_se_%d" % strand, "dense")
    k = 0
    for p in range(16):
        for n in range(1, 49):
            for pat in PATTERNS:
                k += 1
                pos = p + 16 * ((k * 37) % ((ref.ref_len - n - p) // 16 + 1))
                cig = ops(("M", n))
                b.add_read(aligned_read(ref, pos, cig, flips_of(pat, n), "unlisted" not in pat, salt=k), strand, mapped(pos, strand, cig))
    for n in range(1, 49):
        for pat in ("none", "edges_listed", "all_unlisted"):
            pos, cig = ref.ref_len - n, ops(("M", n))
            b.add_read(aligned_read(ref, pos, cig, flips_of(pat, n), "unlisted" not in pat, salt=n), strand, mapped(pos, strand, cig))
    return b.finish()


def md_words_pe(ref, part):
    """paired end, both soft clips printed: seq_start 0 .. 15 x pos & 15 x n = 1 .. 48, a third of it per block.  A reduction against the
    single-end blocks, which carry every mismatch pattern for every (pos & 15, n): here the five patterns and the two strands cycle over
    the product (k % 5, k // 5 & 1), so not every pattern meets every seq_start; the census asserts (pos & 15, n mod 16) and
    seq_start & 15, not pattern x seq_start"""
    b = Block("md_words_pe_%d" % part, "dense", paired=True)
    k = 0
    for s0 in range(16):
        for p in range(16):
            for n in range(1 + part, 49, 3):
                k += 1
                pat, strand, clip3 = PATTERNS[k % 5], (k // 5) & 1, 1 + k % 3
                room = ref.ref_len - n - p
                pos = p + 16 * ((k * 41) % (room // 16 + 1)) if k % 7 else ref.ref_len - n       # every seventh ends on the last base
                cig = ops(("M", n))
                b.add_read(aligned_read(ref, pos, cig, flips_of(pat, n), "unlisted" not in pat, s0, clip3, salt=k), strand,
                           mapped(pos, strand, cig, seq_start=s0))
    return b.finish()


def densest_window(ref, n=512):
    site = ((ref.mask & (ref.mask - 1)) != 0).astype(np.int64)
    c = np.concatenate([[0], np.cumsum(site)])
    w = int(np.argmax(c[n:] - c[:-n]))
    return w, [int(g) for g in np.nonzero(site[w:w + n])[0] + w]


def xv_cap(ref, paired):
    """512 bases over the densest stretch, listed alleles at 63, 64, 65 and all of its sites; both strands; the same with one N (the walk)"""
    b = Block("xv_cap_" + ("pe" if paired else "se"), "dense", paired=paired)
    w, sites = densest_window(ref)
    assert len(sites) > XV_CAP + 1
    cig = ops(("M", 512))
    for with_n in (False, True):
        for strand in (0, 1):
            for k in (XV_CAP - 1, XV_CAP, XV_CAP + 1, len(sites)):
                codes = aligned_read(ref, w, cig, [g - w for g in sites[:k]], True, salt=k)
                if with_n:
                    codes[min(set(range(512)) - {g - w for g in sites})] = 4
                b.add_read(codes, strand, mapped(w, strand, cig))
    return b.finish()


def gapped_cigars():
    a = 6
    out = {"I1": ops(("M", 20), ("I", 1), ("M", 20)), "I30": ops(("M", 20), ("I", 30), ("M", 20)),
           "D1": ops(("M", 20), ("D", 1), ("M", 20)), "D30": ops(("M", 20), ("D", 30), ("M", 20)),
           "D_behind_mismatch": ops(("M", 20), ("D", 3), ("M", 20)), "I_first": ops(("I", 5), ("M", 30)), "I_last": ops(("M", 30), ("I", 5))}
    for n_ops in (2, 15, 16, 17, 64):
        out["ops%d" % n_ops] = ops(*[("M", a) if j % 2 == 0 else ("ID"[(j // 2) % 2], 1 + j % 3) for j in range(n_ops)])
    return out


def walk_block(ref, paired):
    """the per-base walk: one M with an N in the read (first base, last base, inside a mismatch window), and gapped CIGARs"""
    b = Block("walk_" + ("pe" if paired else "se"), "dense", paired=paired)
    k = 0
    for p in range(16):
        for n in range(1, 49):
            k += 1
            strand, clip5, clip3 = k & 1, (k % 16 if paired else 0), (1 + k % 3 if paired else 0)
            pos = p + 16 * ((k * 29) % ((ref.ref_len - n - p) // 16 + 1))
            cig = ops(("M", n))
            codes = aligned_read(ref, pos, cig, flips_of("edges_listed", n), True, clip5, clip3, salt=k)
            codes[clip5 + (0, n - 1, min(n - 1, 16))[k % 3]] = 4
            b.add_read(codes, strand, mapped(pos, strand, cig, seq_start=clip5))
    for name, cig in sorted(gapped_cigars().items()):
        for strand in (0, 1):
            for pos in (100, 1111, ref.ref_len - cigar_spans(cig)[0]):
                k += 1
                clip5, clip3 = ((3, 4) if paired else (0, 0))
                flips = {"D_behind_mismatch": (19,), "I_first": (5,), "I_last": (29,)}.get(name, (0, cigar_spans(cig)[1] - 1))
                b.add_read(aligned_read(ref, pos, cig, flips, k & 1 == 0, clip5, clip3, salt=k), strand, mapped(pos, strand, cig, seq_start=clip5))
    if paired and len(b.recs) % 2:
        b.add_read(aligned_read(ref, 5, ops(("M", 9))), 0, mapped(5, 0, ops(("M", 9))))
    return b.finish()


def long_tails(ref, paired):
    """512 bases with every second base another one (NM 256: type S in BAM; 255: type C), a tail far beyond the slot"""
    b = Block("long_tails_" + ("pe" if paired else "se"), "dense", paired=paired)
    cig = ops(("M", 512))
    for strand in (0, 1):
        for n_mis in (256, 255):
            for listed in (True, False):
                b.add_read(aligned_read(ref, 1000 + strand, cig, range(0, 2 * n_mis, 2), listed, salt=n_mis), strand, mapped(1000 + strand, strand, cig))
    return b.finish()


def kinds_se(ref):
    """skipped, unmapped and mapped reads in turn, at every length where the eight lanes of a record split their copies differently"""
    b = Block("kinds_se", "dense")
    k = 0
    for rep in range(3):
        for L in (1, 2, 7, 8, 9, 15, 16, 17, 33, 255, 256, 257, 512):
            for kind in range(3):
                k += 1
                strand, pos, cig = (k // 3) & 1, (k * 53) % (ref.ref_len - L), ops(("M", L))
                codes = aligned_read(ref, pos, cig, (L // 2,), True, salt=k)
                if kind == 0:
                    codes[:] = 4
                b.add_read(codes, strand if kind == 2 else 0, (skipped, None, mapped(pos, strand, cig))[kind])
    return b.finish()


def xa_block(ref, c, paired):
    """every split of 0 .. 5 hits over the strands, on every contig, one hit at the row's own pos, gapped hits of 1 and 64 operations"""
    b = Block("xa_%s_c%d" % ("pe" if paired else "se", c), "built", paired=paired, c=c)
    starts = [o for o, _, _ in ref.contigs]
    L, k = 40, 0
    long_cig = ops(*[("M", 1) if j % 2 == 0 else ("ID"[(j // 2) % 2], 1) for j in range(64)])
    for n0 in range(6):
        for n1 in range(6 - n0):
            for variant in range(3):
                k += 1
                strand, pos = k & 1, starts[k % 3] + (k % 15)
                hits = []
                for h in range(n0 + n1):
                    ci = (k + h) % 3
                    hp = starts[ci] + (h * 11 + k + 17) % (ref.contigs[ci][1] - 1)
                    cig = None if (h + variant) % 3 == 0 else (ops(("M", L)) if (h + variant) % 3 == 1 else long_cig)
                    if variant == 1 and h == (k % (n0 + n1)):
                        hp = pos                                     # left out of XA; the hit index still advances
                    hits.append((0 if h < n0 else 1, hp, h + variant, cig))
                cig = ops(("M", L))

                def setter(rows, i, pos=pos, strand=strand, cig=cig, hits=hits):
                    set_mapped(rows, i, pos, strand, cig)
                    set_hits(rows, i, hits)
                b.add_read(aligned_read(ref, pos, cig, (3,), True, salt=k), strand, setter)
    if paired:                                                       # an unmapped mate keeps its XA (alnpe_sam prints it for every record)
        hits = [(0, starts[1] + 3, 1, None), (1, starts[2] + 5, 2, long_cig)]
        b.add_read(filler(L, 1), 0, lambda rows, i: set_hits(rows, i, hits))
        b.add_read(aligned_read(ref, starts[2], ops(("M", L))), 1, mapped(starts[2], 1, ops(("M", L))))
        if len(b.recs) % 2:
            b.add_read(aligned_read(ref, starts[0] + 77, ops(("M", L))), 0, mapped(starts[0] + 77, 0, ops(("M", L))))
    return b.finish()


def slot_edges(ref, paired, rg_len):
    """exact reads of 50 bases (tail: MD:Z:50 NM:i:0 and the read group, 21 + rg_len bytes) on the 74-character contig at positions of 1 to 4
    digits and MAPQ of 1 to 3 digits: heads on both sides of the 96 bytes, tails on both sides of the 224"""
    b = Block("slot_%s_rg%d" % ("pe" if paired else "se", rg_len), "built", paired=paired, rg="g" * rg_len, min_tlen=1, max_tlen=100000)
    off3 = ref.contigs[2][0]
    cig = ops(("M", 50))
    for strand in (0, 1):
        for at in (0, 4, 8, 9, 10, 98, 99, 100, 998, 999, 1000, 2950):
            for mapq in (5, 37, 255):
                for mate_at in ((4, 99, 1500) if paired else (None,)):
                    pos = off3 + at
                    b.add_read(aligned_read(ref, pos, cig), strand, mapped(pos, strand, cig, mapq=mapq))
                    if paired:
                        pos2 = off3 + mate_at
                        b.add_read(aligned_read(ref, pos2, cig), 1 - strand, mapped(pos2, 1 - strand, cig, mapq=mapq))
    return b.finish()


def contig_search(ref, name):
    """rows on the first and last possible position of every contig, and one base on the genome's last"""
    b = Block("contig_search_" + name, name, c=1)
    L = 25
    for ci, (off, ln, _) in enumerate(ref.contigs):
        for pos in (off, off + ln - L, off + ln - 1, off + 1):
            for strand in (0, 1):
                n = min(L, off + ln - pos)
                cig = ops(("M", n))
                hits = [(0, off, 0, None), (1, off + ln - 1, 1, None)] + ([(1, off - 1, 2, None)] if off else [])

                def setter(rows, i, pos=pos, strand=strand, cig=cig, hits=hits):
                    set_mapped(rows, i, pos, strand, cig)
                    set_hits(rows, i, hits)
                b.add_read(aligned_read(ref, pos, cig), strand, setter)
    last = ref.ref_len - 1
    b.add_read(aligned_read(ref, last, ops(("M", 1))), 0, mapped(last, 0, ops(("M", 1))))
    return b.finish()


def bins_block(ref, paired):
    """the first contig's 2^14, 2^17 and 2^20 boundaries: reads that end on them, begin on them and straddle them"""
    b = Block("bins_" + ("pe" if paired else "se"), "built", paired=paired, min_tlen=1, max_tlen=1 << 21)
    k = 0
    for edge in (1 << 14, 2 << 14, 1 << 17, 1 << 20):
        for L in (50, 51):
            for pos in (edge - L - 1, edge - L, edge - L + 1, edge - 1, edge):
                k += 1
                if k % 4 == 0:                                       # a D moves the end, not the read
                    cig = ops(("M", L - 20), ("D", 7), ("M", 20))
                    pos -= 7 if pos < edge - 1 else 0
                else:
                    cig = ops(("M", L))
                b.add_read(aligned_read(ref, pos, cig), k & 1, mapped(pos, k & 1, cig))
    return b.finish()


PE_KINDS = ("U", "F", "R")


def pe_matrix(ref):
    """alnpe_sam's head: {unmapped, forward, reverse} x the same for the mate; same and different contigs; equal positions; TLEN just inside
    and outside both window ends (250, 550); seq_start / seq_end of 0, 1 and L - 2; mates of different, also odd, lengths"""
    b = Block("pe_matrix", "built", paired=True)
    off = [o for o, _, _ in ref.contigs]
    k = 0

    def mate(kind, pos, L, s0, s1):
        """kind U / F / R; the aligned part is read bases [s0, s1]"""
        nonlocal k
        k += 1
        if kind == "U":
            return b.add_read(filler(L, k), 0, None)
        strand, cig = PE_KINDS.index(kind) - 1, ops(("M", s1 - s0 + 1))
        return b.add_read(aligned_read(ref, pos, cig, (0,), True, s0, L - 1 - s1, salt=k), strand, mapped(pos, strand, cig, seq_start=s0, mapq=20 + k % 30))

    spans = lambda L: ((0, L - 1), (1, L - 1), (0, L - 2), (1, L - 2), (L - 2, L - 2), (L - 2, L - 1), (0, 0), (0, 1))
    for k0 in PE_KINDS:
        for k1 in PE_KINDS:
            for c0, c1 in ((0, 0), (0, 2), (2, 0), (1, 1)):
                for j, ((a0, a1), (b0, b1)) in enumerate(zip(spans(31), spans(44)[3:] + spans(44)[:3])):
                    base0, base1 = off[c0] + (20 if c0 == 1 else 100) + j, off[c1] + (20 if c1 == 1 else 100) + j
                    for d in (0, 1, 249 - (b1 - b0 + 1), 250 - (b1 - b0 + 1), 550 - (b1 - b0 + 1), 551 - (b1 - b0 + 1)):
                        if c0 == 1 and d > 10:
                            continue                                 # the 60-base contig holds no template
                        L0, L1 = (31, 44) if c0 != 1 else (9, 12)
                        s = [(min(a0, L0 - 1), min(a1, L0 - 1)), (min(b0, L1 - 1), min(b1, L1 - 1))]
                        s = [(x, max(x, y)) for x, y in s]
                        mate(k0, base0, L0, *s[0])
                        mate(k1, base1 + d, L1, *s[1])
                        # and mate 0 to the right (the second TLEN arm), the same template lengths
                        mate(k0, base0 + d + s[1][1] - s[0][1], L0, *s[0])
                        mate(k1, base1, L1, *s[1])
    return b.finish()


# ---- the FASTQ scan: every row unmapped, the expected line written out from the Python parse ----
NL_CLASSES = ((1024, 1023), (1024, 0), (1024, 1), (256, 255), (256, 0), (256, 1), (4, 3), (4, 0))


def scan_cycle(eol=b"\n", n_rec=2000):
    """name lengths chosen record by record so that each of a record's four newlines in turn falls on every offset class"""
    b = Block("scan_cycle" + ("_crlf" if eol != b"\n" else ""), "dense", direct=True, eol=eol)
    at, e = 0, len(eol)
    for i in range(n_rec):
        j, (m, r) = i % 4, NL_CLASSES[(i // 4) % len(NL_CLASSES)]
        s = 1 + (i * 5) % 40
        behind = (0, e + s, 2 * e + s + 1, 3 * e + 2 * s + 1)[j]   # bytes between the header's newline and newline j
        n_name = (r - (at + 1 + (e - 1) + behind)) % m
        if n_name == 0:
            n_name = m
        b.add(bytes(97 + (i + x) % 26 for x in range(n_name)), LETTER[filler(s, i)].tobytes())
        at += 1 + n_name + 4 * e + 2 * s + 1
    return b.finish()


def scan_sizes(k, delta):
    """a block of exactly 1024 k + delta bytes"""
    b = Block("scan_size_%d%+d" % (k, delta), "dense", direct=True)
    recs = [(b"s%d" % i, LETTER[filler(30, i)].tobytes()) for i in range((1024 * k - 150) // 70)]
    have = sum(1 + len(h) + 1 + 2 * (len(s) + 1) + 2 for h, s in recs)
    pad = 1024 * k + delta - have
    assert pad > 0
    recs[-1] = (recs[-1][0] + b"x" * pad, recs[-1][1])
    for h, s in recs:
        b.add(h, s)
    b.finish()
    assert len(b.fq1) == 1024 * k + delta
    return b


def scan_shapes(eol=b"\n", long_names=False):
    """the header, third-line, quality and base shapes; with long_names the names no BAM record holds: empty ones, a 2 100-byte one (two
    tiles without a newline) and its like"""
    b = Block("scan_" + ("long_names" if long_names else "shapes") + ("_crlf" if eol != b"\n" else ""), "dense", direct=True, eol=eol)
    seq = b"ACGTNacgtnRYKMSWBDHVU.-*XACGT"
    heads = (b"a/1", b"/1", b"ab/12", b"a/x", b"abc/1", b"abc/0", b"abc/9", b"ab/", b"a//2", b"name\tcomment/1", b"name comment", b"name/2 c/1",
             b"n\x0bv", b"n\x0cf", b"x" * 254, b"x" * 254 + b"/1", b"@at", b"+plus", b"1/1/1")
    if long_names:
        heads = (b"", b" only a comment", b"\tx", b"x" * 2100, b"x" * 255, b"y" * 1023, b"z" * 1024 + b"/2", b"w" * 3000 + b" c")
    for h in heads:
        for plus in (b"+", b"+" + h[:40]):
            for q0 in (b"@", b"+", b"I"):
                b.add(h, seq, q0 + b"!~" + bytes(33 + x for x in range(len(seq) - 3)), plus)
    return b.finish()


def scan_pairs(r):
    """two blocks, the first of n1 bytes with n1 mod 4 = r: block 2 lies at (n1 + 3) & ~3"""
    b = Block("scan_pairs_%d" % r, "dense", paired=True)
    for p in range(40):
        b.add(b"p%d/1" % p, LETTER[filler(20 + p % 7, p)].tobytes())
        b.add(b"p%d/2" % p, LETTER[filler(33 - p % 5, p + 1)].tobytes())
    b.finish()
    pad = (r - len(b.fq1)) % 4
    h, s, pl, q = b.recs[0]
    b.recs[0] = (b"p0" + b"z" * pad + b"/1", s, pl, q)
    b.finish()
    assert len(b.fq1) % 4 == r
    return b


def scan_blocks():
    return ([scan_cycle(), scan_cycle(b"\r\n", 600), scan_shapes(), scan_shapes(b"\r\n"), scan_shapes(long_names=True), scan_shapes(b"\r\n", True)] + [scan_sizes(2, d) for d in (-1, 0, 1)] + [scan_sizes(1, 0)]
            + [scan_pairs(r) for r in range(4)])


def row_blocks(dense, built):
    out = [md_words_se(dense, 0), md_words_se(dense, 1)] + [md_words_pe(dense, part) for part in range(3)]
    for paired in (False, True):
        out += [xv_cap(dense, paired), walk_block(dense, paired), long_tails(dense, paired), bins_block(built, paired)]
        out += [xa_block(built, c, paired) for c in (0, 1)]
        out += [slot_edges(built, paired, TAIL_CAP - 21 + d) for d in (-1, 0, 1)]
    out += [kinds_se(dense), contig_search(dense, "dense"), contig_search(built, "built"), pe_matrix(built)]
    return out


def all_blocks(dense, built):
    return row_blocks(dense, built) + scan_blocks()


# what all_blocks builds, by name (tests are parametrised before an index exists; test_text_rows_model.py holds the two lists to the builders)
ROW_BLOCKS = (["md_words_se_0", "md_words_se_1", "md_words_pe_0", "md_words_pe_1", "md_words_pe_2"]
              + [n + e for e in ("_se", "_pe") for n in ("xv_cap", "walk", "long_tails", "bins")]
              + ["xa_%s_c%d" % (e, c) for e in ("se", "pe") for c in (0, 1)]
              + ["slot_%s_rg%d" % (e, TAIL_CAP - 21 + d) for e in ("se", "pe") for d in (-1, 0, 1)]
              + ["kinds_se", "contig_search_dense", "contig_search_built", "pe_matrix"])
SCAN_BLOCKS = (["scan_cycle", "scan_cycle_crlf", "scan_shapes", "scan_shapes_crlf", "scan_long_names", "scan_long_names_crlf",
                "scan_size_2-1", "scan_size_2+0", "scan_size_2+1", "scan_size_1+0"] + ["scan_pairs_%d" % r for r in range(4)])
SAM_ONLY = ("scan_cycle", "scan_cycle_crlf", "scan_long_names", "scan_long_names_crlf")      # names no BAM record holds


# ---- the expected bytes ----
def expected_sam(ref, blk):
    opt = blk.opt(ref)
    reads = blk.reads()
    assert len(reads) == len(blk.rows)
    out = []
    if blk.paired:
        for p in range(0, len(reads), 2):
            (n0, s0, q0), (n1, s1, q1) = reads[p], reads[p + 1]
            out.append(ref.ix.sampe(opt, [n0, n1], [s0, s1], [q0, q1], blk.rows[p:p + 2]))
    else:
        for i, (name, codes, qual) in enumerate(reads):
            if blk.direct:
                out.append(name + SE_UNMAPPED_HEAD + LETTER[codes].tobytes() + b"\t" + qual + b"\n")
            else:
                out.append(ref.ix.samse(opt, name, codes, qual, blk.rows[i:i + 1]) + b"\n")
    return b"".join(out)


def expected_bam(ref, sam):
    import salt_amd
    return salt_amd.bam_from_sam(ref.ix, sam)


def bam_able(blk):
    """a BAM record holds a name of 1 to 254 bytes (the host encoder refuses an empty one, the device a longer one)"""
    return all(1 <= len(name) <= 254 for name, _, _ in blk.reads())


# ---- the census ----
def reg2bin(beg, end):
    end -= 1
    for level, (shift, first) in enumerate(((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1))):
        if beg >> shift == end >> shift:
            return level, first + (beg >> shift)
    return 5, 0


def listed_mismatches(ref, codes, row):
    """how many mismatches of the row's M operations show a base the mask lists (sam.c:246-328 without its cap)"""
    sq = revcomp(codes) if row["strand"] == 1 else codes
    g, s, n = int(row["pos"]), int(row["seq_start"]), 0
    for c in row["cigar"][:row["n_cigar"]]:
        k, op = int(c) >> 4, int(c) & 15
        if op == 0:
            a, gb, m = sq[s:s + k], ref.base[g:g + k], ref.mask[g:g + k]
            n += int(((a != gb) & (a < 4) & (((m >> np.minimum(a, 3)) & 1) != 0)).sum())
            g += k
            s += k
        elif op == 1:
            s += k
        else:
            g += k
    return n


def census(refs, pairs):
    """pairs: [(block, expected SAM)].  Counts of every class of record the kernels treat differently; census_check asserts the minimums."""
    import re
    from collections import Counter
    cnt = Counter()
    pos_n, starts, flags, xa_items, nl = set(), set(), set(), set(), set()
    for blk, sam in pairs:
        ref = refs[blk.ref]
        reads = blk.reads()
        lines = [l for l in sam.split(b"\n\n" if blk.paired else b"\n")[:-1]]
        assert len(lines) == len(reads), blk.name
        if blk.direct:
            at = np.nonzero(np.frombuffer(blk.fq1, dtype=np.uint8) == 10)[0]
            for j in range(4):
                for m, r in NL_CLASSES:
                    if (at[j::4] % m == r).any():
                        nl.add((j, m, r))
            cnt["no_newline_tiles"] += int((np.diff(at) > 2048).sum())
            cnt["size_mod_1024=%d" % (len(blk.fq1) % 1024 if len(blk.fq1) % 1024 in (0, 1, 1023) else -1)] += 1
        if blk.paired:
            cnt["pair_block_mod4=%d" % (len(blk.fq1) % 4)] += 1
        for i, ((name, codes, qual), line, row) in enumerate(zip(reads, lines, blk.rows)):
            if line == b"":
                cnt["skipped"] += 1
                continue
            f = line.split(b"\t")
            assert f[0] == name
            flag, L = int(f[1]), len(f[9])
            is_mapped = not flag & 4
            kind = ("pe" if blk.paired else "se") + ("_rev" if flag & 16 else "_fwd")
            head, tail = len(b"\t".join(f[1:9])) + 2, len(line) - len(b"\t".join(f[:11]))
            cnt["unmapped" if not is_mapped else "mapped"] += 1
            cnt["empty_name"] += name == b""
            cnt["name_over_254"] += len(name) > 254
            cnt["len=%d" % L] += 1
            if blk.paired:
                flags.add(flag)
                cnt["odd_len_rev"] += bool(flag & 16 and L & 1)
            if not is_mapped:
                continue
            cnt["odd_len_rev"] += bool(flag & 16 and L & 1)
            cnt["head=%d_%s" % (head, kind)] += 1
            cnt["tail=%d_%s" % (tail, kind)] += 1
            cnt["head_over"] += head > HEAD_CAP
            cnt["tail_over"] += tail > TAIL_CAP + 100
            cig = re.findall(rb"(\d+)([MIDS])", f[5])
            cnt["cigar_words=%d" % len(cig) if len(cig) in (BAM_HEAD_WORDS, BAM_HEAD_WORDS + 1) else "cigar_words_other"] += 1
            cnt["cigar_words_over"] += len(cig) > BAM_HEAD_WORDS
            cnt["soft_clipped"] += any(o == b"S" for _, o in cig)
            on_ref = sum(int(n) for n, o in cig if o in b"MD")
            beg = int(f[3]) - 1
            level, _ = reg2bin(beg, beg + max(on_ref, 1))
            cnt["bin_level=%d" % level] += 1
            for sh in (14, 17, 20):
                cnt["straddles_2^%d" % sh] += (beg >> sh) != ((beg + on_ref - 1) >> sh)
                cnt["ends_on_2^%d" % sh] += (beg + on_ref) % (1 << sh) == 0
            tags = {t[:2]: t[5:] for t in f[11:]}
            for t in f[11:]:
                if t.startswith(b"XA:Z:"):
                    xa_items.add((int(row["n_hits"][0]), int(row["n_hits"][1]), t.count(b";")))
                    cnt["xa_gapped_64"] += len(re.findall(rb"(?:\d+[MID]){64},", t))
            if b"NM" in tags:
                nm = int(tags[b"NM"])
                cnt["nm_C" if nm < 256 else "nm_S"] += 1
                cnt["nm=255"] += nm == 255
                cnt["nm=256"] += nm == 256
                words = row["n_cigar"] == 1 and (row["cigar"][0] & 15) == 0 and not (codes > 3).any()
                cnt["words_path" if words else "walk_path"] += 1
                cnt["walk_one_N"] += (not words) and row["n_cigar"] == 1
                n = int(row["cigar"][0]) >> 4
                if words:
                    pos_n.add((int(row["pos"]) & 15, n % 16))
                    starts.add(int(row["seq_start"]) & 15)
                    cnt["words_ends_on_last_base"] += int(row["pos"]) + n == ref.ref_len
                    cnt["words_strand%d" % row["strand"]] += 1
                    md = re.findall(rb"\d+|[ACGT]", tags[b"MD"])
                    cnt["md_first_col"] += n > 0 and not md[0].isdigit()
                    cnt["md_last_col"] += n > 0 and not md[-1].isdigit()
                if b"XV" in tags:
                    xv = [int(x) for x in tags[b"XV"].split(b",")]
                    cnt["xv_lists"] += 1
                    if words:
                        cnt["xv_col0_of_window"] += any(x % 16 == 0 for x in xv)
                        cnt["xv_col15_of_window"] += any(x % 16 == 15 for x in xv)
                    if len(xv) == XV_CAP and listed_mismatches(ref, codes, row) > XV_CAP:
                        cnt["xv_cut_words" if words else "xv_cut_walk"] += 1
                    cnt["xv_63"] += len(xv) == XV_CAP - 1
                    assert len(xv) <= XV_CAP
    return cnt, pos_n, starts, flags, xa_items, nl


def pe_matrix_flags():
    """the flags of alnpe_sam over {U, F, R}^2, without and with 0x2"""
    out = set()
    for me in PE_KINDS:
        for ot in PE_KINDS:
            for first in (0x40, 0x80):
                out.add(1 | (4 if me == "U" else 0) | (8 if ot == "U" else 0) | (0x10 if me == "R" else 0) | (0x20 if ot == "R" else 0) | first)
    return out


def census_check(result):
    cnt, pos_n, starts, flags, xa_items, nl = result
    need = {"words_path": 5000, "walk_path": 800, "walk_one_N": 700, "words_strand0": 2000, "words_strand1": 2000, "words_ends_on_last_base": 100,
            "md_first_col": 500, "md_last_col": 500, "xv_col0_of_window": 100, "xv_col15_of_window": 100,
            "xv_cut_words": 4, "xv_cut_walk": 4, "xv_63": 2, "nm_C": 1000, "nm_S": 4, "nm=255": 2, "nm=256": 2,
            "cigar_words=15": 1, "cigar_words=16": 1, "cigar_words_over": 8, "soft_clipped": 1000, "odd_len_rev": 100,
            "head_over": 10, "tail_over": 8, "skipped": 10, "unmapped": 1000, "mapped": 10000, "empty_name": 4, "name_over_254": 10,
            "bin_level=0": 1000, "bin_level=1": 4, "bin_level=2": 2, "bin_level=3": 2, "straddles_2^14": 4, "straddles_2^17": 2, "straddles_2^20": 2,
            "ends_on_2^14": 2, "ends_on_2^17": 1, "xa_gapped_64": 20, "no_newline_tiles": 1,
            "size_mod_1024=0": 2, "size_mod_1024=1": 1, "size_mod_1024=1023": 1}
    for L in (1, 2, 7, 8, 9, 15, 16, 17, 33, 255, 256, 257, 512):
        need["len=%d" % L] = 3
    for r in range(4):
        need["pair_block_mod4=%d" % r] = 1
    for kind in ("se_fwd", "se_rev", "pe_fwd", "pe_rev"):
        for h in (HEAD_CAP - 1, HEAD_CAP, HEAD_CAP + 1):
            need["head=%d_%s" % (h, kind)] = 1
        for t in (TAIL_CAP - 1, TAIL_CAP, TAIL_CAP + 1):
            need["tail=%d_%s" % (t, kind)] = 1
    short = {k: (cnt[k], v) for k, v in need.items() if cnt[k] < v}
    assert not short, "classes below their minimum (have, need): %r" % short
    assert pos_n == {(p, n) for p in range(16) for n in range(16)}, "missing (pos & 15, n mod 16): %r" % sorted({(p, n) for p in range(16) for n in range(16)} - pos_n)
    assert starts == set(range(16)), starts
    want = pe_matrix_flags()
    assert want <= {f & ~2 for f in flags}, sorted(want - {f & ~2 for f in flags})
    assert {f for f in flags if f & 2} >= {f | 2 for f in want if not f & 12}, "a proper-pair flag is missing"
    # every split of 0 .. 5 hits over the strands, whole and with one hit left out
    assert {(a, b) for a, b, _ in xa_items} >= {(a, b) for a in range(6) for b in range(6 - a) if a + b}, xa_items
    assert any(n < a + b for a, b, n in xa_items)
    assert nl == {(j, m, r) for j in range(4) for m, r in NL_CLASSES}, sorted({(j, m, r) for j in range(4) for m, r in NL_CLASSES} - nl)
