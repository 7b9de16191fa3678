"""The gapped-pass fixture (tests/golden/make_gap_fixture.py) as the tests see it: its cases, and loaders for its files.

Every read of these files was built to have no gap-free hit, so each of them takes the gapped pass of the aligner: single-end reads of
40..512 bases with insertions / deletions of 1..L/10+1 bases at both sides of the 8-base words of the nibble-packed text windows, reads
whose Landau-Vishkin window ends at the genome's end -1 / +0 / +1, and pairs whose mates of 100..250 bases carry the indel.  The files
are cut where the aligner changes route: `se_lane` (L <= 129: one candidate per lane, k_gap), `se_mid` (130..168: the inline wave
route at a window that would still fit the lanes), `se_long` (>= 170), `pe_short` (mates <= 164: k_gap at k = 3) and `pe_long`."""
import collections
import gzip
import os
import re
import sys

import numpy as np

from conftest import LAMBDA, ROOT

# name -> (salt arguments, FASTQ file names under tests/golden/lambda, each stored as <name>.gz); the golden SAM is expect_<name>.sam.gz
GAP_CASES = {
    "gap_se_lane": (["-d", "-c"], ["reads_gap_se_lane.fq"]),
    "gap_se_mid": (["-d", "-c"], ["reads_gap_se_mid.fq"]),
    "gap_se_long": (["-d", "-c"], ["reads_gap_se_long.fq"]),
    "gap_pe_short": (["-d", "-p", "-c", "-a", "300", "-b", "700"], ["reads_gap_pe_short_1.fq", "reads_gap_pe_short_2.fq"]),
    "gap_pe_long": (["-d", "-p", "-c", "-a", "300", "-b", "700"], ["reads_gap_pe_long_1.fq", "reads_gap_pe_long_2.fq"]),
}
SE_CASES = [c for c in sorted(GAP_CASES) if len(GAP_CASES[c][1]) == 1]
PE_CASES = [c for c in sorted(GAP_CASES) if len(GAP_CASES[c][1]) == 2]

# what the fixture is for, per case: (records, records whose own CIGAR has an I or D, records with an XA tag) at the least.  The
# oracle test asserts these on the golden files, so that no regenerated fixture can lose its gapped reads unnoticed.
MINIMA = {
    "gap_se_lane": (1300, 500, 150),
    "gap_se_mid": (1200, 500, 60),
    "gap_se_long": (600, 250, 30),
    "gap_pe_short": (960, 250, 40),
    "gap_pe_long": (960, 250, 25),
}
MIN_GAPPED_PER_LENGTH = 40


def paths(case):
    return [os.path.join(LAMBDA, f + ".gz") for f in GAP_CASES[case][1]]


def plain_paths(case, tmp_dir):
    """the FASTQ files of a case unpacked into tmp_dir, for the programs that are to read plain text"""
    out = []
    for f in GAP_CASES[case][1]:
        out.append(os.path.join(str(tmp_dir), f))
        with gzip.open(os.path.join(LAMBDA, f + ".gz"), "rb") as src, open(out[-1], "wb") as dst:
            dst.write(src.read())
    return out


def golden(case):
    with gzip.open(os.path.join(LAMBDA, "expect_%s.sam.gz" % case), "rb") as f:
        return f.read()


def records(sam):
    return [l.split(b"\t") for l in sam.split(b"\n") if l and not l.startswith(b"@")]


def census(sam):
    """(records, gapped records, records with XA, {read length: gapped records}) of a SAM text"""
    recs = records(sam)
    by_len = {}
    n_gap = n_xa = 0
    for t in recs:
        g = re.search(b"[ID]", t[5]) is not None
        by_len[len(t[9])] = by_len.get(len(t[9]), 0) + g
        n_gap += g
        n_xa += any(x.startswith(b"XA:Z:") for x in t[11:])
    return len(recs), n_gap, n_xa, by_len


def xa_gapped(sam):
    """records whose XA list names a hit with an I or D in that hit's own CIGAR (XA:Z:contig,+pos,CIGAR,NM;...)"""
    n = 0
    for t in records(sam):
        xa = [x[5:] for x in t[11:] if x.startswith(b"XA:Z:")]
        n += any(re.search(b"[ID]", h.split(b",")[2]) is not None for x in xa for h in x.split(b";") if h.count(b",") >= 3)
    return n


def diff_message(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
    msg = "\n".join("line %d\n  got  %r\n  want %r" % (i, g[i][:400], w[i][:400]) for i in bad[:5])
    return "%d differing lines (got %d, want %d)\n%s" % (len(bad), len(g), len(w), msg)


# ---- unit vectors of the Landau-Vishkin chain (oracle/ref_harness.c; tests/golden/lv_vectors*.txt[.gz]) ----
LLV_K, LLV_TW = 12, 22                 # salt_align.hip: the lane kernel takes bounds up to LLV_K and windows of L + 4 <= 8 * (LLV_TW - 1) = 168
MAX_CIGAR_OPS = 64                     # SALT_MAX_CIGAR_OPS
LvVector = collections.namedtuple("LvVector", "pos kmis kdiff seq mis diff cret cigar")


def lanes_fit(L, kdiff):
    return kdiff <= LLV_K and L + 4 <= 8 * (LLV_TW - 1)


def load_lv_vectors(path):
    """(reference length, its nibble-packed words, [LvVector])"""
    l_ref, ref, vecs = 0, None, []
    with (gzip.open if path.endswith(".gz") else open)(path, "rt") as f:
        for line in f:
            t = line.split()
            if t[0] == "R":
                l_ref, ref = int(t[1]), np.array([int(x, 16) for x in t[2:]], dtype=np.uint32)
                continue
            vecs.append(LvVector(int(t[1]), int(t[3]), int(t[4]), np.frombuffer(t[5].encode(), dtype=np.uint8) - 48,
                                 int(t[6]), int(t[7]), int(t[8]), t[9]))
    return l_ref, ref, vecs


def check_lv_vector_census(l_ref, vecs):
    """what lv_vectors_shapes.txt.gz is for; asserted where the file is read without a GPU"""
    n_ops = lambda v: len(re.findall("[MID]", v.cigar))
    groups = collections.Counter((len(v.seq), v.kdiff) for v in vecs if lanes_fit(len(v.seq), v.kdiff))
    assert sum(c >= 64 for c in groups.values()) >= 20, groups                         # (L, k) with 64 different cases for the 64 lanes
    fit = [v for v in vecs if lanes_fit(len(v.seq), v.kdiff)]
    assert len(fit) >= 1500 and sum(v.diff >= 0 for v in fit) >= 800 and sum(v.diff == -1 for v in fit) >= 300
    assert sum(len(v.seq) in (164, 165, 168) for v in vecs) >= 100 and sum(len(v.seq) >= 300 for v in vecs) >= 100
    assert sum(0 <= v.diff < 31 and re.search("[ID]", v.cigar) is not None for v in vecs) >= 1000
    assert sum(v.diff >= 13 for v in vecs) >= 50                                       # beyond the lane kernel's bound: the wave kernel alone
    for d in (-2, -1, 0, 1):                                                           # windows that end at the reference's end + d; + 1 is outside
        at = [v for v in vecs if v.pos + len(v.seq) + 4 == l_ref + d]
        assert len(at) >= 40 and (all(v.diff == -1 for v in at) if d == 1 else any(v.diff >= 0 for v in at)), d
    assert sum(v.pos == 0 for v in vecs) >= 50 and sum((v.seq == 4).any() for v in vecs) >= 300
    assert all(n_ops(v) <= MAX_CIGAR_OPS for v in vecs)


def run_lv_units(path):
    """The vectors of `path` through salt_gpu_diag_lv, every answer asserted: mismatch_capped, lv_wave, the CIGAR of lv_cigar, and the
    one-candidate-per-lane kernel (lane_text + lv_lanes) EXACTLY where the case is within its limits (LLV_K, LLV_TW) and -2 elsewhere.
    Returns (vectors, vectors the lane kernel answered)."""
    import ctypes
    import salt_amd
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_diag_lv.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 6
    l_ref, ref, vecs = load_lv_vectors(path)
    n = len(vecs)
    pos_a, kd_a = np.array([v.pos for v in vecs], dtype=np.uint32), np.array([v.kdiff for v in vecs], dtype=np.uint32)
    seq_a = np.concatenate([v.seq for v in vecs]).astype(np.uint8)
    off_a = np.concatenate([[0], np.cumsum([len(v.seq) for v in vecs])]).astype(np.uint32)
    out = np.zeros((n, 4), dtype=np.int32)
    cig = np.zeros((n, MAX_CIGAR_OPS), dtype=np.uint16)
    rc = lib.salt_gpu_diag_lv(ref.ctypes.data, l_ref, n, pos_a.ctypes.data, kd_a.ctypes.data, seq_a.ctypes.data,
                              off_a.ctypes.data, out.ctypes.data, cig.ctypes.data)
    assert rc == 0, lib.salt_gpu_last_error()
    n_lane = 0
    for i, v in enumerate(vecs):
        L = len(v.seq)
        if v.mis != -9:                                                                # -9: the read hangs over the reference's end
            got = int(out[i, 0])
            assert (got if got <= v.kmis else -1) == v.mis, ("mismatch", i, out[i], v)
        assert int(out[i, 1]) == v.diff, ("lv_wave", i, out[i], v)
        if lanes_fit(L, v.kdiff):
            assert int(out[i, 2]) == v.diff, ("lv_lanes", i, out[i], v)
            n_lane += 1
        else:
            assert int(out[i, 2]) == -2, ("lv_lanes beyond its limits", i, out[i], v)
        if 0 <= v.diff < 31:
            got = "".join("%d%s" % (int(x) >> 4, "MID"[int(x) & 3]) for x in cig[i, :max(int(out[i, 3]), 0)])
            assert got == v.cigar, ("cigar", i, got, v)
    return n, n_lane


# ---- the fixture through the library (also the child process of the route legs) ----
def align_case(salt_amd, idx, aln, case):
    """the SAM text of one case through GpuAligner.alnse_core1 / alnpe_core1 + sam_text / sam_text_pe"""
    args, _ = GAP_CASES[case]
    opt, _ = salt_amd.AlnOpt.from_argv(list(args), idx.l_seed)
    fqs = paths(case)
    if len(fqs) == 1:
        names, seqs, offs, quals = salt_amd.read_fastq(fqs[0])
        return salt_amd.sam_text(idx, opt, names, seqs, offs, quals, aln.alnse_core1(opt, seqs, offs))
    names, seqs, offs, quals = salt_amd.interleave_pairs(salt_amd.read_fastq(fqs[0]), salt_amd.read_fastq(fqs[1]))
    return salt_amd.sam_text_pe(idx, opt, names, seqs, offs, quals, aln.alnpe_core1(opt, idx, seqs, offs))


def main(out_dir, cases):
    """Child process of a route leg (the switches are read once per process): each case through the library on one workspace, the SAM
    bytes to out_dir/<case>.sam, and the workspace's counters after each case (reads k_light queued for k_heavy, reads that asked for a
    k_gap slot, k_gap items) to out_dir/counts.json."""
    import json
    sys.path.insert(0, ROOT)
    try:
        import torch                              # torch's HIP context first, as in the test session (tests/conftest.py)
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=4096)
    counts = {}
    for case in cases:
        sam = align_case(salt_amd, idx, aln, case)
        q = aln.queue_counts()
        counts[case] = {"heavy_reads": int(len(aln.heavy_reads())), "gap_slots_asked": int(q[2]), "gap_items": int(q[5])}
        with open(os.path.join(out_dir, case + ".sam"), "wb") as f:
            f.write(sam)
    aln.close()
    idx.destroy()
    with open(os.path.join(out_dir, "counts.json"), "w") as f:
        json.dump(counts, f)
    print("gap routes: %s" % counts)


# ---- reads inside a tandem repeat (test_gpu_gap.py, against the oracle) ----
REPEAT_LENS = (100, 129, 130, 164)


def repeat_genome():
    """(genome codes, SNP positions, SNP masks): 4 000 diverged copies of a 30-base unit between two 1 000-base flanks, ~600 SNPs"""
    from salt_amd import workload
    genome = workload.make_tandem(30, 4000, 0.01, 1000)
    pos, mask = workload.make_snps(genome, 600, seed=5)
    return genome, pos, mask


def repeat_reads(genome, n, seed):
    """n reads of REPEAT_LENS bases from INSIDE the block of copies, each with one insertion or deletion of 1, 2, 3, L/10 - 1 or L/10 bases
    at one of the fixture's positions, half of them reverse-complemented: (codes, offsets).  The reference keeps a strand's alternative
    hits only when the first of them is as good as the best hit, so in diverged copies XA lists are rare; most reads here come from
    stretches of exact copies, where they are not."""
    rng = np.random.default_rng(seed)
    lo, hi = 1000 + 300, len(genome) - 1000 - 300
    seqs, offs = [], [0]
    for i in range(n):
        L = REPEAT_LENS[i % len(REPEAT_LENS)]
        size = int(rng.choice([1, 2, 3, L // 10 - 1, L // 10]))
        p = int(rng.choice([0, 1, 2, 3, 7, 8, 9, L // 2, L - 9, L - 8, L - 3, L - 2, L - 1] + [7, 8, 9, L // 2, L - 9, L - 8]))   # an indel at a read's end rarely needs a gap
        while True:                                   # three reads of four from copies without a diverged base: hundreds of copies tie with them
            start = int(rng.integers(lo, hi - L - 2 * size - 8))
            w = genome[start - 30:start + L + 60]
            if i % 4 == 0 or (w[30:] == w[:-30]).all():
                break
        src = genome[start:start + L + 2 * size + 8].copy()
        if rng.random() < 0.5:
            r = np.concatenate([src[:p], rng.integers(0, 4, size).astype(np.uint8), src[p:]])[:L]
        else:
            r = np.concatenate([src[:p], src[p + size:]])[:L]
        if rng.random() < 0.5:
            r = (3 - r[::-1]).astype(np.uint8)
        seqs.append(r.astype(np.uint8)); offs.append(offs[-1] + L)
    return np.concatenate(seqs), np.array(offs, dtype=np.uint32)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
