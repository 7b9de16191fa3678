"""The tail of the gapped chain: k_gapfin's candidate rule on lists in global memory (rule_unsorted with GAPFIN_B trips of rows in
flight, k_diag_rule mode 5), lv_cigar with its tables in the block's LDS (k_diag_lv's flag, what k_cigar runs for a distance of at
most LLV_K), and the chain itself on a batch in which every read needs the gapped pass, single end and as pairs."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import gap_cases
from conftest import GOLDEN, LAMBDA, ROOT

pytestmark = pytest.mark.gpu

GAPFIN_B = 8                            # salt_align.hip: trips of 64 rows k_gapfin asks for together
LLV_K = gap_cases.LLV_K


# ---- the rule on global lists ----
def _sequential_rule(pos, val, bound, vmax, in_range):
    """The reference's candidate loop on the SORTED, duplicate-free list (code_kdiff alnse.c:371-393 as alnse_check_withgap drives
    it): what the kernels must reproduce on the unsorted list."""
    seen, cand = set(), []
    for p, v in sorted(zip(pos, val)):
        if p in seen:
            continue
        seen.add(p)
        if in_range(p):
            cand.append((p, v))
    found, best_pos, best_v, hits, a0 = 0, 0, 0, [], 0
    for p, v in cand:
        if v > vmax or v > bound:
            continue
        if v < bound or not found:
            bound, best_pos, best_v = v, p, v
        if len(hits) < 6:
            hits.append((p, v))
        if not found:
            a0 = v
        found = 1
    return found, best_pos, best_v, hits, a0, bound


def _rule_cases(L, ref_len):
    """(pos, val, bound) per case: every list length at which the front end takes another path (no row, one trip or less, a batch
    of GAPFIN_B trips less one row / exactly / and one row, the cap of a strand's list) x 0, 1, 64 and 65 rows inside the bound (the
    copy of P's members into the lanes ends at 64) x the incoming bounds x distinct or repeated positions.  The rows outside the
    bound hold every distance above it (and 255), a row AT the range filter's edge with distance 0 (p + L + 4 == ref_len: filtered)
    and, among the members, a row one base under it."""
    rng = np.random.Generator(np.random.PCG64(19))
    edge = ref_len - L - 4
    cases = []
    for n in (0, 1, 63, 64, 65, 64 * GAPFIN_B - 1, 64 * GAPFIN_B, 64 * GAPFIN_B + 1, 1000, 1024):
        for m in (0, 1, 64, 65):
            if m > n:
                continue
            for bound in (0, 3, 10, 12):
                for dup in (False, True):
                    pos = np.zeros(n, dtype=np.int64)
                    val = np.zeros(n, dtype=np.int64)
                    inside = rng.permutation(n)[:m]
                    out = np.setdiff1d(np.arange(n), inside)
                    # members: positions all over the reference (or few distinct ones, each with one distance), one at the edge - 1
                    n_loci = max(1, m // 3) if dup else max(1, m)
                    loci = rng.choice(edge - 1, size=n_loci, replace=False)
                    if m and rng.random() < 0.5:
                        loci[0] = edge - 1
                    dist = rng.integers(0, bound + 1, size=n_loci)
                    pick = rng.integers(0, n_loci, size=m) if dup else rng.permutation(n_loci)[:m]
                    pos[inside], val[inside] = loci[pick], dist[pick]
                    # the others: another set of positions, every distance above the bound, or filtered by the range
                    o_loci = np.setdiff1d(rng.choice(edge - 1, size=max(1, len(out) // 3 if dup else len(out)), replace=False), loci)
                    if len(o_loci) == 0:
                        o_loci = np.setdiff1d(np.arange(5), loci)[:1]
                    above = [v for v in range(bound + 1, 13)] + [255]
                    o_dist = rng.choice(above, size=len(o_loci))
                    opick = rng.integers(0, len(o_loci), size=len(out))
                    pos[out], val[out] = o_loci[opick], o_dist[opick]
                    if len(out):                                                       # at the filter's edge and beyond it, distance 0
                        pos[out[0]], val[out[0]] = edge, 0
                    if len(out) > 1:
                        pos[out[1]], val[out[1]] = edge + 1 + int(rng.integers(0, 50)), 0
                    cases.append((pos.astype(np.uint32), val.astype(np.uint8), bound))
    # and lists without a plan: random lengths up to the cap, few or many loci, some straddling the reference's end
    for c in range(400):
        n = int(rng.choice([0, 1, 2, 17, 64, 65, 200, 511, 512, 513, 700, 1000]))
        n_distinct = int(rng.choice([1, 2, 3, 8, 100, 2000]))
        lo = ref_len - 300 if rng.random() < 0.2 else 0
        universe = rng.integers(lo, ref_len + 150 if lo else ref_len - 300, size=n_distinct, dtype=np.int64)
        p = universe[rng.integers(0, n_distinct, size=n)]
        dist_of = {int(u): int(rng.choice([0, 1, 2, 3, 4, 7, 10, 12, 200], p=[.05, .1, .1, .1, .1, .1, .1, .1, .25])) for u in universe}
        v = np.array([dist_of[int(x)] for x in p], dtype=np.int64)
        v[v > 12] = 255
        cases.append((p.astype(np.uint32), v.astype(np.uint8), int(rng.choice([0, 3, 10, 12]))))
    return cases


def _run_rule(lib, cases, L, ref_len, mode):
    n_cases = len(cases)
    offs = np.zeros(n_cases + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(c[0]) for c in cases])
    pos_a = np.concatenate([c[0] for c in cases]).astype(np.uint32)
    val_a = np.concatenate([c[1] for c in cases]).astype(np.uint8)
    b_a = np.array([c[2] for c in cases], dtype=np.uint32)
    out = np.zeros((n_cases, 18), dtype=np.uint32)
    rc = lib.salt_gpu_diag_rule(n_cases, pos_a.ctypes.data, val_a.ctypes.data, offs.ctypes.data, b_a.ctypes.data, L, ref_len, mode, out.ctypes.data)
    assert rc == 0, lib.salt_gpu_last_error()
    return out


def test_gpu_rule_on_global_lists_equals_the_sequential_rule():
    """k_diag_rule mode 5 (the rule as k_gapfin runs it: the first batch of rows asked for ahead, two batches in flight, the hit
    passes of a list with more than 64 members a batch at a time) against the sequential loop over the sorted unique list, and
    against mode 2 (the same rule, a trip at a time) on every case."""
    import salt_amd
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_diag_rule.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    L, ref_len, vmax = 100, 1000000, 12
    in_range = lambda p: not ((p + L + 4) & 0xFFFFFFFF >= ref_len)
    cases = _rule_cases(L, ref_len)
    lens = {len(c[0]) for c in cases}
    assert {0, 1, 63, 64, 65, 511, 512, 513, 1000, 1024} <= lens
    got5, got2 = _run_rule(lib, cases, L, ref_len, 5), _run_rule(lib, cases, L, ref_len, 2)
    members = set()
    for c, (pos, val, b) in enumerate(cases):
        found, bp, bv, hits, a0, bound = _sequential_rule([int(x) for x in pos], [int(x) for x in val], b, vmax, in_range)
        want = [found, bp if found else 0, bv if found else 0, len(hits), a0 if hits else 0, bound]
        for h in range(6):
            want += list(hits[h]) if h < len(hits) else [0, 0]
        assert [int(x) for x in got5[c]] == want, ("mode 5", c, len(pos), b, got5[c].tolist(), want)
        assert [int(x) for x in got2[c]] == want, ("mode 2", c, len(pos), b, got2[c].tolist(), want)
        members.add(int(sum(1 for p, v in zip(pos, val) if v <= b and in_range(int(p)))))
    assert {0, 1, 64, 65} <= members, sorted(members)[:20]            # rows inside the bound: the lane copy's boundary was met


# ---- lv_cigar with its tables in LDS ----
def _run_lv(lib, ref, l_ref, pos, kdiff, seqs, lds_tab):
    n = len(pos)
    pos_a, kd_a = np.array(pos, dtype=np.uint32), np.array(kdiff, dtype=np.uint32)
    seq_a = np.concatenate(seqs).astype(np.uint8)
    off_a = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint32)
    out = np.zeros((n, 4), dtype=np.int32)
    cig = np.zeros((n, gap_cases.MAX_CIGAR_OPS), dtype=np.uint16)
    rc = lib.salt_gpu_diag_lv_tab(ref.ctypes.data, l_ref, n, pos_a.ctypes.data, kd_a.ctypes.data, seq_a.ctypes.data, off_a.ctypes.data,
                                  out.ctypes.data, cig.ctypes.data, lds_tab)
    assert rc == 0, lib.salt_gpu_last_error()
    return out, cig


def _lv_lib():
    import salt_amd
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_diag_lv_tab.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 6 + [ctypes.c_int]
    return lib


def _cigar_text(words, n):
    return "".join("%d%s" % (int(x) >> 4, "MID"[int(x) & 3]) for x in words[:max(int(n), 0)])


def test_gpu_lv_cigar_from_lds_tables_on_the_shape_vectors():
    """The shape vectors of oracle/ref_harness.c --shapes through lv_cigar twice: tables in global memory (the present mode) and
    placed as k_cigar places them (LDS up to a distance of LLV_K, global memory above).  Op for op the same, and the recorded CIGAR."""
    lib = _lv_lib()
    l_ref, ref, vecs = gap_cases.load_lv_vectors(os.path.join(GOLDEN, "lv_vectors_shapes.txt.gz"))
    args = ([v.pos for v in vecs], [v.kdiff for v in vecs], [v.seq for v in vecs])
    out_g, cig_g = _run_lv(lib, ref, l_ref, *args, 0)
    out_l, cig_l = _run_lv(lib, ref, l_ref, *args, 1)
    assert (out_g == out_l).all() and (cig_g == cig_l).all(), np.nonzero((out_g != out_l).any(axis=1) | (cig_g != cig_l).any(axis=1))[0][:10]
    n_lds = n_glob = 0
    for i, v in enumerate(vecs):
        assert int(out_l[i, 1]) == v.diff, ("lv_wave", i, out_l[i], v)
        if 0 <= v.diff < 31:
            assert _cigar_text(cig_l[i], out_l[i, 3]) == v.cigar, ("cigar", i, _cigar_text(cig_l[i], out_l[i, 3]), v)
            n_lds += 1 <= v.diff <= LLV_K
            n_glob += v.diff > LLV_K
    assert n_lds >= 800 and n_glob >= 50, (n_lds, n_glob)             # tracebacks out of LDS, and the ones that keep the global table
    # the restated algorithm, the reference of the generated cases below, on every seventh vector: the recorded distance and CIGAR
    mask_at = lambda i: int((ref[i >> 3] >> (4 * (i & 7))) & 15) if i < l_ref else 0
    n_model = 0
    for v in vecs[::7]:
        L = len(v.seq)
        if v.pos + L + 4 > l_ref:
            continue
        e, _, text = _lv_model([mask_at(v.pos + i) for i in range(L + 4)], [(1 << int(c)) if c < 4 else 15 for c in v.seq], v.kdiff)
        assert e == v.diff and (not 0 <= v.diff < 31 or text == v.cigar), ("model", v.pos, L, v.kdiff, e, v.diff, text, v.cigar)
        n_model += 1
    assert n_model >= 400, n_model


def _lv_model(T, P, k):
    """lv_wave + lv_cigar's traceback restated (computeEditDistanceWithCigar, useM = 1, LandauVishkin.c:230-330): T text masks, P the
    read's one-hot masks, zero behind both.  Returns (e, finishing diagonal, CIGAR text); e = -1: more than k."""
    tlen, plen = len(T), len(P)
    tz = lambda i: T[i] if 0 <= i < tlen else 0
    pz = lambda i: P[i] if 0 <= i < plen else 0
    end0 = min(plen, tlen)
    i = 0
    while i < end0 and (P[i] & T[i]):
        i += 1
    if i == end0:
        return (plen - end0 if plen > end0 else 0), 0, "%dM" % plen
    ds = list(range(-31, 33))
    prev = {d: -2 for d in ds}
    prev[0] = i
    Ls, As = [dict(prev)], [{}]
    for e in range(1, min(k, 30) + 1):
        cur, act = {}, {}
        for d in ds:
            left = prev[d - 1] if d > -31 else -2
            right = prev[d + 1] if d < 32 else -2
            best, a = prev[d] + 1, "X"
            if left > best:
                best, a = left, "D"
            if right + 1 > best:
                best, a = right + 1, "I"
            c = -2
            if abs(d) <= e and abs(d) <= 30:
                if pz(best) == tz(d + best):
                    end = min(plen, tlen - d)
                    if best >= end:
                        best = end
                    else:
                        j = best
                        while j < end and (pz(j) & tz(d + j)):
                            j += 1
                        best = j
                c = best
            cur[d], act[d] = c, a
        Ls.append(cur)
        As.append(act)
        reach = [d for d in ds if abs(d) <= e and abs(d) <= 30 and cur[d] == plen]
        if reach:
            d_fin = min(reach, key=lambda d: 0 if d == 0 else (2 * -d - 1 if d < 0 else 2 * d))
            acts, matched, cd = {}, {}, d_fin
            for ce in range(e, 0, -1):
                a = As[ce][cd]
                acts[ce] = a
                c = Ls[ce][cd]
                if a == "I":
                    matched[ce] = c - Ls[ce - 1][cd + 1] - 1
                    cd += 1
                elif a == "D":
                    matched[ce] = c - Ls[ce - 1][cd - 1]
                    cd -= 1
                else:
                    matched[ce] = c - Ls[ce - 1][cd] - 1
            ops, acc, ce = [], Ls[0][0], 1
            while ce <= e:
                a, cnt = acts[ce], 1
                while ce + 1 <= e and matched[ce] == 0 and acts[ce + 1] == a:
                    cnt += 1
                    ce += 1
                if a == "X":
                    acc += cnt
                else:
                    if acc:
                        ops.append("%dM" % acc)
                    acc = 0
                    ops.append("%d%s" % (cnt, a))
                if matched[ce] > 0:
                    acc += matched[ce]
                ce += 1
            if acc:
                ops.append("%dM" % acc)
            return e, d_fin, "".join(ops)
        prev = cur
    return -1, 0, ""


def _generated_lv_cases():
    """Reads against a random genome without SNPs, built for a distance k and a finishing diagonal: k substitutions (diagonal 0), k
    inserted bases (-k), deleted reference bases (+).  The window is four bases longer than the read, so no traceback ends above
    diagonal +4: for k = 12 and 13 the "+" cases are 4 deleted bases and k - 4 substitutions.  Every length also with the window
    ending at the genome's last base.  (pos, read, k wanted, diagonal wanted) -- what the cases turn out to be is asserted on the
    restated algorithm by the caller."""
    rng = np.random.Generator(np.random.PCG64(7))
    l_ref = 4000
    genome = rng.integers(0, 4, l_ref).astype(np.uint8)
    cases = []
    for L in (21, 100, 120, 129):
        for k in ((1,) if L == 21 else (1, 12, 13)):
            for sign in (-1, 0, 1):
                for at_end in (False, True):
                    for _ in range(6):
                        p = l_ref - L - 4 if at_end else int(rng.integers(0, l_ref - L - 40))
                        n_del = min(k, 4) if sign > 0 else 0
                        n_ins = k if sign < 0 else 0
                        n_sub = k - n_del - n_ins
                        src = genome[p:p + L + n_del - n_ins].copy()
                        a = int(rng.integers(L // 3, 2 * L // 3 - n_ins)) if L > 21 else 8
                        if n_ins:
                            ins = (genome[p + a:p + a + n_ins] + 1 + rng.integers(0, 3, n_ins)) % 4     # none equal to the base it is put in front of
                            read = np.concatenate([src[:a], ins.astype(np.uint8), src[a:]])
                        elif n_del:
                            read = np.concatenate([src[:a], src[a + n_del:]])
                        else:
                            read = src
                        read = read[:L].copy()
                        assert len(read) == L
                        if n_sub:                                                   # substitutions away from the indel and from each other
                            spots = [s for s in range(2, L - 2, max(2, (L - 4) // (n_sub + 1))) if abs(s - a) > n_ins + n_del + 2][:n_sub]
                            for s in spots:
                                read[s] = (read[s] + 1 + rng.integers(0, 3)) % 4
                        cases.append((p, read.astype(np.uint8), k, sign * (n_ins if sign < 0 else n_del)))
    ref = np.zeros((l_ref + 7) // 8 + 4, dtype=np.uint32)
    for i, c in enumerate(genome):
        ref[i >> 3] |= np.uint32(1 << int(c)) << np.uint32(4 * (i & 7))
    return l_ref, genome, ref, cases


def test_gpu_lv_cigar_from_lds_tables_at_the_bounds_edges():
    """Generated tracebacks at distance 1, 12 (the last that takes the LDS tables) and 13 (the first that takes the global one), ending
    on the lowest diagonal, on diagonal 0 and on the highest the window admits, for reads of 21, 100, 120 and 129 bases, also with
    the window ending at the genome's last base: both placements of the tables op for op, and the restated algorithm's CIGAR."""
    lib = _lv_lib()
    l_ref, genome, ref, cases = _generated_lv_cases()
    out_g, cig_g = _run_lv(lib, ref[:(l_ref + 7) // 8], l_ref, [c[0] for c in cases], [14] * len(cases), [c[1] for c in cases], 0)
    out_l, cig_l = _run_lv(lib, ref[:(l_ref + 7) // 8], l_ref, [c[0] for c in cases], [14] * len(cases), [c[1] for c in cases], 1)
    assert (out_g == out_l).all() and (cig_g == cig_l).all()
    met = set()
    for i, (p, read, k, dg) in enumerate(cases):
        L = len(read)
        T = [1 << int(x) for x in genome[p:p + L + 4]]
        e, d_fin, text = _lv_model(T, [1 << int(x) for x in read], 14)
        assert int(out_l[i, 1]) == e, ("distance", i, out_l[i], e, k, dg)
        assert e >= 0 and _cigar_text(cig_l[i], out_l[i, 3]) == text, ("cigar", i, _cigar_text(cig_l[i], out_l[i, 3]), text, e, d_fin)
        met.add((L, e, d_fin, p + L + 4 == l_ref))
    for L in (21, 100, 120, 129):
        for k in ((1,) if L == 21 else (1, 12, 13)):
            for d in (-k, 0, min(k, 4)):
                for at_end in (False, True):
                    assert (L, k, d, at_end) in met, ((L, k, d, at_end), sorted(m for m in met if m[0] == L and m[1] == k))


# ---- the chain ----
def _genome_codes(path):
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    with open(path) as f:
        return np.array([code.get(ch, 4) for line in f if not line.startswith(">") for ch in line.strip().upper()], dtype=np.uint8)


def _gapped_pairs(genome, n_pairs, seed):
    """n_pairs pairs, 400 bases apart, mate 1 from the forward strand and mate 2 from the reverse: three pairs of four with 100-base
    mates, the fourth with 150-base ones, every mate with an insertion or a deletion of 1 .. 3 bases near its middle, so that none
    has a gap-free hit within three mismatches."""
    rng = np.random.default_rng(seed)
    seqs, offs = [], [0]
    for i in range(n_pairs):
        L = 150 if i % 4 == 3 else 100
        start = int(rng.integers(100, len(genome) - 700))
        while (genome[start:start + 600] > 3).any():                     # not across an N
            start = int(rng.integers(100, len(genome) - 700))
        for mate in range(2):
            p = start if mate == 0 else start + 400 - L
            size = int(rng.integers(1, 4))
            at = int(rng.integers(L // 2 - 15, L // 2 + 15))
            src = genome[p:p + L + size + 8]
            if rng.random() < 0.5:
                ins = (src[at:at + size] + 1 + rng.integers(0, 3, size)) % 4
                r = np.concatenate([src[:at], ins.astype(np.uint8), src[at:]])[:L]
            else:
                r = np.concatenate([src[:at], src[at + size:]])[:L]
            if mate == 1:
                r = (3 - r[::-1])
            seqs.append(r.astype(np.uint8))
            offs.append(offs[-1] + L)
    return np.concatenate(seqs), np.array(offs, dtype=np.uint32)


@pytest.fixture(scope="module")
def chain():
    import salt_amd
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    genome = _genome_codes(os.path.join(LAMBDA, "genome.fa"))
    seqs, offs = _gapped_pairs(genome, 2048, seed=23)
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=4096, max_bases=int(offs[-1]) + 64)
    ora = oracle_py.Oracle(os.path.join(LAMBDA, "idx"))
    yield salt_amd, oracle_py, idx, aln, ora, seqs, offs
    ora.close()
    aln.close()
    idx.destroy()


def test_gpu_chain_on_a_batch_of_gapped_reads_equals_the_oracle(chain, tmp_path, monkeypatch):
    """4 096 reads that all take the gapped pass, 100 and 150 bases mixed, at k_cigar's own grid (a block an item) and on a second
    workspace with 256 k_cigar blocks (SALT_GPU_CIGAR_BLOCKS, read when a workspace is created): about 3 100 items, a dozen a block,
    all but the first through the queue head.  Every field against the oracle, the alternative hits' CIGARs through the SAM text; the
    two grids byte for byte the same rows."""
    salt_amd, oracle_py, idx, aln, ora, seqs, offs = chain
    opt, _ = salt_amd.AlnOpt.from_argv(["-d", "-c"], idx.l_seed)
    monkeypatch.setenv("SALT_GPU_CIGAR_BLOCKS", "256")
    aln_few = salt_amd.GpuAligner(idx, device=0, max_reads=4096, max_bases=int(offs[-1]) + 64)
    monkeypatch.delenv("SALT_GPU_CIGAR_BLOCKS")
    try:
        res_few = aln_few.alnse_core1(opt, seqs, offs).copy()
        assert aln_few.queue_counts()[7] > 2500                         # the queue head moved: the items behind the blocks' own went through it
    finally:
        aln_few.close()
    res = aln.alnse_core1(opt, seqs, offs)
    q = aln.queue_counts()
    for f in ("pos", "strand", "n_diff", "is_gap", "mapq", "n_cigar", "n_hits", "hit_n_cigar"):
        assert (res[f] == res_few[f]).all(), f
    for i in range(len(res)):
        assert (res["cigar"][i, :res["n_cigar"][i]] == res_few["cigar"][i, :res["n_cigar"][i]]).all(), i
        for h in range(int(res["n_hits"][i].sum())):
            assert (res["hit_cigar"][i, h, :res["hit_n_cigar"][i, h]] == res_few["hit_cigar"][i, h, :res["hit_n_cigar"][i, h]]).all(), (i, h)
    want = ora.align(ora.opt(), seqs, offs, n_threads=8)
    short = np.diff(offs.astype(np.int64)) == 100
    n_short_gapped = int(((want["is_gap"] == 1) & (want["pos"] != 0xFFFFFFFF) & short).sum())
    print("gapped reads %d of 4096, %d of them of 100 bases; k_gap slots asked %d, k_cigar items %d" % (
        int(((want["is_gap"] == 1) & (want["pos"] != 0xFFFFFFFF)).sum()), n_short_gapped, q[2], q[6]))
    assert int(((want["is_gap"] == 1) & (want["pos"] != 0xFFFFFFFF)).sum()) >= 4000   # what the batch is for: (nearly) every read is gapped
    assert n_short_gapped >= 2900                                     # (the oracle's rows: eleven items a block and more at 256 blocks)
    assert q[2] >= n_short_gapped and q[6] >= n_short_gapped, q         # each of them went through k_gap, k_gapfin and k_cigar
    bad = oracle_py.compare(res, want)
    assert len(bad) == 0, (len(bad), bad[:10])
    fq = str(tmp_path / "reads.fq")
    from salt_amd import workload
    workload.write_fastq(fq, seqs, offs)
    want_sam = subprocess.run([os.path.join(ROOT, "oracle", "salt_oracle"), "-d", "-c", os.path.join(LAMBDA, "idx"), fq], check=True, capture_output=True).stdout
    names, fseqs, foffs, quals = salt_amd.read_fastq(fq)
    got = salt_amd.sam_text(idx, opt, names, fseqs, foffs, quals, res)
    assert got == want_sam, gap_cases.diff_message(got, want_sam)


def test_gpu_chain_on_the_same_batch_as_pairs_equals_the_oracle(chain):
    """The same reads as 2 048 pairs (-p): k_gapfin at bound 3 for mates of both lengths, k_cigar behind k_pe_final.  Every field of
    both mates after pairing against the oracle."""
    salt_amd, oracle_py, idx, aln, ora, seqs, offs = chain
    opt, _ = salt_amd.AlnOpt.from_argv(["-p", "-c", "-a", "250", "-b", "550"], idx.l_seed)
    res = aln.alnpe_core1(opt, idx, seqs, offs)
    q = aln.queue_counts()
    oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
    want = ora.align_pe(oo, seqs, offs, opt.min_tlen, opt.max_tlen, n_threads=8)
    print("pairs: gapped mates %d of 4096, k_gap slots asked %d" % (int((want["is_gap"] == 1).sum()), q[2]))
    assert int(((want["is_gap"] == 1) & (want["pos"] != 0xFFFFFFFF)).sum()) >= 2048 and q[2] >= 2048, q     # the deferred pass ran for most mates
    bad = oracle_py.compare(res, want, pe=True)
    detail = [(int(i), [(f, res[f][i].tolist(), want[f][i].tolist()) for f in ("pos", "strand", "n_diff", "is_gap", "mapq", "b0", "b1", "seq_start", "seq_end")]) for i in bad[:4]]
    assert len(bad) == 0, (len(bad), detail)
