"""The parts of the light pass on a quarter of a wave (k_light4: four reads a wave, 16 lanes each), through the diagnostic kernels.

k_diag_rule mode 4 runs rule_sparse<3, false, 16> and k_diag_verify mode 7 runs verify_quads_2<4, 16>, four cases a wave, case
4b + q in quarter q of block b.  Neighbouring cases differ in length (and in the path they take), so the quarters of a wave do not run
in step, and a ballot, broadcast or LDS row that leaked from one quarter into another shows as a wrong value."""
import ctypes

import numpy as np
import pytest


def _sequential_rule(pos, val, bound, vmax, in_range):
    """The reference's candidate loop on the sorted, duplicate-free list (code_kmismatch, alnse.c:348-369, as alnse_check_nogap drives
    it): what the kernels must reproduce from the unsorted list."""
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


@pytest.mark.gpu
def test_gpu_quarter_rule_on_unsorted_lists_equals_the_sequential_rule():
    """The 3000 random lists of the half-wave test (test_gpu_parity, mode 3: the same generator and seed): lengths 0..300, few distinct
    loci or many, duplicates, loci at and beyond the reference end, every incoming bound."""
    import salt_amd
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_diag_rule.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    rng = np.random.Generator(np.random.PCG64(103))
    L, ref_len, vmax, n_cases = 100, 1000000, 3, 3000
    in_range = lambda p: p < ref_len
    pos, val, offs, bounds = [], [], [0], []
    for c in range(n_cases):
        n = int(rng.choice([0, 1, 2, 5, 17, 63, 64, 65, 128, 300]))
        n_distinct = int(rng.choice([1, 2, 3, 8, 1000]))
        lo = ref_len - 200 if rng.random() < 0.2 else 0                   # some lists straddle the reference end
        universe = rng.integers(lo, ref_len + 150 if lo else ref_len - 200, size=max(n_distinct, 1), dtype=np.int64)
        p = universe[rng.integers(0, len(universe), size=n)]
        dist_of = {int(u): int(rng.choice([0, 1, 2, 3, 4, 7, 12, 200], p=[.1, .15, .15, .15, .1, .05, .05, .25])) for u in universe}
        v = np.array([dist_of[int(x)] for x in p], dtype=np.uint8)
        v[v > vmax] = 255
        pos.append(p.astype(np.uint32)); val.append(v); offs.append(offs[-1] + n)
        bounds.append(int(rng.integers(0, vmax + 1)) if rng.random() < 0.5 else vmax)
    pos_a, val_a = np.concatenate(pos), np.concatenate(val)
    offs_a, b_a = np.array(offs, dtype=np.uint32), np.array(bounds, dtype=np.uint32)
    out = np.zeros((n_cases, 18), dtype=np.uint32)
    rc = lib.salt_gpu_diag_rule(n_cases, pos_a.ctypes.data, val_a.ctypes.data, offs_a.ctypes.data, b_a.ctypes.data, L, ref_len, 4, out.ctypes.data)
    assert rc == 0, lib.salt_gpu_last_error()
    for c in range(n_cases):
        found, bp, bv, hits, a0, bound = _sequential_rule([int(x) for x in pos[c]], [int(x) for x in val[c]], bounds[c], vmax, in_range)
        got = [int(x) for x in out[c]]
        want = [found, bp if found else 0, bv if found else 0, len(hits), a0 if hits else 0, bound]
        for h in range(6):
            want += list(hits[h]) if h < len(hits) else [0, 0]
        assert got == want, (c, got, want, pos[c][:10], val[c][:10], bounds[c])


@pytest.mark.gpu
def test_gpu_quarter_verify_equals_the_host_hamming_count():
    """verify_quads_2<4, 16> against the masked Hamming count of the host (0..3, or 255 above 3), on a mixRef of 8000 positions with
    SNP masks.  Every case holds windows at each word alignment 0..7 (position mod 8), the window at the genome's start, the one that
    ends with the genome's last base, wild values at and beyond the end (255, never used as an address), and the read's own origin
    and its neighbour.  Up to 28 rows a case: two trips of 16 rows, split between the "strands".  Lengths 8 .. 120."""
    from salt_amd import api
    lib = api.gpu_lib()
    rng = np.random.default_rng(18)
    ref_len = 8000
    masks = (1 << rng.integers(0, 4, size=ref_len)).astype(np.uint32)
    snp = rng.random(ref_len) < 0.05
    masks[snp] |= (1 << rng.integers(0, 4, size=int(snp.sum()))).astype(np.uint32)
    words = np.zeros((ref_len + 7) // 8, dtype=np.uint32)
    for q in range(8):
        m = masks[q::8]
        words[:len(m)] |= m << np.uint32(4 * q)
    reads, cands, coffs, want = [], [], [0], []
    for t, L in enumerate([100, 120, 37, 8, 64, 101, 119, 21, 96] * 4):
        # the read: a cut at alignment t % 8, or one that touches an end of the genome
        p = (0, ref_len - L)[t % 2] if t % 9 == 4 else int(rng.integers(1, (ref_len - L) // 8)) * 8 + t % 8
        r = np.array([int(np.log2(int(m) & -int(m))) for m in masks[p:p + L]], dtype=np.uint8)
        e = rng.random(L) < 0.02
        r[e] = (r[e] + 1) & 3
        aligned = [p - p % 8 + a for a in range(8) if p - p % 8 + a + L <= ref_len]            # the origin's word, every alignment
        ends = [0, ref_len - L]
        wild = [0xFFFFFFF0, 0xFFFFFFFF, 0x80000000, ref_len, ref_len + 5]
        far = [int(x) for x in rng.integers(0, ref_len - L, size=int(rng.integers(2, 12)))]
        c = [int(x) for x in rng.permutation(np.array([p, max(0, p - 1)] + aligned + ends + wild + far, dtype=np.uint64))]
        assert {x % 8 for x in c if x < ref_len} == set(range(8)) or len(aligned) < 8
        for x in c:
            if x >= ref_len:
                want.append(255)
            else:
                assert x + L <= ref_len
                mm = sum(1 for i in range(L) if not (int(masks[x + i]) >> int(r[i])) & 1)
                want.append(mm if mm <= 3 else 255)
        reads.append(r); cands += c; coffs.append(len(cands))
    assert any(0 in cands[coffs[i]:coffs[i + 1]] for i in range(len(reads))) and min(want) == 0
    offs = np.zeros(len(reads) + 1, dtype=np.uint32); offs[1:] = np.cumsum([len(r) for r in reads])
    seqs = np.concatenate(reads)
    cand = np.array(cands, dtype=np.uint32); co = np.array(coffs, dtype=np.uint32)
    out = np.zeros(len(cand), dtype=np.uint8)
    rc = lib.salt_gpu_diag_verify(words.ctypes.data, ref_len, len(reads), seqs.ctypes.data, offs.ctypes.data, cand.ctypes.data, co.ctypes.data,
                                  7, out.ctypes.data)
    assert rc == 0, lib.salt_gpu_last_error()
    want = np.array(want, dtype=np.uint8)
    assert np.array_equal(out, want), np.nonzero(out != want)[0][:10]
