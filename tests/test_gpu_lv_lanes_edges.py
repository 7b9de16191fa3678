"""The one-candidate-per-lane Landau-Vishkin kernel (lane_text + lane_pattern + lv_lanes) at the edges of its staging: the zero words
behind the text window and the pattern, the word-major text, the word pair that the equality gate and the extension share, and the
previous row carried in registers.

The cases are generated here from a fixed seed and the expected distances come from the oracle's so_ed_diff, which
test_oracle_golden.py pins to the reference's vectors.  salt_gpu_diag_lv runs 64 cases of one (L, k) in one wave, a lane each with its
own read, so every group below is 64 lanes that mix: the eight values of pos & 7, pos = 0, windows ending at the reference's end
-1 / 0 / +1, exact copies (done at level 0 beside lanes that run to k), 1..k substitutions, insertions and deletions of 1..k bases inside
the first and the last 8 bases and at both sides of an 8-base word boundary, indels at read position 0, reads with N, and random reads
that run the full depth.  About 3 % of the reference's sites carry two or three alleles: there the equality gate (nibbles equal) and
the match (mask AND one-hot != 0) disagree, as they do in the reference.

What the kernel stages, restated from salt_align.hip (LLV_TS, LLV_PW): with bound k <= LLV_K and a window of L + 4 nibbles the loops
ask for text nibbles 0 .. L + LLV_K and pattern nibbles 0 .. L, eight at a time from any start, i.e. for text words
0 .. (L + LLV_K) // 8 + 1 and pattern words 0 .. L // 8 + 1; staged_words() below is that arithmetic and the census holds it against
the 24 and 22 words a lane has."""
import collections
import ctypes

import numpy as np
import pytest

import gap_cases

SEED = 20240613
L_REF = 4096
LENGTHS = (40, 41, 47, 48, 49, 96, 100, 104, 129, 160, 163, 164)
GROUPS_PER_SHAPE = 3                    # 64-lane groups per (L, k)
BEYOND = (165, 12)                      # L + 4 = 169 > 168: the lane kernel must answer -2
LLV_TS, LLV_PW = 24, 22                 # salt_align.hip: text / pattern words staged per lane

Case = collections.namedtuple("Case", "L k pos seq kind")


def staged_words(L, k_max=gap_cases.LLV_K):
    """(text words, pattern words) the lane kernel can index for a read of L bases: see the module docstring"""
    return (L + k_max) // 8 + 2, L // 8 + 2


def shapes():
    out = []
    for L in LENGTHS:
        for k in sorted({L // 10, 12}):
            if gap_cases.lanes_fit(L, k):
                out.append((L, k))
    return out


def make_reference(rng):
    """L_REF nibble masks: one base per site, about 3 % of the sites with two or three alleles"""
    base = rng.integers(0, 4, L_REF)
    mask = (1 << base).astype(np.uint8)
    multi = rng.random(L_REF) < 0.03
    for p in np.nonzero(multi)[0]:
        for _ in range(int(rng.integers(1, 3))):
            mask[p] |= 1 << int(rng.integers(0, 4))
    words = np.zeros(L_REF // 8, dtype=np.uint32)
    for q in range(8):
        words |= mask[q::8].astype(np.uint32) << np.uint32(4 * q)
    return mask, words


def copy_of(mask, rng, start, n):
    """n read bases that match the reference from `start`: at a site with several alleles any one of them"""
    out = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        m = int(mask[start + i])
        alleles = [b for b in range(4) if m >> b & 1]
        out[i] = alleles[int(rng.integers(0, len(alleles)))]
    return out


def substitute(mask, rng, seq, start, at):
    """seq with the base at `at` replaced by one the reference site does not carry (a site with all four alleles keeps its base)"""
    m = int(mask[start + at]) if start + at < L_REF else 0
    wrong = [b for b in range(4) if not m >> b & 1]
    if wrong:
        seq[at] = wrong[int(rng.integers(0, len(wrong)))]


def make_case(mask, rng, L, k, lane, g):
    """lane `lane` of group g of shape (L, k)"""
    room = L_REF - (L + 4) - 2 * gap_cases.LLV_K - 8
    pos = (int(rng.integers(8, room)) & ~7) | (lane & 7)                   # all eight values of pos & 7 in every group
    size = 1 + (lane + g) % k                                              # 1 .. k over the lanes and groups
    kind = lane % 32 if lane < 48 else 31                                  # lanes 48..63: random reads
    tag = "copy"

    def indel(at, size, insert):
        src = copy_of(mask, rng, pos, L + size + 8)
        if insert:
            return np.concatenate([src[:at], rng.integers(0, 4, size).astype(np.uint8), src[at:]])[:L]
        return np.concatenate([src[:at], src[at + size:]])[:L]

    if kind == 0:                                                          # exact copy: done at level 0
        seq = copy_of(mask, rng, pos, L)
    elif kind == 1:
        pos, tag = 0, "pos0"
        seq = copy_of(mask, rng, pos, L)
        if g:
            substitute(mask, rng, seq, pos, int(rng.integers(0, L)))
    elif kind in (2, 3, 4):                                                # the window ends at the reference's end -1 / 0 / +1
        d = kind - 3
        pos, tag = L_REF + d - (L + 4), "end%+d" % d
        seq = copy_of(mask, rng, pos, L)
        if g == 1:
            substitute(mask, rng, seq, pos, int(rng.integers(0, L)))
        if g == 2:                                                         # a deletion that pushes the read's tail towards the end
            src = copy_of(mask, rng, pos, L + 3)
            seq = np.concatenate([src[:L // 2], src[L // 2 + 3:]])[:L]
    elif kind in (5, 6, 7):                                                # 1 .. k substitutions
        tag = "subst"
        seq = copy_of(mask, rng, pos, L)
        for at in rng.choice(L, size=size, replace=False):
            substitute(mask, rng, seq, pos, int(at))
    elif kind in (8, 9, 10, 11):                                           # indel inside the first 8 bases
        tag = "lead_ins" if kind & 1 else "lead_del"
        seq = indel(int(rng.integers(1, 8)), size, kind & 1)
    elif kind in (12, 13, 14, 15):                                         # indel inside the last 8 bases
        tag = "trail_ins" if kind & 1 else "trail_del"
        seq = indel(L - 1 - int(rng.integers(0, 7)), size, kind & 1)
    elif kind in (16, 17, 18, 19, 20, 21):                                 # indel at each side of a word boundary of the read
        tag = "word_ins" if kind & 1 else "word_del"
        word = 1 + int(rng.integers(0, max(1, L // 8 - 1)))
        seq = indel(8 * word + (-1, 0, 1)[(kind - 16) // 2], size, kind & 1)
    elif kind in (22, 23):                                                 # ... and of the text window (pos & 7 decides where that is)
        tag = "tword_ins" if kind & 1 else "tword_del"
        at = 8 * (1 + int(rng.integers(0, max(1, L // 8 - 2)))) - (pos & 7) + int(rng.integers(-1, 2))
        seq = indel(min(max(at, 1), L - 1), size, kind & 1)
    elif kind in (24, 25, 26):                                             # indel at read position 0: the outermost diagonals
        tag = "lead_ins" if kind == 25 else "lead_del"
        seq = indel(0, size, kind == 25)
        if kind == 26:                                                     # the read starts before the window: its first bases have no text
            pos = max(pos - size, 0)
            seq = np.concatenate([rng.integers(0, 4, size).astype(np.uint8), copy_of(mask, rng, pos, L)])[:L]
            tag = "lead_ins"
    elif kind in (27, 28, 29):                                             # one to three N
        tag = "N"
        seq = copy_of(mask, rng, pos, L)
        seq[rng.choice(L, size=kind - 26, replace=False)] = 4
        if g == 2:
            seq = np.concatenate([seq[:9], seq[10:], copy_of(mask, rng, pos + L, 1)])
    elif kind == 30:                                                       # a mix: substitutions around one short indel
        tag = "mixed"
        seq = indel(L // 2, 1 + (lane + g) % 2, g & 1)
        for at in rng.choice(L // 2 - 1, size=min(k - 2, 2), replace=False):
            substitute(mask, rng, seq, pos, int(at))
    else:                                                                  # random: full depth, -1
        tag = "random"
        seq = rng.integers(0, 4, L).astype(np.uint8)
    if kind in (1, 2, 3, 4) and lane >= 32:                                # the second lane of these kinds: the same window, an N and substitutions
        for at in rng.choice(L, size=size - 1, replace=False):
            substitute(mask, rng, seq, pos, int(at))
        seq[5] = 4
    assert len(seq) == L
    return Case(L, k, pos, np.ascontiguousarray(seq, dtype=np.uint8), tag)


def generate():
    rng = np.random.default_rng(SEED)
    mask, words = make_reference(rng)
    cases = []
    for L, k in shapes() + [BEYOND]:
        for g in range(GROUPS_PER_SHAPE if (L, k) != BEYOND else 1):
            cases.extend(make_case(mask, rng, L, k, lane, g) for lane in range(64))
    return mask, words, cases


@pytest.fixture(scope="module")
def edge_cases(oracle_lib):
    """(reference words, cases, the oracle's distances): computed once for both tests"""
    mask, words, cases = generate()
    refp = np.concatenate([words, np.zeros(8, dtype=np.uint32)])
    rp = refp.ctypes.data_as(ctypes.c_void_p)
    want = [oracle_lib.so_ed_diff(rp, L_REF, c.pos, c.L + 4, c.seq.ctypes.data_as(ctypes.c_void_p), c.L, c.k) for c in cases]
    return mask, words, cases, want


def test_edge_cases_census(edge_cases):
    """What the generator is for, from the oracle's answers alone."""
    mask, words, cases, want = edge_cases
    n = len(cases)
    assert 3000 <= n <= 5000
    n_multi = int(sum(bin(int(m)).count("1") > 1 for m in mask))
    assert 0.02 * L_REF <= n_multi <= 0.04 * L_REF, n_multi
    assert set(shapes()) == {(c.L, c.k) for c in cases if (c.L, c.k) != BEYOND}
    assert {L for L, _ in shapes()} == set(LENGTHS) and all(k in (L // 10, 12) for L, k in shapes())
    assert sum(w >= 0 for w in want) >= 0.35 * n, sum(w >= 0 for w in want)
    assert sum(w == -1 for w in want) >= 0.20 * n, sum(w == -1 for w in want)
    assert sum(c.kind.startswith(("lead_", "trail_")) for c in cases) >= 200
    for (L, k) in shapes() + [BEYOND]:
        mine = [(c, w) for c, w in zip(cases, want) if (c.L, c.k) == (L, k)]
        assert len(mine) % 64 == 0
        for b in range(0, len(mine), 64):
            grp = mine[b:b + 64]
            assert len({(c.pos, c.seq.tobytes()) for c, _ in grp}) == 64, (L, k, b)
            assert {c.pos & 7 for c, _ in grp} == set(range(8))
            assert any(c.pos == 0 for c, _ in grp) and {c.pos + L + 4 - L_REF for c, _ in grp} >= {-1, 0, 1}
            assert all(w == -1 for c, w in grp if c.pos + L + 4 == L_REF + 1)              # + 1 is no candidate
            assert any(w == 0 for _, w in grp) and any(w == -1 for _, w in grp)           # level 0 beside the full depth
            assert any((c.seq == 4).any() for c, _ in grp)
        # every distance 1 .. k is reached somewhere in the shape's groups up to the bound that indels of 1 .. k bases allow
        assert {w for _, w in mine if w > 0} >= set(range(1, min(k, 4) + 1)), (L, k)
    # the staging covers what the loops can index (salt_align.hip: LLV_TS, LLV_PW), at the same limits as lanes_fit
    for L in range(1, 200):
        fits = gap_cases.lanes_fit(L, gap_cases.LLV_K)
        assert fits == (L <= 164)
        if fits:
            tw, pw = staged_words(L)
            assert tw <= LLV_TS and pw <= LLV_PW, L
    assert staged_words(164) == (LLV_TS, LLV_PW)
    # gate and match disagree at sites with several alleles: some read base there is one allele of two
    assert sum(bin(int(mask[c.pos + i])).count("1") > 1 for c in cases[:640] if c.kind == "copy" for i in range(c.L)) >= 10


@pytest.mark.gpu
def test_lv_lanes_edges_on_the_gpu(edge_cases):
    """out[.][2] (lane_text + lv_lanes) equals the oracle's distance for every case within the lane kernel's limits and is -2 beyond
    them; out[.][1] (lv_unpack + lv_wave) equals it for every case."""
    import salt_amd
    _, words, cases, want = edge_cases
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_diag_lv.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 6
    n = len(cases)
    pos_a = np.array([c.pos for c in cases], dtype=np.uint32)
    kd_a = np.array([c.k for c in cases], dtype=np.uint32)
    seq_a = np.concatenate([c.seq for c in cases]).astype(np.uint8)
    off_a = np.concatenate([[0], np.cumsum([c.L for c in cases])]).astype(np.uint32)
    out = np.zeros((n, 4), dtype=np.int32)
    cig = np.zeros((n, gap_cases.MAX_CIGAR_OPS), dtype=np.uint16)
    ref = np.ascontiguousarray(words)
    rc = lib.salt_gpu_diag_lv(ref.ctypes.data, L_REF, n, pos_a.ctypes.data, kd_a.ctypes.data, seq_a.ctypes.data, off_a.ctypes.data,
                              out.ctypes.data, cig.ctypes.data)
    assert rc == 0, lib.salt_gpu_last_error()
    want_a = np.array(want, dtype=np.int32)
    fit = np.array([gap_cases.lanes_fit(c.L, c.k) for c in cases])
    assert fit.sum() == n - 64
    bad_wave = np.nonzero(out[:, 1] != want_a)[0]
    assert len(bad_wave) == 0, [("lv_wave", int(i), out[i].tolist(), int(want_a[i]), cases[i]) for i in bad_wave[:5]]
    bad = np.nonzero(fit & (out[:, 2] != want_a))[0]
    assert len(bad) == 0, (len(bad), [("lv_lanes", int(i), i % 64, out[i].tolist(), int(want_a[i]), cases[i]) for i in bad[:5]])
    assert (out[~fit, 2] == -2).all()
