"""A plain model of the device index image (salt_amd/csrc/salt_device.h), in numpy, for tests/test_index_image_model.py (CPU) and
tests/test_gpu_index_image.py (GPU).

Every array of the image -- COcc, ROcc, c_sa, r_pos, lkt, ref, text, wlkt, c_ctx -- and r_ctx beside it is computed here from the index
files alone: .C.pac, .C.bwt (header only: primary and L2), .C.sa (header only), .R.backward.{bwt,occ,sa},
.ref and .R.seedLen.  The definitions are the textbook ones -- a sorted suffix array, BWT = T[SA - 1], Occ = a plain cumulative
count -- and not the kernels': nothing here reads salt_amd/csrc or tools/ctx_model.cc, the record geometry (9 bases in front, 37
behind from 2 k on, 2 + 2 bits of special-site counts) is restated from the comment of salt_ctx_record.h.

edge_cases() builds the small generated indexes whose lengths sit on the block and word boundaries no committed index has.
"""
import os

import numpy as np

NONE = 0xFFFFFFFF
LKT_LEN = 12
CTX_N_B, CTX_N_A, CTX_A_SEEDS = 9, 37, 2          # salt_ctx_record.h: side B in front of the suffix, side A behind it from 2 k on
CTX_SAT = 3                                        # 2 + 2 bits: a count of 3 means "3 or more, or the side is not whole"


def _u32(path, offset=0, count=-1):
    return np.fromfile(path, dtype="<u4", offset=offset, count=count)


def suffix_array(sym):
    """Suffix array of sym + a terminator smaller than every symbol, the terminator's (empty) suffix first: prefix doubling."""
    n = len(sym) + 1
    rank = np.concatenate([np.asarray(sym, dtype=np.int64) + 1, [0]])
    k = 1
    while True:
        r2 = np.zeros(n, dtype=np.int64)
        r2[:n - k] = rank[k:]
        order = np.lexsort((r2, rank))
        key = rank[order] * (n + 1) + r2[order]
        new = np.concatenate([[0], np.cumsum(key[1:] != key[:-1])])
        rank = np.empty(n, dtype=np.int64)
        rank[order] = new
        if new[-1] == n - 1:
            return order.astype(np.int64)
        k *= 2


def _planes64(bits):
    """bits: 0/1 array whose length is a multiple of 64 -> uint64 words, element i of a word in bit i."""
    b = np.asarray(bits, dtype=np.uint8).reshape(-1, 8)
    return np.packbits(b, axis=1, bitorder="little").reshape(-1).view("<u8")


class Model:
    """The image of one index prefix.  Arrays are built on first use and kept."""

    def __init__(self, prefix, l_seed=None):
        self.prefix = prefix
        p = prefix
        self.l_seed = int(np.fromfile(p + ".R.seedLen", dtype="<i4", count=1)[0]) if l_seed is None else l_seed
        h = _u32(p + ".C.bwt", count=5)
        self.c_primary = int(h[0])
        self.c_L2 = np.concatenate([[0], h[1:5]]).astype(np.int64)
        self.c_seq_len = n = int(h[4])
        hs = _u32(p + ".C.sa", count=7)
        self.c_sa_intv = int(hs[5])
        self.c_sa_file = _u32(p + ".C.sa", offset=28)
        pac = np.fromfile(p + ".C.pac", dtype=np.uint8)
        self.T = ((pac[np.arange(n) >> 2] >> ((~np.arange(n) & 3) << 1)) & 3).astype(np.uint8)
        # ---- C ----
        self.SA = suffix_array(self.T)                               # row 0: the empty suffix, SA[0] = n
        self.c_sa = self.SA.astype(np.uint32)
        self.c_sa[0] = NONE
        self.primary = int(np.nonzero(self.SA == 0)[0][0])
        bwt = self.T[(self.SA - 1) % max(n, 1)] if n else np.zeros(1, np.uint8)
        self.B = np.delete(bwt, self.primary)                        # the '$'-removed BWT, n symbols
        self.c_cum = np.zeros((4, n + 1), dtype=np.int64)           # c_cum[c][i] = occurrences of c in B[0:i]
        for c in range(4):
            self.c_cum[c, 1:] = np.cumsum(self.B == c)
        # padded 12-mer keys of every suffix, the empty one included
        tp = np.concatenate([self.T, np.zeros(LKT_LEN, np.uint8)]).astype(np.int64)
        key = np.zeros(n + 1, dtype=np.int64)
        for j in range(LKT_LEN):
            key = (key << 2) | tp[j:j + n + 1]
        self.key12 = key
        # ---- R ----
        hr = _u32(p + ".R.backward.bwt", count=8)
        self.r_text_len = m = int(hr[0])
        self.r_inv_sa0 = int(hr[1])
        self.r_cum = np.concatenate([[0], hr[2:7]]).astype(np.int64)
        self.r_bwt_words = int(hr[7])
        words = _u32(p + ".R.backward.bwt", offset=32, count=self.r_bwt_words)
        i = np.arange(m)
        self.RB = ((words[i >> 3] >> ((7 - (i & 7)) * 4)) & 15).astype(np.uint8)      # stored R BWT symbols ('$' not stored)
        self.r_occ_cum = np.zeros((5, m + 1), dtype=np.int64)
        for c in range(5):
            self.r_occ_cum[c, 1:] = np.cumsum(self.RB == c)
        occ = _u32(p + ".R.backward.occ")
        self.r_minor = occ[1:1 + int(occ[0])]
        self.r_major = occ[2 + int(occ[0]):2 + int(occ[0]) + int(occ[1 + int(occ[0])])]
        rsa = _u32(p + ".R.backward.sa")
        self.r_sa = rsa[1:1 + int(rsa[0])]
        rf = _u32(p + ".ref")
        self.ref_len = int(rf[0])
        self.ref_words = rf[1:1 + (self.ref_len + 7) // 8]
        j = np.arange(self.ref_len)
        self.mask = ((self.ref_words[j >> 3] >> (4 * (j & 7))) & 15).astype(np.uint8)
        self._memo = {}

    # ---- rank queries, from the plain cumulative counts ----
    def c_occ(self, k, c):
        """Occ(k, c) of the C index: occurrences of c in BWT rows [0, k], the '$' row not counted; k = c_seq_len: all, 0xFFFFFFFF: 0."""
        k = np.asarray(k, dtype=np.int64)
        c = np.asarray(c, dtype=np.int64)
        kk = np.clip(k - (k >= self.c_primary), 0, max(self.c_seq_len - 1, 0))
        v = self.c_cum[c, kk + 1]
        v = np.where(k == self.c_seq_len, self.c_L2[c + 1] - self.c_L2[c], v)
        return np.where(k == NONE, 0, v)

    def c_row_sym(self, k):
        """BWT symbol of row k; 4 for the '$' row and for 0xFFFFFFFF."""
        k = np.asarray(k, dtype=np.int64)
        ok = (k != NONE) & (k != self.c_primary)
        kk = np.clip(k - (k > self.c_primary), 0, self.c_seq_len - 1)
        return np.where(ok, self.B[kk], 4)

    def r_occ(self, index, c):
        """Occ(index, c) of the R index: occurrences of c in the rows [0, index), the '$' row not counted."""
        index = np.asarray(index, dtype=np.int64)
        return self.r_occ_cum[np.asarray(c, dtype=np.int64), index - (index > self.r_inv_sa0)]

    def r_row_sym(self, row):
        """BWT symbol of R row `row` in [0, r_text_len]; the '$' row reads as '#' (4)."""
        row = np.asarray(row, dtype=np.int64)
        st = np.clip(row - (row > self.r_inv_sa0), 0, self.r_text_len - 1)
        return np.where(row == self.r_inv_sa0, 4, self.RB[st])

    # ---- the arrays ----
    def c_occ_words(self):
        """COcc as uint32 words, 8 per block: 4 counts in front of the block's 64 symbols, low plane, high plane."""
        n = self.c_seq_len
        nb = n // 64 + 1
        sym = np.zeros(nb * 64, dtype=np.uint8)
        sym[:n] = self.B
        out = np.zeros((nb, 8), dtype="<u4")
        for c in range(4):
            out[:, c] = self.c_cum[c, np.minimum(np.arange(nb) * 64, n)]
        out[:, 4:6] = _planes64(sym & 1).view("<u4").reshape(nb, 2)
        out[:, 6:8] = _planes64(sym >> 1).view("<u4").reshape(nb, 2)
        return out.reshape(-1)

    def r_occ_words(self):
        """ROcc as uint32 words, 16 per block: counts of A C G T in front of the block's 128 symbols, three bit planes of two words."""
        m = self.r_text_len
        nb = m // 128 + 1
        sym = np.zeros(nb * 128, dtype=np.uint8)
        sym[:m] = self.RB
        out = np.zeros((nb, 16), dtype="<u4")
        for c in range(4):
            out[:, c] = self.r_occ_cum[c, np.minimum(np.arange(nb) * 128, m)]
        for b in range(3):
            out[:, 4 + 4 * b:8 + 4 * b] = _planes64((sym >> b) & 1).view("<u4").reshape(nb, 4)
        return out.reshape(-1)

    def lkt(self):
        """item[x] = the first row whose A-padded suffix is >= x, x in [0, 4^12]."""
        if "lkt" not in self._memo:
            cnt = np.bincount(self.key12, minlength=1 << (2 * LKT_LEN))
            self._memo["lkt"] = np.concatenate([[0], np.cumsum(cnt)]).astype("<u4")
        return self._memo["lkt"]

    def text_words(self):
        n = self.c_seq_len
        nw = n // 16 + 4
        t = np.zeros(nw * 16, dtype=np.uint64)
        t[:n] = self.T
        sh = (30 - 2 * (np.arange(nw * 16) & 15)).astype(np.uint64)
        return (t << sh).reshape(nw, 16).sum(axis=1).astype("<u4")

    def ref_image_words(self):
        return np.concatenate([self.ref_words, np.zeros(4, dtype="<u4")]).astype("<u4")

    def r_pos(self):
        """The value of Rbwt_back_bwt_sa (rbwt.c:316-333) for every R row: LF steps until the row is a '#' row (row > cum[4]), then
        the '#' table's entry + steps - 1."""
        if "r_pos" in self._memo:
            return self._memo["r_pos"]
        m, n_acgt = self.r_text_len, int(self.r_cum[4])
        row = np.arange(m + 1, dtype=np.int64)
        step = np.zeros(m + 1, dtype=np.int64)
        for _ in range(1 << 20):
            act = np.nonzero(row <= n_acgt)[0]
            if len(act) == 0:
                break
            c = self.r_row_sym(row[act])
            row[act] = self.r_cum[c] + self.r_occ(row[act], c) + 1
            step[act] += 1
        assert (row > n_acgt).all(), "an LF walk that never reaches a '#' row"
        out = ((self.r_sa[row - n_acgt - 1].astype(np.int64) + step - 1) & 0xFFFFFFFF).astype("<u4")
        self._memo["r_pos"] = out
        return out

    def r_text(self):
        """(text, row_of) of the R index, recovered by inverting the stored BWT with this model's own Occ: text[t] for t in
        [0, r_text_len) (codes 0..4), and row_of[t] = the row whose suffix starts at t, t in [0, r_text_len] (the last one is '$')."""
        if "r_text" in self._memo:
            return self._memo["r_text"]
        m = self.r_text_len
        rows = np.arange(m + 1)
        c = self.r_row_sym(rows)
        lf = self.r_cum[c] + self.r_occ(rows, c) + 1
        lf[self.r_inv_sa0] = 0                                   # that row's symbol is '$': the suffix before the whole text is the last one
        lf = lf.tolist()
        row_of = np.empty(m + 1, dtype=np.int64)
        row = 0                                                  # row 0: the suffix "$"
        for t in range(m, -1, -1):
            row_of[t] = row
            row = lf[row]
        assert row == 0 and len(np.unique(row_of)) == m + 1, "the stored R BWT is not the BWT of one text"
        self._memo["r_text"] = (c[row_of[1:]].astype(np.uint8), row_of)
        return self._memo["r_text"]

    def ctx_records(self, first, s_none):
        """One record (4 uint32) per entry of `first` (a table of suffix starts; 0xFFFFFFFF stands at s_none), for seed length l_seed."""
        first = np.asarray(first, dtype=np.int64)
        s = np.where(first == NONE, s_none, first)
        ln = min(self.c_seq_len, self.ref_len)
        a_start = CTX_A_SEEDS * self.l_seed
        T = np.concatenate([self.T[:ln].astype(np.int64), [0]])
        special = np.concatenate([self.mask[:ln].astype(np.int64) != (1 << self.T[:ln].astype(np.int64)), [False]])
        lo = np.zeros(len(s), dtype=np.uint64)
        hi = np.zeros(len(s), dtype=np.uint64)
        ns = []
        for side, n_side in ((0, CTX_N_A), (1, CTX_N_B)):
            whole = (s + a_start + CTX_N_A <= ln) if side == 0 else ((s >= CTX_N_B) & (s <= ln))
            cnt = np.zeros(len(s), dtype=np.int64)
            for t in range(n_side):
                p = np.where(whole, s + a_start + t if side == 0 else s - 1 - t, ln)      # ln: the zero entry appended above
                bit = np.uint64(t if side == 0 else CTX_N_A + t)
                lo |= (T[p] & 1).astype(np.uint64) << bit
                hi |= (T[p] >> 1).astype(np.uint64) << bit
                cnt += special[p]
            ns.append(np.where(whole, np.minimum(cnt, CTX_SAT), CTX_SAT).astype(np.uint64))
        out = np.zeros((len(s), 4), dtype="<u4")
        m32 = np.uint64(0xFFFFFFFF)
        out[:, 0] = first & 0xFFFFFFFF
        out[:, 1] = lo & m32
        out[:, 2] = ((lo >> np.uint64(32)) | (hi << np.uint64(14))) & m32
        out[:, 3] = ((hi >> np.uint64(18)) | (ns[0] << np.uint64(28)) | (ns[1] << np.uint64(30))) & m32
        return out

    def c_ctx(self):
        return self.ctx_records(self.c_sa, self.c_seq_len)          # row 0, the empty suffix, stands at c_seq_len

    def r_ctx(self):
        return self.ctx_records(self.r_pos(), NONE)                  # a row without a position stands beyond the genome

    def wlkt(self, W):
        """The non-empty entries of the W-mer table: (x, rows) with x ascending and rows[i] the 8 uint32 of entry x[i]; every other
        entry is ((1, 0, 1, 0), (0, 0, 0, 0))."""
        n = self.c_seq_len
        # C: the rows whose padded suffix starts with the last 12 bases, then W - 12 exact backward steps
        x, start = np.unique(self.key12[self.SA], return_index=True)
        assert (np.diff(self.key12[self.SA]) >= 0).all(), "padded 12-mer keys are not monotone along the suffix array"
        k = start.astype(np.int64)
        l = np.concatenate([start[1:], [n + 1]]).astype(np.int64) - 1
        for t in range(W - LKT_LEN):
            c = np.repeat(np.arange(4, dtype=np.int64), len(x))
            x4, k4, l4 = np.tile(x, 4), np.tile(k, 4), np.tile(l, 4)
            nk = self.c_L2[c] + self.c_occ(np.where(k4 == 0, NONE, k4 - 1), c) + 1
            nl = self.c_L2[c] + self.c_occ(l4, c)
            keep = nk <= nl
            x, k, l = (x4 | (c << (2 * (LKT_LEN + t))))[keep], nk[keep], nl[keep]
        cx, ck, cl = x, k, l
        # R: W steps of the exact backward search from (0, r_text_len), the last base first
        x, k, l = np.zeros(1, np.int64), np.zeros(1, np.int64), np.full(1, self.r_text_len, np.int64)
        for t in range(W):
            c = np.repeat(np.arange(4, dtype=np.int64), len(x))
            x4, k4, l4 = np.tile(x, 4), np.tile(k, 4), np.tile(l, 4)
            nk = self.r_cum[c] + self.r_occ(k4, c) + 1
            nl = self.r_cum[c] + self.r_occ(l4 + 1, c)
            keep = nk <= nl
            x, k, l = (x4 | (c << (2 * t)))[keep], nk[keep], nl[keep]
        rx, rk, rl = x, k, l
        allx = np.union1d(cx, rx)
        rows = np.zeros((len(allx), 8), dtype=np.int64)
        rows[:, 0] = rows[:, 2] = 1
        ci, ri = np.searchsorted(allx, cx), np.searchsorted(allx, rx)
        rows[ci, 0], rows[ci, 1] = ck, cl
        rows[ri, 2], rows[ri, 3] = rk, rl
        # second half: for a C interval of one or two rows, per row the suffix's position and the 16 bases in front of it (the one
        # right in front in the lowest bits; fewer near the genome's start); three rows or more: zero
        for q in range(2):
            sel = (cl - ck <= 1) & (cl - ck >= q)
            p0 = self.SA[ck[sel] + q]
            prev = np.zeros(len(p0), dtype=np.int64)
            for j in range(1, 17):
                ok = p0 >= j
                prev |= np.where(ok, self.T[np.where(ok, p0 - j, 0)].astype(np.int64), 0) << (2 * (j - 1))
            rows[ci[sel], 4 + 2 * q], rows[ci[sel], 5 + 2 * q] = p0, prev
        return allx, rows.astype("<u4")


# ---- generated edge cases ----
# name -> (generator seed, genome length, what the case is in the table for beside the repeats and special sites every case has).  Found by a random search over seeds and lengths on the
# CPU: each candidate was built with the host suffix sorter and its properties read off this model (edge_properties); the table is the
# record and tests/test_index_image_model.py asserts that every case still has what it is listed for.
# Not reachable: a .ref whose length differs from c_seq_len -- the builder writes both from the same packed genome.
EDGE_CASES = {
    "s219": (219, 1344, ['c_len%128=64', 'c_primary%64=63', 'r_len%128=0,even', 'r_len%256=0']),
    "s2016": (2016, 1024, ['c_len%128=0', 'r_inv_sa0%128=127', 'r_len%128=0,odd']),
    "s1856": (1856, 1215, ['c_len%128=63', 'c_primary%64=0', 'r_len%128=127']),
    "s1981": (1981, 1025, ['c_len%128=1', 'r_inv_sa0%128=0']),
    "s749": (749, 1151, ['c_len%128=127', 'r_len%128=1']),
    "s28": (28, 1089, ['c_len%128=65']),
    "s3987": (3987, 1600, ['c_len%128=64', 'c_primary%64=0', 'r_len%128=0,even', 'r_len%256=0']),
    "s2396": (2396, 1343, ['c_len%128=63', 'c_primary%64=63', 'r_len%128=127']),
    "s2310": (2310, 1024, ['c_len%128=0', 'r_inv_sa0%128=0']),
    "s2107": (2107, 1025, ['c_len%128=1', 'r_len%128=1']),
    "s64": (64, 1217, ['c_len%128=65', 'r_inv_sa0%128=127']),
    "s485": (485, 1407, ['c_len%128=127', 'r_len%128=0,odd']),
}
# what every case has, and what the cases must have together
EDGE_COMMON = ["two_rows", "three_rows", "p0<16", "ends_at_last_base", "special_near_start", "special_near_end"]
EDGE_WANTED = (["c_len%%128=%d" % r for r in (0, 1, 63, 64, 65, 127)] + ["c_primary%64=0", "c_primary%64=63"]
               + ["r_len%128=0,even", "r_len%128=0,odd", "r_len%128=1", "r_len%128=127", "r_len%256=0", "r_inv_sa0%128=0", "r_inv_sa0%128=127"]
               + EDGE_COMMON)


def make_edge_genome(seed, length):
    """(base codes 0..4, SNP positions, SNP allele masks, l_seed) of a case: a random genome with a 40-base segment copied to
    position 3 (present twice; its suffixes have fewer than 16 bases in front), another present three times, a third whose second copy
    ends at the last base, N runs and SNPs within 9 bases of the start and within 2 k + 37 of the end, and a random set of single,
    clustered and three-allele SNPs elsewhere (clusters and three-allele sites near an edge move the R text's length off the even
    amounts single SNPs add)."""
    rng = np.random.default_rng(seed)
    n, k = length, (21 if seed % 4 == 0 else 19)
    g = rng.integers(0, 4, n).astype(np.uint8)
    g[3:43] = g[100:140]
    g[300:340] = g[200:240]
    g[400:440] = g[200:240]
    g[n - 40:] = g[500:540]
    g[0:2] = 4
    g[n - 70:n - 67] = 4
    pos = {2: 2, 6: 2, n - 50: 2, n - 10: 2}                          # position -> number of alleles
    for _ in range(int(rng.integers(2, 20))):
        p = int(rng.integers(0, n))
        for j in range(int(rng.choice([1, 1, 2, 3, 4]))):
            q = p + j * int(rng.integers(1, 9))
            if 0 <= q < n:
                pos[q] = 3 if rng.random() < 0.3 else 2
    ps = np.array(sorted(q for q in pos if g[q] < 4), dtype=np.uint32)
    masks = np.zeros(len(ps), dtype=np.uint8)
    for i, q in enumerate(ps):
        alts = rng.permutation(3)[:pos[int(q)] - 1] + 1
        masks[i] = (1 << g[q]) | sum(1 << int((g[q] + a) % 4) for a in alts)
    return g, ps, masks, k


def build_edge_case(seed, length, prefix):
    """Builds the case with the host suffix sorter; the index files go to prefix.*"""
    import salt_amd
    g, pos, masks, k = make_edge_genome(seed, length)
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)[g]
    salt_amd.idx_build_mem([("edge", letters)], [("edge", pos, masks, g[pos])], prefix, k, gpu_device=None, flags=salt_amd.IDX_NO_LP)
    return prefix


def edge_cases(out_dir):
    """{name: index prefix} of every EDGE_CASES entry, built into out_dir."""
    return {name: build_edge_case(seed, length, os.path.join(str(out_dir), name)) for name, (seed, length, _) in EDGE_CASES.items()}


def edge_properties(m):
    """The properties of EDGE_WANTED that the index of Model m has, read off the index files alone."""
    n, k = m.c_seq_len, m.l_seed
    out = set()
    if n % 128 in (0, 1, 63, 64, 65, 127):
        out.add("c_len%%128=%d" % (n % 128))
    if m.c_primary % 64 in (0, 63):
        out.add("c_primary%%64=%d" % (m.c_primary % 64))
    r = m.r_text_len
    if r % 128 == 0:
        out.add("r_len%%128=0,%s" % ("odd" if (r // 128) & 1 else "even"))
    if r % 128 in (1, 127):
        out.add("r_len%%128=%d" % (r % 128))
    if r % 256 == 0:
        out.add("r_len%256=0")
    if m.r_inv_sa0 % 128 in (0, 127):
        out.add("r_inv_sa0%%128=%d" % (m.r_inv_sa0 % 128))
    x, rows = m.wlkt(LKT_LEN)
    rows = rows.astype(np.int64)
    width = rows[:, 1] - rows[:, 0] + 1
    if (width == 2).any():
        out.add("two_rows")
    if (width == 3).any():
        out.add("three_rows")
    two = rows[width == 2]
    p0 = np.concatenate([two[:, 4], two[:, 6]])
    if ((p0 > 0) & (p0 < 16)).any():
        out.add("p0<16")
    if (p0 == n - LKT_LEN).any():
        out.add("ends_at_last_base")
    ln = min(n, m.ref_len)
    special = np.nonzero(m.mask[:ln] != (1 << m.T[:ln].astype(np.int64)))[0]
    multi = np.nonzero(np.isin(m.mask[:ln], (3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15)))[0]
    zero = np.nonzero(m.mask[:ln] == 0)[0]
    if (multi < CTX_N_B).any() and (zero < CTX_N_B).any():
        out.add("special_near_start")
    far = ln - (CTX_A_SEEDS * k + CTX_N_A)
    if (multi >= far).any() and (zero >= far).any() and len(special):
        out.add("special_near_end")
    return out
