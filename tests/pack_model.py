"""k_pack's two records of a batch of reads, stated in plain numpy from DESIGN.md section 3 (PackGeom, salt_kernels.h).

A read is a run of codes: 0..3 = A C G T, 4 = N, anything above 4 reads as N (nst_nt4_table).  A record holds min(L, 8 * nw8) bases of
the read on both strands; strand 1 is the reverse complement with N kept (query_seq_reverse).  With nw8 / nw16 / nw32 = the words of
max_read_len bases at 8 / 16 / 32 bases a word:

  pm record  [0, nw8) forward, [nw8, 2 nw8) reverse: one-hot nibbles, base i of the strand in bits 4 (i % 8) .. + 3 of word i / 8
             (A = 1, C = 2, G = 4, T = 8, N = 15, no base = 0); [2 nw8] = L.
  tb record  [0, nw16) forward, [nw16, 2 nw16) reverse: 2-bit codes, base i in bits 30 - 2 (i % 16) .. + 1 of word i / 16 (N and no base
             read 0); [2 nw16, + nw32) forward, [.., + nw32) reverse: 'is N' flags, base i in bit 31 - i % 32 of word i / 32; then L.

Words behind the L word up to the stride (a multiple of four words) are not part of a record."""
import numpy as np

NO_BASE = 8                        # marks the places behind a read's end in strands()
_NIBBLE = np.array([1, 2, 4, 8, 15, 0, 0, 0, 0], dtype=np.int64)


def geom(max_read_len):
    m = max(1, int(max_read_len))
    nw8, nw16, nw32 = (m + 7) // 8, (m + 15) // 16, (m + 31) // 32
    return {"nw8": nw8, "nw16": nw16, "nw32": nw32, "pm_stride": (2 * nw8 + 4) // 4 * 4, "tb_stride": (2 * nw16 + 2 * nw32 + 4) // 4 * 4}


def strands(seqs, offs, max_read_len):
    """(lengths (n,), codes (n, 2, 32 nw32)): the bases each record holds, strand 0 and strand 1, NO_BASE behind the read's end."""
    g = geom(max_read_len)
    offs = np.asarray(offs, dtype=np.int64)
    seqs = np.asarray(seqs, dtype=np.uint8)
    n, W = len(offs) - 1, 32 * g["nw32"]
    L = np.minimum(offs[1:] - offs[:-1], 8 * g["nw8"])
    col = np.arange(W, dtype=np.int64)[None, :]
    inside = col < L[:, None]
    pad = np.concatenate([seqs, np.zeros(1, dtype=np.uint8)])                      # so that an empty batch of bytes can be indexed
    take = lambda idx: np.minimum(pad[np.clip(idx, 0, len(seqs))].astype(np.int64), 4)   # codes above 4 read as N
    fwd = np.where(inside, take(offs[:-1, None] + col), NO_BASE)
    rev = take(offs[:-1, None] + L[:, None] - 1 - col)
    rev = np.where(inside, np.where(rev < 4, 3 - rev, rev), NO_BASE)
    return L, np.stack([fwd, rev], axis=1).reshape(n, 2, W)


def _words(vals, per, shift):
    """vals (n, 2, W) small integers -> (n, 2, W / per) words, value q of a word shifted left by shift(q)."""
    n, _, W = vals.shape
    sh = np.array([shift(q) for q in range(per)], dtype=np.int64)
    return (vals.reshape(n, 2, W // per, per) << sh).sum(axis=3)


def records(seqs, offs, max_read_len):
    """(pm (n, 2 nw8 + 1), tb (n, 2 nw16 + 2 nw32 + 1)) as int64 arrays of the uint32 words: every defined word of both records."""
    g = geom(max_read_len)
    L, c = strands(seqs, offs, max_read_len)
    n = len(L)
    pmw = _words(_NIBBLE[c], 8, lambda q: 4 * q)[:, :, :g["nw8"]]
    two = _words(np.where(c < 4, c, 0), 16, lambda q: 30 - 2 * q)[:, :, :g["nw16"]]
    isn = _words((c == 4).astype(np.int64), 32, lambda q: 31 - q)[:, :, :g["nw32"]]
    pm = np.concatenate([pmw.reshape(n, -1), L[:, None]], axis=1)
    tb = np.concatenate([two.reshape(n, -1), isn.reshape(n, -1), L[:, None]], axis=1)
    return pm, tb
