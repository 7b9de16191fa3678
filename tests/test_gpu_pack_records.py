"""k_pack's records word by word against tests/pack_model.py, through salt_gpu_diag_pack (salt_amd.diag_pack): every defined word of the pm
and the tb record of every read, both strands, and the words between a record's L word and its stride left as they were.

The reads sit inside a larger device tensor, MARGIN bytes from both of its ends, and those bytes hold valid codes that differ from the
batch's own first and last base: a record that reflects a byte in front of the first read or behind the last one shows as a wrong word.
This is a test of content; nothing here is placed against the end of an allocation."""
import numpy as np
import pytest

import pack_model as pk

LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 99, 100, 101, 119, 120, 121, 150, 151, 247, 248, 249, 255, 256, 257, 511, 512)
CODES = (0, 1, 2, 3, 4, 5, 15, 16, 127, 128, 255)
MARGIN = 64


def _random_reads(rng, lengths):
    """Reads of the given lengths: A C G T, 6 % N, 3 % codes above 4."""
    alphabet = np.array([0, 1, 2, 3, 4, 5, 16, 255], dtype=np.uint8)
    return [rng.choice(alphabet, size=int(L), p=[.2275, .2275, .2275, .2275, .06, .01, .01, .01]) for L in lengths]


def _check(reads, max_read_len, lead=0):
    """The batch through k_pack with its first byte `lead` bytes behind the margin (so at byte alignment lead % 4 of a fresh device tensor
    and lead % 16 of its 16-byte units) against the model."""
    import torch
    import salt_amd
    n = len(reads)
    seqs = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads] + [np.zeros(0, dtype=np.uint8)])
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    ends = {min(int(seqs[0]), 4), min(int(seqs[-1]), 4)} if len(seqs) else set()
    around = [c for c in (0, 1, 2, 3) if c not in ends][0]
    buf = np.full(MARGIN + lead + len(seqs) + MARGIN, around, dtype=np.uint8)
    buf[MARGIN + lead:MARGIN + lead + len(seqs)] = seqs
    d_buf = torch.from_numpy(buf).to("cuda:0")
    d_offs = torch.from_numpy(offs.astype(np.int32)).to("cuda:0")
    g, pm, tb = salt_amd.diag_pack(n, max_read_len, d_buf, d_offs, byte_offset=MARGIN + lead)
    assert g == pk.geom(max_read_len)
    want_pm, want_tb = pk.records(seqs, offs, max_read_len)
    for name, got, want, stride in (("pm", pm, want_pm, g["pm_stride"]), ("tb", tb, want_tb, g["tb_stride"])):
        assert got.shape == (n, stride) and want.shape[1] <= stride
        bad = np.argwhere(got[:, :want.shape[1]] != want)
        assert len(bad) == 0, "%s: %d words differ; first: read %d (length %d) word %d: got %#x, want %#x (max_read_len %d, lead %d, %s)" % (
            name, len(bad), bad[0][0], offs[bad[0][0] + 1] - offs[bad[0][0]], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])],
            max_read_len, lead, g)
        assert (got[:, want.shape[1]:] == salt_amd.PACK_FILL).all(), "%s: a word behind the L word was written" % name


@pytest.mark.gpu
@pytest.mark.parametrize("L", LENGTHS)
def test_gpu_pack_uniform_batches_of_every_length(L):
    """67 reads of L bases with max_read_len = L: more than one block at every geometry, the last block partly filled."""
    rng = np.random.Generator(np.random.PCG64(1000 + L))
    _check(_random_reads(rng, [L] * 67), L)


def _mixed(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = rng.permutation(np.resize(np.array(LENGTHS), 257))
    return _random_reads(rng, lengths)


@pytest.mark.gpu
def test_gpu_pack_all_lengths_mixed_in_one_batch():
    """257 reads of all the lengths in one batch of max_read_len 512: reads start at every byte alignment and end inside every word kind."""
    reads = _mixed(7)
    assert {int(o) % 4 for o in np.cumsum([len(r) for r in reads])} == {0, 1, 2, 3}
    _check(reads, 512)


@pytest.mark.gpu
@pytest.mark.parametrize("L", (100, 512))
@pytest.mark.parametrize("n", (1, 2, 15, 16, 17, 63, 64, 65, 257))
def test_gpu_pack_batch_sizes_around_the_block_boundaries(n, L):
    """Blocks take 64 reads of 100 bases and 16 reads of 512 bases: batches that end in front of, at and behind a block's last read."""
    rng = np.random.Generator(np.random.PCG64(2000 + 7 * n + L))
    _check(_random_reads(rng, [L] * n), L)


@pytest.mark.gpu
@pytest.mark.parametrize("lead", (0, 1, 2, 3, 13))
def test_gpu_pack_reads_at_every_byte_alignment_keep_their_neighbours_out(lead):
    """seqs starting at byte lead of a larger tensor whose other bytes hold valid codes: uniform reads of 100 and the mixed batch."""
    rng = np.random.Generator(np.random.PCG64(3000 + lead))
    _check(_random_reads(rng, [100] * 65), 100, lead)
    _check(_random_reads(rng, [1, 2, 3, 5]), 5, lead)
    _check(_mixed(3100 + lead), 512, lead)


def _edge_positions(L):
    pos = {0, L - 1}
    for b in range(8, L, 8):                                    # both sides of every 8-, 16- and 32-base boundary of both strands
        pos |= {b - 1, b, L - b, L - 1 - b}
    return sorted(p for p in pos if 0 <= p < L)


@pytest.mark.gpu
def test_gpu_pack_every_code_at_the_edges_of_reads_and_words():
    """Codes 0 .. 4 and 5, 15, 16, 127, 128, 255, one at a time in a read of other bases, at the first and the last base and on both sides of
    every word boundary of either strand; then several of them in one read."""
    rng = np.random.Generator(np.random.PCG64(4000))
    for L in (100, 97):
        reads = []
        for v in CODES:
            for p in _edge_positions(L):
                r = (rng.integers(0, 3, size=L) + (min(v, 4) + 1)) % 4 if v < 4 else rng.integers(0, 4, size=L)
                r = r.astype(np.uint8)
                r[p] = v
                reads.append(r)
            r = rng.integers(0, 4, size=L).astype(np.uint8)
            r[_edge_positions(L)] = v
            reads.append(r)
        _check(reads, L)


@pytest.mark.gpu
def test_gpu_pack_reads_of_n():
    """Reads of N alone (code 4 and codes above it) at several lengths, and a read of 33 bases with its one N at each position."""
    reads = [np.full(L, v, dtype=np.uint8) for L in (1, 8, 33, 100) for v in (4, 5, 255)]
    _check(reads, 100)
    rng = np.random.Generator(np.random.PCG64(4100))
    single = []
    for p in range(33):
        r = rng.integers(0, 4, size=33).astype(np.uint8)
        r[p] = 4
        single.append(r)
    _check(single, 33)
    _check(single, 100)


@pytest.mark.gpu
def test_gpu_pack_truncates_reads_longer_than_max_read_len():
    """Reads of max_read_len + 1 and + 37 among reads of 100 and 99 with max_read_len 100: the records hold 8 nw8 = 104 bases at most,
    strand 1 is the reverse complement of those, L says 101 and 104."""
    rng = np.random.Generator(np.random.PCG64(5000))
    _check(_random_reads(rng, np.resize(np.array([100, 101, 137, 99, 137, 101, 0, 104, 105]), 67)), 100)
    _check(_random_reads(rng, [101]), 100)
    _check(_random_reads(rng, [137] * 65), 100, 3)


@pytest.mark.gpu
def test_gpu_pack_paired_end_geometry():
    """2 000 mates of 150 bases, as the paired-end path packs them."""
    rng = np.random.Generator(np.random.PCG64(6000))
    _check(_random_reads(rng, [150] * 2000), 150)
