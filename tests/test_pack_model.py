"""tests/pack_model.py against itself and against words worked out by hand: what test_gpu_pack_records.py holds k_pack to."""
import numpy as np

import pack_model as pk


def _revcomp(read):
    out = []
    for c in reversed(list(read)):
        c = min(int(c), 4)
        out.append(3 - c if c < 4 else 4)
    return np.array(out, dtype=np.uint8)


def test_pack_model_words_of_a_five_base_read_by_hand():
    """ACGTN: one-hot nibbles LSB first, 2-bit codes and N flags first base highest, strand 1 = NACGT."""
    pm, tb = pk.records(np.array([0, 1, 2, 3, 4], dtype=np.uint8), [0, 5], 5)
    assert pk.geom(5) == {"nw8": 1, "nw16": 1, "nw32": 1, "pm_stride": 4, "tb_stride": 8}
    assert [hex(w) for w in pm[0]] == ["0xf8421", "0x8421f", "0x5"]
    assert [hex(w) for w in tb[0]] == ["0x1b000000", "0x6c00000", "0x8000000", "0x80000000", "0x5"]


def test_pack_model_geometry_of_the_usual_shapes():
    assert pk.geom(100) == {"nw8": 13, "nw16": 7, "nw32": 4, "pm_stride": 28, "tb_stride": 24}
    assert pk.geom(150) == {"nw8": 19, "nw16": 10, "nw32": 5, "pm_stride": 40, "tb_stride": 32}
    assert pk.geom(0) == pk.geom(1)
    assert pk.geom(512)["pm_stride"] == 132 and pk.geom(512)["tb_stride"] == 100


def test_pack_model_strand_1_is_strand_0_of_the_reverse_complement():
    """Every word of strand 1 of a read equals the word of strand 0 of its reverse complement and the other way round, at lengths that end
    inside every word kind, with N and codes above 4 in the reads."""
    rng = np.random.Generator(np.random.PCG64(21))
    for L in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 99, 100, 101, 150, 255, 256, 257, 511, 512):
        for max_len in sorted({max(L, 1), 512}):
            read = rng.choice(np.array([0, 1, 2, 3, 4, 5, 15, 255], dtype=np.uint8), size=L, p=[.22, .22, .22, .22, .06, .02, .02, .02])
            g = pk.geom(max_len)
            pm, tb = pk.records(read, [0, L], max_len)
            pr, tr = pk.records(_revcomp(read), [0, L], max_len)
            n8, n16, n32 = g["nw8"], g["nw16"], g["nw32"]
            assert (pm[0, n8:2 * n8] == pr[0, :n8]).all() and (pm[0, :n8] == pr[0, n8:2 * n8]).all()
            assert (tb[0, n16:2 * n16] == tr[0, :n16]).all() and (tb[0, :n16] == tr[0, n16:2 * n16]).all()
            assert (tb[0, 2 * n16 + n32:2 * n16 + 2 * n32] == tr[0, 2 * n16:2 * n16 + n32]).all()
            assert (tb[0, 2 * n16:2 * n16 + n32] == tr[0, 2 * n16 + n32:2 * n16 + 2 * n32]).all()
            assert pm[0, -1] == L and tb[0, -1] == L and pm.shape[1] == 2 * n8 + 1 and tb.shape[1] == 2 * n16 + 2 * n32 + 1


def test_pack_model_truncates_at_the_pm_words_and_keeps_neighbours_out():
    """A read longer than 8 nw8 bases is cut there on both strands (strand 1 is the reverse complement of the CUT read), and a record
    holds nothing of the read beside it."""
    rng = np.random.Generator(np.random.PCG64(22))
    seqs = rng.integers(0, 4, size=101 + 137 + 30, dtype=np.uint8)
    offs = [0, 101, 238, 268]
    pm, tb = pk.records(seqs, offs, 100)
    cap = 8 * pk.geom(100)["nw8"]
    assert cap == 104 and list(pm[:, -1]) == [101, 104, 30] and list(tb[:, -1]) == [101, 104, 30]
    for r in range(3):
        alone = seqs[offs[r]:min(offs[r + 1], offs[r] + cap)]
        p1, t1 = pk.records(alone, [0, len(alone)], 100)
        assert (p1[0] == pm[r]).all() and (t1[0] == tb[r]).all()
