"""The Python statement of `salt --stats` (tests/stats_check.py) on a hand-written SAM whose expected cells are spelled out here, worked out
by hand from the definition of the tables: both mates, an unmapped mate, a pair across two contigs, each orientation, TLEN at 4095, 4096
and 4097, a read of all N, GC roundings at x.5, I and D of length 64 and 65, a record at the genome's last position and one across it."""
import numpy as np

import stats_check as sc

CONTIGS = [("c1", 0, 10000), ("c2", 10000, 500)]                   # ref_len 10500
S10 = "ACGTACGTAC"                                                 # 3 C + 2 G of 10: 50 %


def _rec(name, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, *tags):
    return "\t".join([name, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, "I" * len(seq)] + list(tags))


PAIRS = [
    # A: inward, |TLEN| 4095
    _rec("A", 99, "c1", 100, 60, "10M", "=", 4185, 4095, S10), _rec("A", 147, "c1", 4185, 60, "10M", "=", 100, -4095, S10),
    # B: outward (mate 0 reverse at 1000, its forward mate behind it), |TLEN| 4096
    _rec("B", 83, "c1", 1000, 60, "10M", "=", 5086, 4096, S10), _rec("B", 163, "c1", 5086, 60, "10M", "=", 1000, -4096, S10),
    # C: both forward, |TLEN| 4097
    _rec("C", 67, "c1", 200, 60, "10M", "=", 4288, 4097, S10), _rec("C", 131, "c1", 4288, 60, "10M", "=", 200, -4097, S10),
    # D: mate 0 all N with soft clips, mate 1 unmapped and printed at its mate's place; 1 C of 8: 12.5 % -> 13
    _rec("D", 73, "c1", 300, 30, "3S5M2S", "=", 300, 0, "N" * 10), _rec("D", 133, "c1", 300, 255, "*", "=", 300, 0, "CAAAAAAA"),
    # E: across the contigs; mate 0 has 3 of 8: 37.5 % -> 38 and MAPQ 10; mate 1 ends at the genome's last position (10000 + 493 - 1 + 8 = 10500)
    _rec("E", 65, "c1", 9000, 10, "8M", "c2", 493, 0, "CCGAAAAA"), _rec("E", 145, "c2", 493, 40, "8M", "c1", 9000, 0, "ACGTNNNN"),
    # F: inward, outside the window; I and D of 64 and 65; two XA entries
    _rec("F", 97, "c1", 2000, 60, "5M64I5M65D5M", "=", 2500, 0, "A" * 79, "NM:i:129", "XA:Z:c1,+1,10M,0;c2,-5,10M,1;"),
    _rec("F", 145, "c1", 2500, 60, "5M65I5M64D5M1I2D", "=", 2000, 0, "G" * 81, "NM:i:132"),
    # H: outward on c2; mate 0 runs 5 columns past the genome's end
    _rec("H", 97, "c2", 496, 60, "10M", "=", 400, 0, S10), _rec("H", 145, "c2", 400, 60, "10M", "=", 496, 0, S10),
]
SAM = ("@HD\tVN:1.0\n" + "\n".join(PAIRS[:6]) + "\n\n\n" + "\n".join(PAIRS[6:]) + "\n").encode()      # (the blank lines of a skipped pair)

#          seen skip unm low cnt rev gap xa prop m_unm m_other bases m_b i_b d_b s_b
SN_0 = [[7, 0, 0, 0, 7, 1, 2, 1, 3, 1, 1, 137, 63, 64, 65, 5],
        [7, 0, 1, 0, 6, 4, 1, 0, 3, 0, 1, 137, 63, 66, 66, 0]]
SN_20 = [[7, 0, 0, 1, 6, 1, 2, 1, 3, 1, 0, 137, 55, 64, 65, 5], SN_0[1]]
SPARSE = {                                                         # table -> {index: count}, every other cell 0
    "MQ": {(0, 60): 5, (0, 30): 1, (0, 10): 1, (1, 60): 5, (1, 40): 1},
    "RL": {(0, 10): 5, (0, 8): 1, (0, 79): 1, (1, 10): 4, (1, 8): 2, (1, 81): 1},
    "GC": {(0, 50): 4, (0, 101): 1, (0, 38): 1, (0, 0): 1, (1, 50): 5, (1, 13): 1, (1, 100): 1},
    "XA": {(0, 0): 6, (0, 2): 1, (1, 0): 6},
    "IS": {(4095,): 1, (4096,): 2},
    "OR": {(0,): 2, (1,): 2, (2,): 1},
    "ID": {(0, 64): 2, (0, 1): 1, (1, 64): 2, (1, 2): 1},
}
CT_0 = [[6, 4, 6, 4, 3, 103, 0, 0], [1, 2, 1, 2, 2, 23, 0, 0]]
CT_20 = [[6, 4, 5, 4, 3, 95, 0, 0], CT_0[1]]


def _expect(sn, sparse, ct):
    cells = np.zeros(sc.CELLS, dtype=np.uint64)
    T = sc.split(cells)
    T["SN"][:] = sn
    for name, items in sparse.items():
        for at, v in items.items():
            T[name][at] = v
    return cells, np.array(ct, dtype=np.uint64)


def _same(got, want):
    for name in sc.TABLES:
        g, w = sc.split(got[0])[name], sc.split(want[0])[name]
        assert np.array_equal(g, w), (name, np.argwhere(g != w).tolist(), g[g != w].tolist(), w[g != w].tolist())
    assert np.array_equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())


def test_the_tables_tile_the_cells():
    at = 0
    for name in ("SN", "MQ", "RL", "GC", "XA", "IS", "OR", "ID"):
        assert sc.TABLES[name][0] == at
        at += int(np.prod(sc.TABLES[name][1]))
    assert at == sc.CELLS == 6021


def test_hand_written_pairs_at_floor_0():
    cells, ct, n = sc.tables_of_sam(CONTIGS, SAM, 0)
    assert n == 13
    _same((cells, ct), _expect(SN_0, SPARSE, CT_0))


def test_hand_written_pairs_at_floor_20():
    cells, ct, n = sc.tables_of_sam(CONTIGS, SAM, 20)
    assert n == 12
    sparse = dict(SPARSE, XA={(0, 0): 5, (0, 2): 1, (1, 0): 6})
    _same((cells, ct), _expect(SN_20, sparse, CT_20))


def test_two_texts_add_into_the_same_tables():
    t = sc.tables_of_sam(CONTIGS, SAM, 0)
    cells, ct, _ = sc.tables_of_sam(CONTIGS, SAM, 0, tables=t[:2])
    want = _expect(SN_0, SPARSE, CT_0)
    assert np.array_equal(cells, 2 * want[0]) and np.array_equal(ct, 2 * want[1])


def test_the_file_of_the_hand_written_pairs():
    cells, ct, _ = sc.tables_of_sam(CONTIGS, SAM, 0)
    text = sc.text_of(CONTIGS, cells, ct, 0)
    lines = text.decode().split("\n")
    assert lines[0] == "#salt-stats\tv1\tmin_mapq=0\tISQ mean: hundredths, the >=4096 bin left out"
    assert lines[1] == "SN\t0\tseen\t7" and lines[16] == "SN\t0\ts_bases\t5" and lines[17] == "SN\t1\tseen\t7" and lines[33].startswith("MQ\t0\t10\t1")
    for want in ("GC\t0\tnone\t1", "GC\t1\t13\t1", "GC\t0\t38\t1", "IS\t4095\t1", "IS\t>=4096\t2", "ISQ\t3\t4095\t>=4096\t>=4096\t4095.00", "OR\t2\t2\t1",
                 "ID\t1\t1\t0", "ID\t2\t0\t1", "ID\t>=64\t2\t2", "CT\tc1\t10000\t6\t4\t6\t4\t3\t103", "CT\tc2\t500\t1\t2\t1\t2\t2\t23", "XA\t0\t2\t1"):
        assert want in lines, want
    assert "IS\t4096\t2" not in lines and not any(l.startswith("ID\t64") or l.startswith("ID\t0\t") for l in lines)
    p = sc.parse_file(text)
    assert p["min_mapq"] == 0 and np.array_equal(p["cells"], cells) and np.array_equal(p["ct"], ct)
    assert p["names"] == ["c1", "c2"] and p["lengths"] == [10000, 500] and p["isq"] == ["3", "4095", ">=4096", ">=4096", "4095.00"]


def test_single_end_prints_mate_0_only_and_an_empty_insert_size_line():
    sam = "\n".join([_rec("r1", 0, "c1", 10, 60, "10M", "*", 0, 0, S10), _rec("r2", 16, "c2", 1, 3, "4M1D6M", "*", 0, 0, S10, "XA:Z:c1,+7,10M,1;"),
                     _rec("r3", 4, "*", 0, 0, "*", "*", 0, 0, "NNNN")]).encode() + b"\n"
    cells, ct, n = sc.tables_of_sam(CONTIGS, sam, 0)
    T = sc.split(cells)
    assert n == 2 and T["SN"][0].tolist() == [3, 0, 1, 0, 2, 1, 1, 1, 0, 0, 0, 24, 20, 0, 1, 0] and not T["SN"][1].any()
    assert not T["IS"].any() and not T["OR"].any() and T["ID"][1, 1] == 1 and T["XA"][0].tolist() == [1, 1, 0, 0, 0, 0, 0, 0]
    assert ct.tolist() == [[1, 0, 1, 0, 0, 10, 0, 0], [1, 0, 1, 0, 1, 10, 0, 0]]
    text = sc.text_of(CONTIGS, cells, ct, 0).decode()
    assert "\nSN\t1\t" not in text and "\nISQ\t0\t.\t.\t.\t.\n" in text and "\nOR\t0\t0\t0\n" in text and "\nGC\t0\tnone\t1\n" in text
    p = sc.parse_file(text.encode())
    assert np.array_equal(p["cells"], cells) and np.array_equal(p["ct"], ct)


def test_the_insert_size_quartiles_and_the_mean_in_hundredths():
    IS = np.zeros(4097, dtype=np.uint64)
    IS[[100, 200, 300, 301]] = [1, 1, 1, 1]
    assert sc.isq(IS) == (4, [100, 200, 300], 22525)               # 901 / 4 = 225.25
    IS[:] = 0
    IS[[10, 11]] = [1, 2]
    assert sc.isq(IS) == (3, [10, 11, 11], 1067)                   # 32 / 3 = 10.666..., rounded half up to 10.67
    IS[:] = 0
    IS[4096] = 5
    assert sc.isq(IS) == (5, [4096, 4096, 4096], None)
    assert [sc.gc_bin(s) for s in (b"CAAAAAAA", b"CCGAAAAA", b"NNNN", b"GGGGGGGN", b"ACGT", b"CAA")] == [13, 38, 101, 100, 50, 33]
