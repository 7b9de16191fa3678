"""The run's summary on the host: salt_stats_add_sam and salt_stats_text (the twin of the device's k_stats_add and the printer of the file)
against the Python statement in tests/stats_check.py, over every committed golden SAM at floors 0 and 20, and on hand-made lines."""
import glob
import os

import numpy as np
import pytest

import snp_check
import stats_check as sc
import test_stats_model as hand
from conftest import LAMBDA

GOLDENS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(LAMBDA, "expect_*.sam")) + glob.glob(os.path.join(LAMBDA, "expect_*.sam.gz")))
# Polished records (`polish`'s and `salt --polish`'s output) are not the aligner's lines: the Landau-Vishkin re-scoring prints a mapped record
# whose alignment it dropped with CIGAR `*`.  No twin reads those (under --polish the tallies run on the device, over the rows); the twin
# refuses these four goldens, which hold such records, and the statement is compared on the other 25.
NO_CIGAR = ["expect_polish_edge_pe.sam", "expect_polish_edge_se.sam", "expect_polish_se_lv.sam", "expect_polish_se_r1_lv.sam"]


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield salt_amd, ix, sc.lambda_contigs()
    ix.destroy()


def _same(lam, sam, min_mapq=0):
    salt_amd, ix, contigs = lam
    cells, ct, n = salt_amd.stats_add_sam(ix, sam, min_mapq)
    w_cells, w_ct, w_n = sc.tables_of_sam(contigs, sam, min_mapq)
    assert cells.dtype == np.uint64 and cells.shape == (sc.CELLS,) and ct.shape == (len(contigs), 8)
    for name, t in sc.split(cells).items():
        w = sc.split(w_cells)[name]
        assert np.array_equal(t, w), (name, np.argwhere(t != w)[:4].tolist(), t[t != w][:4].tolist(), w[t != w][:4].tolist())
    assert np.array_equal(ct, w_ct) and n == w_n
    text = salt_amd.stats_text(ix, cells, ct, min_mapq)
    assert text == sc.text_of(contigs, w_cells, w_ct, min_mapq)
    p = sc.parse_file(text)
    assert p["min_mapq"] == min_mapq and np.array_equal(p["cells"], cells) and np.array_equal(p["ct"], ct)
    assert p["names"] == [c[0] for c in contigs] and p["lengths"] == [c[2] for c in contigs]
    return cells, ct, n


def test_the_index_and_the_ann_file_agree_on_the_contigs(lam):
    salt_amd, ix, contigs = lam
    assert [(c[2].decode(), c[0]) for c in ix.contigs()] == [(name, off) for name, off, _ in contigs] and len(GOLDENS) == 29


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("golden", [g for g in GOLDENS if g not in NO_CIGAR])
def test_tables_and_file_equal_the_python_statement(golden, min_mapq, lam):
    cells, ct, n = _same(lam, snp_check.golden_sam(golden), min_mapq)
    T = sc.split(cells)
    assert n > 0 and int(T["SN"][:, 4].sum()) == n == int(ct[:, 2:4].sum()) and int(T["MQ"].sum()) == int(ct[:, :2].sum())
    if golden in snp_check.GOLDENS:
        assert n == snp_check.GOLDENS[golden][0 if min_mapq == 0 else 1]


@pytest.mark.parametrize("golden", NO_CIGAR)
def test_a_polished_golden_with_a_mapped_record_without_cigar_is_refused_whole(golden, lam):
    salt_amd, ix, contigs = lam
    assert golden in GOLDENS
    cells, ct = np.zeros(sc.CELLS, dtype=np.uint64), np.zeros((len(contigs), 8), dtype=np.uint64)
    with pytest.raises(salt_amd.SaltError, match="stats: malformed CIGAR"):
        salt_amd.stats_add_sam(ix, snp_check.golden_sam(golden), tables=(cells, ct))


def test_the_goldens_reach_every_table_and_every_sn_cell_but_skipped():
    """What the device tests rely on: the inputs they align can make every table and every SN cell non-zero (skipped reads print as empty
    lines, so that cell is the device's alone)."""
    contigs = sc.lambda_contigs()
    t = None
    for g, q in (("expect_pe_default.sam", 20), ("expect_gap_pe_short.sam.gz", 0), ("expect_pe_geom_a350.sam.gz", 0), ("expect_gap_se_mid.sam.gz", 0)):
        t = sc.tables_of_sam(contigs, snp_check.golden_sam(g), q, tables=t)[:2]
    T = sc.split(t[0])
    assert all(T[name].any() for name in sc.TABLES) and t[1][:, :6].all()
    sn = T["SN"].sum(axis=0)
    assert [k for k in range(16) if not sn[k]] == [1], sn.tolist()
    assert T["OR"][:3].all() and not T["OR"][3] and T["ID"][0].any() and T["ID"][1].any() and T["XA"][:, 1:].any()


def test_the_hand_written_pairs_of_the_model_test(lam):
    """the same lines on contigs of the lambda index: every cell the model test spells out, but the two that depend on the genome's end"""
    salt_amd, ix, contigs = lam
    sam = hand.SAM.replace(b"\tc1\t", b"\tlambdaA\t").replace(b"\tc2\t", b"\tlambdaB_div2pct\t").replace(b"XA:Z:c1,+1,10M,0;c2,", b"XA:Z:lambdaA,+1,10M,0;lambdaA,")
    cells, ct, n = _same(lam, sam)
    T = sc.split(cells)
    want = [list(r) for r in hand.SN_0]
    want[0][12] += 5                                                 # H's mate 0 does not cross this genome's end
    assert n == 13 and T["SN"].tolist() == want and T["IS"][4095] == 1 and T["IS"][4096] == 2 and T["OR"].tolist() == [2, 2, 1, 0]
    assert T["ID"][0, 64] == 2 and T["ID"][1, 64] == 2 and T["GC"][0, 101] == 1 and T["GC"][1, 13] == 1 and T["GC"][0, 38] == 1


def test_a_record_at_and_across_the_genomes_last_position(lam):
    salt_amd, ix, contigs = lam
    name, off, length = contigs[-1]
    at = b"r0\t0\t%s\t%d\t30\t40M\t*\t0\t0\t%s\t%s\n" % (name.encode(), length - 39, b"A" * 40, b"I" * 40)
    over = b"r1\t16\t%s\t%d\t30\t40M\t*\t0\t0\t%s\t%s\n" % (name.encode(), length - 9, b"A" * 40, b"I" * 40)
    cells, ct, n = _same(lam, at + over)
    assert n == 2 and sc.split(cells)["SN"][0, 12] == 50 and ct[-1].tolist() == [2, 0, 2, 0, 1, 50, 0, 0]


def test_unmapped_and_low_mapq_records(lam):
    sam = (b"u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n" b"m\t133\tlambdaA\t10\t255\t*\t=\t10\t0\tACGT\tIIII\n"
           b"l\t0\tlambdaA\t10\t3\t4M\t*\t0\t0\tACGT\tIIII\n" b"\n" b"@CO\tx\n")
    cells, ct, n = _same(lam, sam, 20)
    T = sc.split(cells)
    assert n == 0 and T["SN"][:, :5].tolist() == [[2, 0, 1, 1, 0], [1, 0, 1, 0, 0]] and T["MQ"][0, 3] == 1 and int(T["MQ"].sum()) == 1
    assert ct[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and int(T["RL"][:, 4].sum()) == 3 and int(T["GC"][:, 50].sum()) == 3


def test_tables_accumulate_and_a_wrong_size_is_refused(lam):
    salt_amd, ix, _ = lam
    a, b = snp_check.golden_sam("expect_se_default.sam"), snp_check.golden_sam("expect_ragged_pe.sam")
    cells, ct, n_a = salt_amd.stats_add_sam(ix, a)
    first = cells.copy()
    cells2, ct2, n_b = salt_amd.stats_add_sam(ix, b, tables=(cells, ct))
    assert cells2 is cells and np.array_equal(cells, first + salt_amd.stats_add_sam(ix, b)[0])
    both = salt_amd.stats_add_sam(ix, a + b)
    assert np.array_equal(both[0], cells) and np.array_equal(both[1], ct) and both[2] == n_a + n_b
    with pytest.raises(salt_amd.SaltError, match="(?i)shape"):
        salt_amd.stats_add_sam(ix, a, tables=(np.zeros(100, dtype=np.uint64), ct))
    h = salt_amd.host_lib()
    small = np.zeros(100, dtype=np.uint64)
    assert h.salt_stats_add_sam(ix._h, a, len(a), 0, small.ctypes.data, small.size, ct.ctypes.data, ct.size) == -1
    assert b"6021" in h.salt_host_last_error() and not small.any()
    assert h.salt_stats_add_sam(ix._h, a, len(a), 0, cells.ctypes.data, cells.size, ct.ctypes.data, 8) == -1
    assert set(salt_amd.stats_split(cells)) == set(sc.TABLES) and salt_amd.STATS_TABLES == sc.TABLES and salt_amd.STATS_CELLS == sc.CELLS


def test_the_file_of_empty_tables_and_size_only_calls(lam):
    salt_amd, ix, contigs = lam
    zero = salt_amd.stats_text(ix, np.zeros(sc.CELLS, dtype=np.uint64), np.zeros((len(contigs), 8), dtype=np.uint64), 7)
    want = sc.HEAD % 7 + "".join("SN\t0\t%s\t0\n" % k for k in sc.SN_KEYS) + "ISQ\t0\t.\t.\t.\t.\nOR\t0\t0\t0\n" + "".join("CT\t%s\t%d\t0\t0\t0\t0\t0\t0\n" % (c[0], c[2]) for c in contigs)
    assert zero == want.encode()
    h = salt_amd.host_lib()
    cells, ct, _ = salt_amd.stats_add_sam(ix, snp_check.golden_sam("expect_pe_default.sam"))
    full = salt_amd.stats_text(ix, cells, ct)
    part = np.zeros(10, dtype=np.uint8)
    assert h.salt_stats_text(ix._h, cells.ctypes.data, cells.size, ct.ctypes.data, ct.size, 0, part.ctypes.data, 10) == len(full) and bytes(part) == full[:10]


GOOD = b"r0\t99\tlambdaA\t1\t30\t4M\t=\t200\t203\tACGT\tIIII\n"


@pytest.mark.parametrize("bad", [b"not a record\n", b"r1\t0\tlambdaA\t10\t30\n", b"r1\t0\tnowhere\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t5M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t4Q\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\tx\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t2M1D3M\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t0\t30\t4M\t*\t0\t0\tACGT\tIIII\n", b"r1\t99\tlambdaA\t10\t30\t4M\tnowhere\t20\t0\tACGT\tIIII\n",
                                 b"r1\t99\tlambdaA\t10\t30\t4M\t=\tx\t0\tACGT\tIIII\n", b"r1\t99\tlambdaA\t10\t30\t4M\t=\t20\t1e3\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t4M\t*\t0\t0\t\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t513M\t*\t0\t0\t" + b"A" * 513 + b"\t" + b"I" * 513 + b"\n"])
def test_a_line_that_is_no_sam_record_is_an_error_and_adds_nothing(bad, lam):
    salt_amd, ix, contigs = lam
    assert salt_amd.stats_add_sam(ix, b"@HD\tVN:1.0\n\n" + GOOD)[2] == 1              # header and empty lines are skipped
    cells, ct = np.zeros(sc.CELLS, dtype=np.uint64), np.zeros((len(contigs), 8), dtype=np.uint64)
    with pytest.raises(salt_amd.SaltError, match="stats: "):
        salt_amd.stats_add_sam(ix, bad, tables=(cells, ct))
    assert not cells.any() and not ct.any()
