"""The error profile's Python statement (tests/errprof_check.py) on the committed goldens: the census that shows each fixture exercises
what it is there for, and the model's own invariants.  The other two statements are compared with this one in test_errprof_host.py and
test_gpu_errprof.py."""
import numpy as np
import pytest

import errprof_check as ec
import snp_check

# golden -> (records counted, reverse, mate 2, base events, mismatches, masked M columns, M columns with a read N, q values, largest cycle)
# at min_mapq 0, as counted when the feature was written
CENSUS = {
    "expect_se_default.sam": (1907, 988, 0, 182760, 1212, 7574, 203, 21, 99),
    "expect_pe_default.sam": (1929, 951, 965, 184971, 923, 7681, 0, 1, 99),
    "expect_gap_se_mid.sam.gz": (1216, 615, 0, 173207, 2387, 7224, 32, 1, 167),
    "expect_ragged_pe.sam": (573, 279, 285, 60891, 568, 2472, 0, 1, 149),
    "expect_gap_pe_short.sam.gz": (902, 451, 451, 123568, 380, 5029, 0, 1, 163),
    "expect_span_default.sam": (40, 19, 0, 3790, 21, 202, 0, 1, 99),
}


@pytest.fixture(scope="module")
def lam():
    return ec.lambda_masks(), ec.lambda_offsets()


def test_the_lambda_mixref_has_sites_and_n(lam):
    masks, _ = lam
    one = (masks != 0) & ((masks & (masks - 1)) == 0)
    assert (len(masks), int(one.sum()), int(((masks & (masks - 1)) != 0).sum()), int((masks == 0).sum())) == (97004, 93086, 3858, 60)


@pytest.mark.parametrize("golden", sorted(CENSUS))
def test_census_of_the_goldens(golden, lam):
    masks, offsets = lam
    st = {}
    E, R, n = ec.tables_of_sam(masks, offsets, snp_check.golden_sam(golden), 0, stats=st)
    got = (n, int(R[:, 5].sum()), int(R[1, 4]), st["events"], st["mismatches"], st["masked"], st["read_n"], len(st["q"]), st["max_cycle"])
    assert got == CENSUS[golden]
    assert n == snp_check.GOLDENS[golden][0] == int(R[:, 4].sum())
    assert int(E.sum()) == st["events"] and int(R[:, 1].sum()) == 0
    assert np.array_equal(R[:, 0], R[:, 2] + R[:, 3] + R[:, 4])


def test_only_one_golden_varies_its_qualities_so_the_others_are_requalified(lam):
    masks, offsets = lam
    st = {}
    ec.tables_of_sam(masks, offsets, snp_check.golden_sam("expect_se_default.sam"), stats=st)
    assert (min(st["q"]), max(st["q"]), len(st["q"])) == (20, 40, 21)
    sam = snp_check.golden_sam("expect_pe_default.sam")
    base = ec.tables_of_sam(masks, offsets, sam)[0]
    for name, fn, qs in (("!", lambda k, L: b"!" * L, {0}), ("~", lambda k, L: b"~" * L, {93}),
                         ("ramp", lambda k, L: bytes(33 + (k + j) % 94 for j in range(L)), set(range(94)))):
        st = {}
        E = ec.tables_of_sam(masks, offsets, ec.requalify(sam, fn), stats=st)[0]
        assert st["q"] == qs, name
        assert np.array_equal(E.sum(axis=2), base.sum(axis=2))          # the qualities move events between q bins only


def test_min_mapq_moves_records_from_counted_to_low_mapq(lam):
    masks, offsets = lam
    for golden, (n0, n20) in snp_check.GOLDENS.items():
        sam = snp_check.golden_sam(golden)
        E0, R0, a = ec.tables_of_sam(masks, offsets, sam, 0)
        E20, R20, b = ec.tables_of_sam(masks, offsets, sam, 20)
        assert (a, b) == (n0, n20) and int(R20[:, 3].sum()) == n0 - n20 and (E20 <= E0).all()


def test_text_round_trips_and_its_margins_are_the_sums_of_e(lam):
    masks, offsets = lam
    E, R, _ = ec.tables_of_sam(masks, offsets, snp_check.golden_sam("expect_gap_pe_short.sam.gz"), 20)
    for full in (False, True):
        p = ec.parse_file(ec.text_of(E, R, 20, full))
        Q, C, S = ec.margins(E)
        assert p["min_mapq"] == 20 and np.array_equal(p["R"], R) and np.array_equal(p["S"], S)
        assert {k: v[:2] for k, v in p["Q"].items()} == {(m, q): (int(Q[m, q, 0]), int(Q[m, q, 1])) for m in (0, 1) for q in range(95) if Q[m, q, 0]}
        assert p["C"] == {(m, c): (int(C[m, c, 0]), int(C[m, c, 1])) for m in (0, 1) for c in range(512) if C[m, c, 0]}
        assert (p["E"] is None) == (not full) and (not full or np.array_equal(p["E"], E))
