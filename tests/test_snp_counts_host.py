"""Allele counts at the SNP sites on the host: salt_snp_sites and salt_snp_count_sam (the twin of the device's table and kernel) against
the Python statement of the rule in tests/snp_check.py, on the committed goldens."""
import os

import numpy as np
import pytest

import snp_check
from conftest import GOLDEN, LAMBDA

INDEX_DIRS = {"lambda": LAMBDA, **{c: os.path.join(GOLDEN, "index_cases", c) for c in sorted(os.listdir(os.path.join(GOLDEN, "index_cases")))}}


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    sites, _ = snp_check.sites_of_ref(os.path.join(LAMBDA, "idx.ref"))
    yield ix, sites, snp_check.contig_offsets(os.path.join(LAMBDA, "idx.C.ann"))
    ix.destroy()


@pytest.mark.parametrize("case", sorted(INDEX_DIRS))
def test_sites_equal_the_python_decode(case):
    import salt_amd
    d = INDEX_DIRS[case]
    want, masks = snp_check.sites_of_ref(os.path.join(d, "idx.ref"))
    ix = salt_amd.Index.reload(os.path.join(d, "idx"))
    try:
        got = salt_amd.snp_sites(ix)
    finally:
        ix.destroy()
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    if case == "lambda":
        n_alleles = np.array([bin(int(m)).count("1") for m in masks[want]])
        assert (len(masks), len(want), int((n_alleles == 2).sum()), int((n_alleles == 3).sum()), int((masks == 0).sum())) == (97004, 3858, 3739, 119, 60)
        assert want[-1] == 97003 and 97004 % 64 == 44                # a site in the last, partial window


@pytest.mark.parametrize("min_mapq", [0, 20, 255])
@pytest.mark.parametrize("golden", sorted(snp_check.GOLDENS))
def test_counts_equal_the_python_statement(golden, min_mapq, lam):
    import salt_amd
    ix, sites, offsets = lam
    sam = snp_check.golden_sam(golden)
    want, n_rec = snp_check.count_sam(sites, offsets, sam, min_mapq)
    got = salt_amd.snp_count_sam(ix, sam, min_mapq)
    assert got.shape == (len(sites), 4) and got.dtype == np.uint32
    assert np.array_equal(got, want)
    if min_mapq < 255:
        assert n_rec == snp_check.GOLDENS[golden][0 if min_mapq == 0 else 1] and want.sum() > 0
    else:
        assert want.sum() == 0 and n_rec == 0                        # no record of these files has MAPQ 255 and FLAG 4 clear


def test_the_goldens_cover_what_they_are_there_for(lam):
    """None of the comparisons can pass on empty ground: indels, soft clips, a deep site, a read over the contig boundary."""
    ix, sites, offsets = lam
    se, _ = snp_check.count_sam(sites, offsets, snp_check.golden_sam("expect_se_default.sam"))
    assert (int(se.sum()), int((se.sum(axis=1) > 0).sum())) == (7574, 3317)
    se20, _ = snp_check.count_sam(sites, offsets, snp_check.golden_sam("expect_se_default.sam"), 20)
    assert int(se20.sum()) == 3508
    assert snp_check.census(snp_check.golden_sam("expect_gap_se_mid.sam.gz"))[0] >= 1000
    assert snp_check.census(snp_check.golden_sam("expect_pe_default.sam"))[1] >= 40
    assert snp_check.census(snp_check.golden_sam("expect_ragged_pe.sam"))[1] >= 40
    assert snp_check.census(snp_check.golden_sam("expect_gap_pe_short.sam.gz"))[0] >= 300
    span, _ = snp_check.count_sam(sites, offsets, snp_check.golden_sam("expect_span_default.sam"))
    assert int(span.sum(axis=1).max()) >= 30
    # a record of the span fixture starts in the first contig and counts at a site of the second
    edge = offsets["lambdaB_div2pct"]
    crossing = [l for l in snp_check.golden_sam("expect_span_default.sam").split(b"\n") if l and not l.startswith(b"@") and l.split(b"\t")[2] == b"lambdaA"
                and not int(l.split(b"\t")[1]) & 4 and int(l.split(b"\t")[3]) - 1 + len(l.split(b"\t")[9]) > edge]
    assert crossing
    c, _ = snp_check.count_sam(sites, offsets, b"\n".join(crossing))
    assert c[sites >= edge].sum() > 0


def test_counts_accumulate_over_two_calls(lam):
    import salt_amd
    ix, sites, offsets = lam
    a, b = snp_check.golden_sam("expect_se_default.sam"), snp_check.golden_sam("expect_ragged_pe.sam")
    c = salt_amd.snp_count_sam(ix, a)
    first = c.copy()
    assert salt_amd.snp_count_sam(ix, b, counts=c) is c
    assert np.array_equal(c, first + salt_amd.snp_count_sam(ix, b)) and (c != first).any()
    assert np.array_equal(salt_amd.snp_count_sam(ix, a + b), c)


@pytest.mark.parametrize("bad", [b"not a record\n", b"r1\t0\tlambdaA\t10\t30\n", b"r1\t0\tnowhere\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t5M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t4Q\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\tx\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n"])
def test_a_line_that_is_no_sam_record_is_an_error(bad, lam):
    import salt_amd
    ix, _, _ = lam
    good = b"r0\t0\tlambdaA\t1\t30\t4M\t*\t0\t0\tACGT\tIIII\n"
    assert salt_amd.snp_count_sam(ix, b"@HD\tVN:1.0\n\n" + good).sum() >= 0           # header and empty lines are skipped
    with pytest.raises(salt_amd.SaltError, match="snp counts: "):
        salt_amd.snp_count_sam(ix, good + bad)
    with pytest.raises(salt_amd.SaltError, match="contiguous"):
        salt_amd.snp_count_sam(ix, good, counts=np.zeros((3, 4), dtype=np.uint32))


# 2M at lambdaA:4 covers the site at genome position 3; the N behind it is an operation this program does not write
@pytest.mark.parametrize("bad", [b"not a record\n", b"r1\t0\tlambdaA\t10\t30\n", b"r1\t0\tnowhere\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t5M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t4Q\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\tx\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t4\t30\t2M2N\t*\t0\t0\tACGT\tIIII\n"])
def test_a_line_that_is_no_sam_record_adds_nothing(bad, lam):
    import salt_amd
    ix, sites, _ = lam
    assert sites[0] == 3
    assert salt_amd.snp_count_sam(ix, b"r0\t0\tlambdaA\t4\t30\t2M\t*\t0\t0\tAC\tII\n")[0, 0] == 1      # the refused line's first run alone does count
    counts = np.zeros((len(sites), 4), dtype=np.uint32)
    with pytest.raises(salt_amd.SaltError, match="snp counts: "):
        salt_amd.snp_count_sam(ix, bad, counts=counts)
    assert not counts.any()
