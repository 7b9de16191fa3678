"""Coverage on the host: salt_depth_add_sam and salt_depth_text (the twins of the device's k_depth_mark and text kernels) against the Python
statement of the rule in tests/depth_check.py, on the committed goldens and on hand-made arrays over lambda's two contigs of 48 502."""
import os

import numpy as np
import pytest

import depth_check
import snp_check
from conftest import LAMBDA

WINDOWS = [1, 7, 64, 1000, 48502, 100000]
EDGE = 48502                                                           # lambdaA | lambdaB_div2pct
REF_LEN = 97004


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    contigs = depth_check.lambda_contigs()
    assert contigs == [("lambdaA", 0, EDGE), ("lambdaB_div2pct", EDGE, EDGE)] and ix.ref_len == REF_LEN
    yield salt_amd, ix, contigs
    ix.destroy()


@pytest.mark.parametrize("min_mapq", [0, 20, 255])
@pytest.mark.parametrize("golden", sorted(snp_check.GOLDENS))
def test_diff_and_both_texts_equal_the_python_statement(golden, min_mapq, lam):
    salt_amd, ix, contigs = lam
    sam = snp_check.golden_sam(golden)
    want, n_want = depth_check.diff_of_sam(contigs, sam, min_mapq)
    got, n_got = salt_amd.depth_add_sam(ix, sam, min_mapq)
    assert got.dtype == np.uint32 and got.shape == (REF_LEN + 1,) and np.array_equal(got, want) and n_got == n_want
    if min_mapq < 255:
        assert n_got == snp_check.GOLDENS[golden][0 if min_mapq == 0 else 1] and want.any()
    else:
        assert n_got == 0 and not want.any()                           # no record of these files has MAPQ 255 and FLAG 4 clear
    assert salt_amd.depth_text(ix, got) == depth_check.text_of(contigs, want)
    for w in WINDOWS:
        assert salt_amd.depth_text(ix, got, w) == depth_check.text_of(contigs, want, w), w


def test_the_goldens_cover_what_they_are_there_for(lam):
    """None of the comparisons passes on empty ground: the forced cut at the contig boundary at equal depth, a depth step on it, the
    figures of the plainest file, and that no golden reaches the genome's end."""
    salt_amd, ix, contigs = lam
    span = snp_check.golden_sam("expect_span_default.sam")
    d = depth_check.depth_of(salt_amd.depth_add_sam(ix, span)[0])
    assert (int(d[EDGE - 1]), int(d[EDGE])) == (37, 37)
    rows = depth_check.parse_per_base(salt_amd.depth_text(ix, salt_amd.depth_add_sam(ix, span)[0]))
    last_a, first_b = [r for r in rows if r[0] == "lambdaA"][-1], [r for r in rows if r[0] != "lambdaA"][0]
    assert last_a[2:] == (EDGE, 37) and (first_b[1], first_b[3]) == (0, 37)      # two lines, though the depth is the same on both sides
    d20 = depth_check.depth_of(salt_amd.depth_add_sam(ix, span, 20)[0])
    assert (int(d20[EDGE - 1]), int(d20[EDGE])) == (19, 19)
    gap = depth_check.depth_of(salt_amd.depth_add_sam(ix, snp_check.golden_sam("expect_gap_se_mid.sam.gz"))[0])
    assert (int(gap[EDGE - 1]), int(gap[EDGE])) == (0, 2)
    se_diff = salt_amd.depth_add_sam(ix, snp_check.golden_sam("expect_se_default.sam"))[0]
    se = depth_check.depth_of(se_diff)
    assert (salt_amd.depth_text(ix, se_diff).count(b"\n"), int(se.max()), int((se == 0).sum())) == (3940, 26, 13599)
    for golden in snp_check.GOLDENS:                                   # no M run of a golden reaches past the genome's end: nothing was cut
        assert depth_check.max_m_end(contigs, snp_check.golden_sam(golden)) <= REF_LEN


def test_an_m_run_past_the_genomes_end_is_cut_not_wrapped_not_refused(lam):
    salt_amd, ix, contigs = lam
    seq = b"A" * 100
    line = b"r0\t0\tlambdaB_div2pct\t%d\t30\t100M\t*\t0\t0\t%s\t%s\n" % (REF_LEN - EDGE - 39, seq, b"I" * 100)      # covers [96964, 97064)
    diff, n = salt_amd.depth_add_sam(ix, line)
    assert n == 1 and np.array_equal(diff, depth_check.diff_of_sam(contigs, line)[0])
    assert np.flatnonzero(diff).tolist() == [REF_LEN - 40, REF_LEN] and diff[REF_LEN - 40] == 1 and diff[REF_LEN] == 0xFFFFFFFF
    assert depth_check.depth_of(diff)[-41:].tolist() == [0] + [1] * 40
    assert salt_amd.depth_text(ix, diff).endswith(b"lambdaB_div2pct\t0\t48462\t0\nlambdaB_div2pct\t48462\t48502\t1\n")
    # a run that begins at or beyond the end adds nothing; a deletion in front of it moves it there
    beyond = b"r1\t0\tlambdaB_div2pct\t%d\t30\t10M50D90M\t*\t0\t0\t%s\t%s\n" % (EDGE - 19, seq, b"I" * 100)      # 10M [96984, 96994), 90M from 97044
    diff2, _ = salt_amd.depth_add_sam(ix, beyond)
    assert np.flatnonzero(diff2).tolist() == [REF_LEN - 20, REF_LEN - 10]


def test_d_is_no_coverage_and_clips_and_insertions_move_in_the_read_only(lam):
    salt_amd, ix, contigs = lam
    line = b"r0\t0\tlambdaA\t101\t30\t5S10M3I20M4D30M2S\t*\t0\t0\t%s\t%s\n" % (b"C" * 70, b"I" * 70)
    diff, _ = salt_amd.depth_add_sam(ix, line)
    assert np.array_equal(diff, depth_check.diff_of_sam(contigs, line)[0])
    assert salt_amd.depth_text(ix, diff).startswith(b"lambdaA\t0\t100\t0\nlambdaA\t100\t130\t1\nlambdaA\t130\t134\t0\nlambdaA\t134\t164\t1\nlambdaA\t164\t48502\t0\n")


def _both(lam, diff, windows=(1, 7, 1000, 48502, 100000)):
    salt_amd, ix, contigs = lam
    text = salt_amd.depth_text(ix, diff)
    assert text == depth_check.text_of(contigs, diff)
    for w in windows:
        assert salt_amd.depth_text(ix, diff, w) == depth_check.text_of(contigs, diff, w), w
    return text


def test_text_of_hand_made_arrays(lam):
    salt_amd, ix, contigs = lam
    zero = np.zeros(REF_LEN + 1, dtype=np.uint32)
    assert _both(lam, zero) == b"lambdaA\t0\t48502\t0\nlambdaB_div2pct\t0\t48502\t0\n"
    assert salt_amd.depth_text(ix, zero, 48502) == b"lambdaA\t0\t48502\t0.00\nlambdaB_div2pct\t0\t48502\t0.00\n"
    # every position its own depth: 1 2 1 2 ...
    alt = np.ones(REF_LEN + 1, dtype=np.uint32)
    alt[2::2] = 0xFFFFFFFF
    alt[REF_LEN] = 0
    text = _both(lam, alt)
    assert text.count(b"\n") == REF_LEN and text.startswith(b"lambdaA\t0\t1\t1\nlambdaA\t1\t2\t2\n")
    assert salt_amd.depth_text(ix, alt, 7).startswith(b"lambdaA\t0\t7\t1.43\nlambdaA\t7\t14\t1.57\n")      # 10 / 7 and 11 / 7, rounded half up
    # a run that ends exactly at the contig's end, and one over the whole of contig A
    for a in (40000, 0):
        run = zero.copy()
        run[a] += 5
        run[EDGE] = (1 << 32) - 5
        text = _both(lam, run)
        assert text.endswith(b"lambdaA\t%d\t48502\t5\nlambdaB_div2pct\t0\t48502\t0\n" % a)
    # ten digits
    big = zero.copy()
    big[10], big[20] = 4000000000, (1 << 32) - 4000000000
    assert _both(lam, big).startswith(b"lambdaA\t0\t10\t0\nlambdaA\t10\t20\t4000000000\nlambdaA\t20\t48502\t0\n")
    assert salt_amd.depth_text(ix, big, 7).startswith(b"lambdaA\t0\t7\t0.00\nlambdaA\t7\t14\t2285714285.71\nlambdaA\t14\t21\t3428571428.57\n")
    # the sum wraps through 2^32 and comes back: 3e9 + 3e9 = 1705032704 mod 2^32, then both are taken again
    wrap = zero.copy()
    wrap[5], wrap[6], wrap[8], wrap[9] = 3000000000, 3000000000, (1 << 32) - 3000000000, (1 << 32) - 3000000000
    assert _both(lam, wrap).startswith(b"lambdaA\t0\t5\t0\nlambdaA\t5\t6\t3000000000\nlambdaA\t6\t8\t1705032704\nlambdaA\t8\t9\t3000000000\nlambdaA\t9\t48502\t0\n")


def test_diff_accumulates_and_a_wrong_size_is_refused(lam):
    salt_amd, ix, contigs = lam
    a, b = snp_check.golden_sam("expect_se_default.sam"), snp_check.golden_sam("expect_ragged_pe.sam")
    d, n_a = salt_amd.depth_add_sam(ix, a)
    first = d.copy()
    d2, n_b = salt_amd.depth_add_sam(ix, b, diff=d)
    assert d2 is d and np.array_equal(d, first + salt_amd.depth_add_sam(ix, b)[0]) and (d != first).any()
    both, n_ab = salt_amd.depth_add_sam(ix, a + b)
    assert np.array_equal(both, d) and n_ab == n_a + n_b
    with pytest.raises(salt_amd.SaltError, match="97005"):
        salt_amd.depth_add_sam(ix, a, diff=np.zeros(REF_LEN, dtype=np.uint32))
    with pytest.raises(salt_amd.SaltError, match="97005"):
        salt_amd.depth_text(ix, np.zeros(REF_LEN + 2, dtype=np.uint32))


@pytest.mark.parametrize("bad", [b"not a record\n", b"r1\t0\tlambdaA\t10\t30\n", b"r1\t0\tnowhere\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t5M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t4Q\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\tx\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t2M1D3M\t*\t0\t0\tACGT\tIIII\n"])
def test_a_line_that_is_no_sam_record_is_an_error_and_adds_nothing(bad, lam):
    salt_amd, ix, _ = lam
    good = b"r0\t0\tlambdaA\t1\t30\t4M\t*\t0\t0\tACGT\tIIII\n"
    assert salt_amd.depth_add_sam(ix, b"@HD\tVN:1.0\n\n" + good)[1] == 1            # header and empty lines are skipped
    diff = np.zeros(REF_LEN + 1, dtype=np.uint32)
    with pytest.raises(salt_amd.SaltError, match="depth: "):
        salt_amd.depth_add_sam(ix, bad, diff=diff)
    assert not diff.any()
