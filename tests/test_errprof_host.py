"""The error profile on the host: salt_errprof_add_sam and salt_errprof_text (the twin of the device's k_errprof and the printer of the
file) against the Python statement of the rule in tests/errprof_check.py, on the committed goldens, on goldens with other qualities, and
on hand-made lines."""
import os

import numpy as np
import pytest

import errprof_check as ec
import snp_check
from conftest import LAMBDA

EDGE, REF_LEN = 48502, 97004


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield salt_amd, ix, ec.lambda_masks(), ec.lambda_offsets()
    ix.destroy()


def _same(lam, sam, min_mapq=0):
    salt_amd, ix, masks, offsets = lam
    E, R, n = salt_amd.errprof_add_sam(ix, sam, min_mapq)
    wE, wR, wn = ec.tables_of_sam(masks, offsets, sam, min_mapq)
    assert E.dtype == np.uint64 and E.shape == ec.SHAPE and R.shape == (2, 8)
    assert np.array_equal(E, wE) and np.array_equal(R, wR) and n == wn
    for full in (False, True):
        text = salt_amd.errprof_text(E, R, min_mapq, full)
        assert text == ec.text_of(wE, wR, min_mapq, full)
    return E, R, n


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("golden", sorted(snp_check.GOLDENS))
def test_tables_and_file_equal_the_python_statement(golden, min_mapq, lam):
    E, R, n = _same(lam, snp_check.golden_sam(golden), min_mapq)
    assert n == snp_check.GOLDENS[golden][0 if min_mapq == 0 else 1] and E.any()


QUALS = {"bang": lambda k, L: b"!" * L, "tilde": lambda k, L: b"~" * L, "ramp": lambda k, L: bytes(33 + (k + j) % 94 for j in range(L)),
         "star": lambda k, L: b"*"}


@pytest.mark.parametrize("how", sorted(QUALS))
@pytest.mark.parametrize("golden", ["expect_pe_default.sam", "expect_gap_se_mid.sam.gz"])
def test_requalified_goldens(golden, how, lam):
    E, _, _ = _same(lam, ec.requalify(snp_check.golden_sam(golden), QUALS[how]))
    used = set(np.flatnonzero(E.sum(axis=(0, 1, 3, 4))).tolist())
    assert used == {"bang": {0}, "tilde": {93}, "ramp": set(range(94)), "star": {94}}[how]


def test_a_byte_below_33_or_above_126_lands_in_none(lam):
    salt_amd, ix, masks, offsets = lam
    seq = b"ACGTACGTAC"
    qual = bytes([32, 33, 126, 127, 1, 200, 64, 64, 64, 64])
    line = b"r0\t0\tlambdaA\t2001\t30\t10M\t*\t0\t0\t" + seq + b"\t" + qual + b"\n"
    E, R, n = _same(lam, line)
    per_cycle_q = {int(c): int(q) for _, c, q, _, _ in zip(*np.nonzero(E))}
    one_bit = [int(masks[2000 + j]) in (1, 2, 4, 8) for j in range(10)]
    want = {j: q for j, q in enumerate([94, 0, 93, 94, 94, 94, 31, 31, 31, 31]) if one_bit[j]}
    assert n == 1 and per_cycle_q == want and len(want) >= 8


def test_reverse_reads_are_counted_in_the_sequencers_coordinates(lam):
    salt_amd, ix, masks, offsets = lam
    # positions 3000 .. 3009 of lambdaA; SEQ as printed is the genome's own bases but one, the read is reverse
    g0 = 3000
    ref = [int(masks[g0 + j]).bit_length() - 1 for j in range(10)]
    assert all(int(masks[g0 + j]) in (1, 2, 4, 8) for j in range(10))
    printed = list(ref)
    printed[2] = (ref[2] + 1) % 4                                      # SEQ index 2 = cycle 7 of a 10-base reverse read
    seq = bytes(b"ACGT"[b] for b in printed)
    qual = bytes(33 + j for j in range(10))                            # as printed: QUAL[s], so cycle 7 has q 2
    E, R, _ = _same(lam, b"r0\t16\tlambdaA\t%d\t30\t10M\t*\t0\t0\t%s\t%s\n" % (g0 + 1, seq, qual))
    assert R[0].tolist() == [1, 0, 0, 0, 1, 1, 0, 0]
    assert E[0, 7, 2, 3 - ref[2], 3 - printed[2]] == 1 and int(E.sum()) == 10
    assert all(E[0, 9 - s, s, 3 - ref[s], 3 - printed[s]] == 1 for s in range(10))


def test_sites_n_clips_indels_and_the_genomes_end(lam):
    salt_amd, ix, masks, offsets = lam
    inner = lambda a: int([g for g in a.tolist() if 10 <= g % EDGE < EDGE - 10][0])      # not within ten positions of a contig's end
    site, n_pos = inner(np.flatnonzero((masks & (masks - 1)) != 0)), inner(np.flatnonzero(masks == 0))
    for g in (site, n_pos):
        contig, off = ("lambdaA", 0) if g < EDGE else ("lambdaB_div2pct", EDGE)
        E, _, _ = _same(lam, b"r0\t0\t%s\t%d\t30\t9M\t*\t0\t0\tACGTACGTA\tIIIIIIIII\n" % (contig.encode(), g - off - 4 + 1))
        assert not E[0, 4].any() and int(E.sum()) == sum(int(masks[g - 4 + j]) in (1, 2, 4, 8) for j in range(9))
    # 5S10M3I20M4D30M2S: cycles 5 .. 14, 18 .. 37, 38 .. 67 of 70; flag 0x80: mate 1
    E, R, _ = _same(lam, b"r0\t128\tlambdaA\t101\t30\t5S10M3I20M4D30M2S\t*\t0\t0\t%s\t%s\n" % (b"C" * 70, b"I" * 70))
    cyc = set(np.flatnonzero(E[1].sum(axis=(1, 2, 3))).tolist())
    assert cyc <= set(range(5, 15)) | set(range(18, 68)) and not E[0].any() and R[1].tolist() == [1, 0, 0, 0, 1, 0, 1, 0]
    # an M run over the genome's end: the columns at and beyond ref_len count nowhere
    E, _, _ = _same(lam, b"r0\t0\tlambdaB_div2pct\t%d\t30\t100M\t*\t0\t0\t%s\t%s\n" % (REF_LEN - EDGE - 39, b"A" * 100, b"I" * 100))
    assert not E[0, 40:].any() and E[0, :40].any()
    # a read's N
    E, _, _ = _same(lam, b"r0\t0\tlambdaA\t5001\t30\t8M\t*\t0\t0\tACNNACGT\tIIIIIIII\n")
    assert not E[0, 2:4].any()


def test_unmapped_and_low_mapq_records_land_in_r_only(lam):
    sam = (b"u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n" b"m\t133\tlambdaA\t10\t255\t*\t=\t10\t0\tACGT\tIIII\n"
           b"l\t0\tlambdaA\t10\t3\t4M\t*\t0\t0\tACGT\tIIII\n" b"\n" b"@CO\tx\n")
    E, R, n = _same(lam, sam, 20)
    assert n == 0 and not E.any() and R.tolist() == [[2, 0, 1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0, 0]]


def test_tables_accumulate_and_a_wrong_size_is_refused(lam):
    salt_amd, ix, _, _ = lam
    a, b = snp_check.golden_sam("expect_se_default.sam"), snp_check.golden_sam("expect_ragged_pe.sam")
    E, R, n_a = salt_amd.errprof_add_sam(ix, a)
    first = E.copy()
    E2, R2, n_b = salt_amd.errprof_add_sam(ix, b, tables=(E, R))
    assert E2 is E and np.array_equal(E, first + salt_amd.errprof_add_sam(ix, b)[0])
    both = salt_amd.errprof_add_sam(ix, a + b)
    assert np.array_equal(both[0], E) and np.array_equal(both[1], R) and both[2] == n_a + n_b
    with pytest.raises(salt_amd.SaltError, match="(?i)shape"):
        salt_amd.errprof_add_sam(ix, a, tables=(np.zeros((2, 512, 95, 16), dtype=np.uint64), R))
    import ctypes
    h = salt_amd.host_lib()
    small = np.zeros(100, dtype=np.uint64)
    assert h.salt_errprof_add_sam(ix._h, a, len(a), 0, small.ctypes.data, small.size, R.ctypes.data) == -1
    assert b"1556480" in h.salt_host_last_error() and not small.any()


def test_only_mates_with_records_are_printed_and_size_only_calls_agree(lam):
    salt_amd, ix, _, _ = lam
    E, R, _ = salt_amd.errprof_add_sam(ix, snp_check.golden_sam("expect_se_default.sam"))
    text = salt_amd.errprof_text(E, R, 0, True)
    p = ec.parse_file(text)
    assert all(k[0] == 0 for k in list(p["Q"]) + list(p["C"])) and text.count(b"\nS\t") == 16 and b"\nR\t1\t" not in text
    assert len(p["Q"]) == 21 and len(p["C"]) == 100 and np.array_equal(p["E"], E)
    zero = salt_amd.errprof_text(np.zeros(ec.SHAPE, dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64))
    assert zero == (b"#salt-error-profile\tv1\tmin_mapq=0\n#R\tmate\tseen\tskipped\tunmapped\tlow_mapq\tcounted\treverse\tgapped\n"
                    b"#Q\tmate\tq\tbases\tmismatches\tempirical\n#C\tmate\tcycle\tbases\tmismatches\n#S\tmate\tref\tread\tcount\n")


@pytest.mark.parametrize("bad", [b"not a record\n", b"r1\t0\tlambdaA\t10\t30\n", b"r1\t0\tnowhere\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t5M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t4Q\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\tx\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n", b"r1\t0\tlambdaA\t10\t30\t2M1D3M\t*\t0\t0\tACGT\tIIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIII\n",
                                 b"r1\t0\tlambdaA\t10\t30\t513M\t*\t0\t0\t" + b"A" * 513 + b"\t" + b"I" * 513 + b"\n"])
def test_a_line_that_is_no_sam_record_is_an_error_and_adds_nothing(bad, lam):
    salt_amd, ix, _, _ = lam
    good = b"r0\t0\tlambdaA\t1\t30\t4M\t*\t0\t0\tACGT\tIIII\n"
    assert salt_amd.errprof_add_sam(ix, b"@HD\tVN:1.0\n\n" + good)[2] == 1            # header and empty lines are skipped
    E, R = np.zeros(ec.SHAPE, dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
    with pytest.raises(salt_amd.SaltError, match="error profile: "):
        salt_amd.errprof_add_sam(ix, bad, tables=(E, R))
    assert not E.any() and not R.any()
