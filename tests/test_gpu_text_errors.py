"""The two text entry points of the library (GpuAligner.align_se_text / align_pe_text) where they share their code: the parse errors and
their messages, the read-group and capacity errors, that a refused call leaves the workspace usable, one workspace taken through every
output mode in turn, and a small workspace whose buffers all have to grow.  On the first 8 records of the lambda fixture's reads; the
messages are written out here as the library has always worded them."""
import os

import pytest

import bgzf_check
from conftest import LAMBDA

pytestmark = pytest.mark.gpu

N = 8
SE_ARGS = ["-d", "-c"]
PE_ARGS = ["-d", "-p", "-c", "-a", "350", "-b", "650"]


def records(name, n=N):
    lines = open(os.path.join(LAMBDA, name), "rb").read().split(b"\n")
    return [lines[i:i + 4] for i in range(0, 4 * n, 4)]


def text(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def golden_lines(name, per_record, lo, hi):
    """lines [lo * per_record, hi * per_record) of a golden file's part below the header"""
    body = [l for l in open(os.path.join(LAMBDA, name), "rb").read().splitlines(keepends=True) if not l.startswith(b"@")]
    return b"".join(body[lo * per_record:hi * per_record])


SE = records("reads_se.fq")
PE1, PE2 = records("reads_pe_1.fq"), records("reads_pe_2.fq")


def want_se(lo=0, hi=N):
    return golden_lines("expect_se_default.sam", 1, lo, hi)


def want_pe(lo=0, hi=N):
    return golden_lines("expect_pe_default.sam", 4, lo, hi)        # two records a pair, an empty line behind each


@pytest.fixture(scope="module")
def lambda_index():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield ix
    ix.destroy()


@pytest.fixture(scope="module")
def aligner(lambda_index):
    import salt_amd
    aln = salt_amd.GpuAligner(lambda_index, device=0, max_reads=2 * N)
    aln.set_contigs(lambda_index)
    aln.set_pac(lambda_index)
    yield aln
    aln.close()


def opts(ix, paired, rg=None):
    import salt_amd
    o = salt_amd.AlnOpt.from_argv(PE_ARGS if paired else SE_ARGS, ix.l_seed)[0]
    o.rg_id = rg
    return o


def se_call(aln, ix, recs, rg=None):
    return aln.align_se_text(opts(ix, False, rg), text(recs))


def pe_call(aln, ix, recs1, recs2, rg=None):
    return aln.align_pe_text(opts(ix, True, rg), ix, text(recs1), text(recs2))


def refused(call, message):
    import salt_amd
    with pytest.raises(salt_amd.SaltError) as e:
        call()
    got = str(e.value)
    assert "illegal memory access" not in got and "HSA_STATUS_ERROR" not in got, got
    assert got.endswith(": " + message), got


def good_se(aln, ix, lo=0, hi=N):
    assert se_call(aln, ix, SE[lo:hi]) == (want_se(lo, hi), hi - lo)


def good_pe(aln, ix, lo=0, hi=N):
    assert pe_call(aln, ix, PE1[lo:hi], PE2[lo:hi]) == (want_pe(lo, hi), hi - lo)


def broken(recs, i, how):
    """recs with record i spoilt"""
    r = [list(x) for x in recs]
    if how == "at":
        r[i][0] = b"X" + r[i][0][1:]
    elif how == "plus":
        r[i][2] = b"-"
    elif how == "lengths":
        r[i][3] = r[i][3][:-1]
    elif how == "empty":
        r[i][1] = r[i][3] = b""
    return r


WHAT = {"at": "a record does not start with '@'", "plus": "the third line of a record does not start with '+'",
        "lengths": "sequence and quality lengths differ", "empty": "empty read"}


def test_se_block_of_seven_lines(aligner, lambda_index):
    refused(lambda: aligner.align_se_text(opts(lambda_index, False), b"\n".join(text(SE).split(b"\n")[:7]) + b"\n"),
            "FASTQ block does not hold whole 4-line records (7 lines)")
    good_se(aligner, lambda_index)


def test_pe_blocks_of_eight_and_four_records(aligner, lambda_index):
    refused(lambda: pe_call(aligner, lambda_index, PE1, PE2[:4]), "the two FASTQ blocks hold different numbers of reads (8 / 4)")
    good_pe(aligner, lambda_index)


def test_pe_blocks_of_eight_records_and_seven_lines(aligner, lambda_index):
    seven = b"\n".join(text(PE2).split(b"\n")[:7]) + b"\n"
    refused(lambda: aligner.align_pe_text(opts(lambda_index, True), lambda_index, text(PE1), seven),
            "FASTQ block does not hold whole 4-line records (32 / 7 lines)")
    good_pe(aligner, lambda_index)


@pytest.mark.parametrize("how", sorted(WHAT))
def test_se_record_3_is_not_fastq(how, aligner, lambda_index):
    refused(lambda: se_call(aligner, lambda_index, broken(SE, 3, how)), "input is not 4-line FASTQ at record 3 of the block: " + WHAT[how])
    good_se(aligner, lambda_index)


@pytest.mark.parametrize("mate", [1, 2])
@pytest.mark.parametrize("how", sorted(WHAT))
def test_pe_record_3_of_a_mate_is_not_fastq(how, mate, aligner, lambda_index):
    # the record's index within its own block, whichever mate's block it is
    m1, m2 = (broken(PE1, 3, how), PE2) if mate == 1 else (PE1, broken(PE2, 3, how))
    refused(lambda: pe_call(aligner, lambda_index, m1, m2), "input is not 4-line FASTQ at record 3 of the blocks: " + WHAT[how])
    good_pe(aligner, lambda_index)


class EmptyId(str):
    """"" as a read-group id that AlnOpt hands on as it is (an empty str is what it takes for `no read group`)"""
    def __bool__(self):
        return True


def test_empty_read_group_id(aligner, lambda_index):
    refused(lambda: se_call(aligner, lambda_index, SE, EmptyId()), "empty read group id")
    good_se(aligner, lambda_index)
    refused(lambda: pe_call(aligner, lambda_index, PE1, PE2, EmptyId()), "empty read group id")
    good_pe(aligner, lambda_index)


def test_a_read_group_comes_and_goes(aligner, lambda_index):
    got, n = se_call(aligner, lambda_index, SE, "grp1")
    assert n == N and got.count(b"\tRG:Z:grp1") == N and got.replace(b"\tRG:Z:grp1", b"") == want_se()
    good_se(aligner, lambda_index)


def test_more_records_than_the_workspace_holds(aligner, lambda_index):
    small = aligner.fork(max_reads=4)
    try:
        refused(lambda: se_call(small, lambda_index, SE), "more reads in the block (8) than the workspace holds")
        good_se(small, lambda_index, 0, 4)
        refused(lambda: pe_call(small, lambda_index, PE1, PE2), "more reads in the blocks (16) than the workspace holds")
        good_pe(small, lambda_index, 0, 2)
    finally:
        small.close()


def inflated(blocks):
    return b"".join(t for _, t in bgzf_check.members(blocks))


@pytest.mark.parametrize("paired", [False, True])
def test_one_workspace_through_every_output_mode(paired, aligner, lambda_index):
    ws = aligner.fork()
    call = (lambda: pe_call(ws, lambda_index, PE1, PE2)) if paired else (lambda: se_call(ws, lambda_index, SE))
    want = want_pe() if paired else want_se()
    try:
        sam = call()
        ws.set_sam_bgzf(True)
        sam_z = call()
        ws.set_sam_bgzf(False)
        ws.set_sam_bam(True)
        bam = call()
        ws.set_sam_bgzf(True)
        bam_z = call()
        ws.set_sam_bam(False)
        ws.set_sam_bgzf(False)
        ws.set_polish("lv")
        polished = call()
        ws.set_polish(0)
        again = call()
    finally:
        ws.close()
    assert sam == (want, N) and again == sam
    assert sam_z[1] == N and inflated(sam_z[0]) == want and len(sam_z[0]) < len(want)
    import salt_amd
    assert bam == (salt_amd.bam_from_sam(lambda_index, want), N)
    assert bam_z[1] == N and inflated(bam_z[0]) == bam[0]
    name = "expect_polish_pe_lv.sam" if paired else "expect_polish_se_lv.sam"
    assert polished == (golden_lines(name, 2 if paired else 1, 0, N), N)


def test_a_small_workspace_grows_and_keeps_its_answers(aligner, lambda_index):
    ws = aligner.fork(max_reads=N, max_bases=64)                    # not even one read's bases: every buffer of the text path grows
    try:
        good_se(ws, lambda_index, 0, 2)
        good_se(ws, lambda_index)
        good_se(ws, lambda_index, 0, 2)
        good_pe(ws, lambda_index, 0, 1)
        good_pe(ws, lambda_index, 0, 4)
        good_pe(ws, lambda_index, 0, 1)
    finally:
        ws.close()
