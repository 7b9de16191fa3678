"""The four host readers of this program's SAM lines -- the BAM encoder and the twins of the three row tallies -- share one line parser: each
refuses a line that is no record under its own prefix and quotes the line.  Where a line is bad for some of them only, the table says for
which: the encoder takes all nine CIGAR operations and does not hold the CIGAR against SEQ, the SNP and depth twins do not read QUAL, and
only the error profile bounds SEQ at 512 bases."""
import os

import pytest

from conftest import LAMBDA

PREFIX = {"bam": "BAM: ", "snp": "snp counts: ", "depth": "depth: ", "errprof": "error profile: "}
ALL = ("bam", "snp", "depth", "errprof")
TWINS = ("snp", "depth", "errprof")
# the union of the three host test files' bad lines, and who refuses each
CASES = [
    (b"not a record\n", ALL),
    (b"r1\t0\tlambdaA\t10\t30\n", ALL),
    (b"r1\t0\tnowhere\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n", ALL),
    (b"r1\t0\tlambdaA\t10\t30\t5M\t*\t0\t0\tACGT\tIIII\n", TWINS),
    (b"r1\t0\tlambdaA\t10\t30\t4Q\t*\t0\t0\tACGT\tIIII\n", ALL),
    (b"r1\tx\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n", ALL),
    (b"r1\t0\tlambdaA\t10\t30\t2M1D3M\t*\t0\t0\tACGT\tIIII\n", TWINS),
    (b"r1\t0\tlambdaA\t10\t30\t4M\t*\t0\t0\tACGT\tIII\n", ("bam", "errprof")),
    (b"r1\t0\tlambdaA\t10\t30\t513M\t*\t0\t0\t" + b"A" * 513 + b"\t" + b"I" * 513 + b"\n", ("errprof",)),
    (b"r1\t0\tlambdaA\t4\t30\t2M2N\t*\t0\t0\tACGT\tIIII\n", TWINS),
]


@pytest.fixture(scope="module")
def readers():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield salt_amd, {"bam": lambda s: salt_amd.bam_from_sam(ix, s), "snp": lambda s: salt_amd.snp_count_sam(ix, s),
                     "depth": lambda s: salt_amd.depth_add_sam(ix, s), "errprof": lambda s: salt_amd.errprof_add_sam(ix, s)}
    ix.destroy()


@pytest.mark.parametrize("reader", ALL)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_every_reader_refuses_a_bad_line_under_its_own_prefix(case, reader, readers):
    salt_amd, fns = readers
    line, refused_by = CASES[case]
    if reader not in refused_by:
        fns[reader](line)
        return
    with pytest.raises(salt_amd.SaltError) as e:
        fns[reader](line)
    msg = str(e.value)
    assert msg.startswith(PREFIX[reader]) and msg.endswith(" in SAM line '" + line[:-1][:80].decode() + "'"), msg
