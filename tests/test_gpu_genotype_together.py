"""The four row tallies -- SNP counts, depth, the error profile, the genotype sums -- on at once: every table equals the one the same calls
leave with only that tally on, and taking the last call back from the genotype sums moves their table alone.  One single-end and one
paired-end text call over the gapped fixtures, at min_mapq 20, beside test_gpu_tallies_together.py, which covers the first three."""
import gzip
import os

import numpy as np
import pytest

import gap_cases
from conftest import LAMBDA

pytestmark = pytest.mark.gpu

MIN_MAPQ, REF_LEN = 20, 97004
SE = (gap_cases.GAP_CASES["gap_se_mid"][0], ["reads_gap_se_mid.fq.gz"])
PE = (gap_cases.GAP_CASES["gap_pe_short"][0], ["reads_gap_pe_short_1.fq.gz", "reads_gap_pe_short_2.fq.gz"])
TALLIES = ("gt", "errprof", "snp", "depth")


def _fq(name):
    return gzip.decompress(open(os.path.join(LAMBDA, name), "rb").read())


def _enable(aln, which):
    aln.snp_enable("snp" in which, MIN_MAPQ)
    aln.depth_enable("depth" in which, MIN_MAPQ)
    aln.errprof_enable("errprof" in which, MIN_MAPQ)
    aln.gt_enable("gt" in which, MIN_MAPQ)


def _reset(aln):
    aln.snp_counts(reset=True)
    aln.depth_reset()
    aln.errprof_table(reset=True)
    aln.gt_reset()


def _tables(aln):
    E, R = aln.errprof_table()
    return {"snp": aln.snp_counts(), "depth": aln.depth_fetch(0, REF_LEN + 1), "errprof": np.concatenate([E.ravel(), R.ravel()]), "gt": aln.gt_fetch()}


def test_all_four_on_equal_each_alone_and_uncount_moves_one_table():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=8192, max_bases=8192 * 160)
    try:
        aln.set_contigs(ix)
        opt_se, opt_pe = (salt_amd.AlnOpt.from_argv(list(a), ix.l_seed)[0] for a in (SE[0], PE[0]))
        fq, fq1, fq2 = _fq(SE[1][0]), _fq(PE[1][0]), _fq(PE[1][1])
        _enable(aln, TALLIES)                                          # the first enable of each allocates its table
        alone_se, alone_both, sams = {}, {}, None
        for t in TALLIES:
            _enable(aln, (t,))
            _reset(aln)
            sam_se = aln.align_se_text(opt_se, fq)[0]
            alone_se[t] = _tables(aln)
            sam_pe = aln.align_pe_text(opt_pe, ix, fq1, fq2)[0]
            alone_both[t] = _tables(aln)
            assert sams in (None, (sam_se, sam_pe))
            sams = (sam_se, sam_pe)
            for other in TALLIES:                                      # a tally that is off stays empty
                assert other == t or not alone_both[t][other].any(), (t, other)
            assert alone_se[t][t].any() and not np.array_equal(alone_se[t][t], alone_both[t][t]), t
        assert np.array_equal(alone_both["gt"]["gt"][:, :, 0], alone_both["snp"]["snp"].astype(np.uint64))      # the sums' n is the counts' table
        assert np.array_equal(alone_both["gt"]["gt"], salt_amd.gt_add_sam(ix, sams[0] + sams[1], MIN_MAPQ)[0])
        _enable(aln, TALLIES)
        _reset(aln)
        assert aln.align_se_text(opt_se, fq)[0] == sams[0]
        got = _tables(aln)
        for t in TALLIES:
            assert np.array_equal(got[t], alone_se[t][t]), t
        assert aln.align_pe_text(opt_pe, ix, fq1, fq2)[0] == sams[1]
        want = {t: alone_both[t][t] for t in TALLIES}
        got = _tables(aln)
        for t in TALLIES:
            assert np.array_equal(got[t], want[t]), t
        aln.gt_uncount()                                               # the paired-end call leaves the genotype sums, and only them
        want["gt"] = alone_se["gt"]["gt"]
        got = _tables(aln)
        for t in TALLIES:
            assert np.array_equal(got[t], want[t]), t
    finally:
        _enable(aln, ())
        aln.close()
        ix.destroy()
