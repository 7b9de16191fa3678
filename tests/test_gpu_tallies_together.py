"""The three row tallies -- SNP counts, depth, the error profile -- on at once: every table equals the one the same calls leave with only that
tally on, and taking the last call back from one tally moves that tally's table alone.  One single-end and one paired-end text call over
the gapped fixtures of the three tallies' own test files, at min_mapq 20, so that the shared row-head decode meets every kind of row it
tells apart."""
import gzip
import os
import re

import numpy as np
import pytest

import gap_cases
from conftest import LAMBDA

pytestmark = pytest.mark.gpu

MIN_MAPQ, REF_LEN = 20, 97004
SE = (gap_cases.GAP_CASES["gap_se_mid"][0], ["reads_gap_se_mid.fq.gz"])
PE = (gap_cases.GAP_CASES["gap_pe_short"][0], ["reads_gap_pe_short_1.fq.gz", "reads_gap_pe_short_2.fq.gz"])
TALLIES = ("errprof", "snp", "depth")                                  # (the order they are taken back in)


def _fq(name):
    return gzip.decompress(open(os.path.join(LAMBDA, name), "rb").read())


def row_kinds(sam, paired):
    """how many record lines of each kind the row-head decode distinguishes; the expected goldens of both fixtures hold every kind of
    their end (checked on the CPU: gap_se_mid 511 forward, 535 reverse, 558 gapped, 56 unmapped, 170 below 20; gap_pe_short 25 clips)"""
    k = dict.fromkeys(("forward", "reverse", "pe_lead_clip", "gapped", "unmapped", "below_floor"), 0)
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            continue
        f = line.split(b"\t")
        flag, mapq, cigar = int(f[1]), int(f[4]), f[5]
        if flag & 4:
            k["unmapped"] += 1
        elif mapq < MIN_MAPQ:
            k["below_floor"] += 1
        else:
            k["reverse" if flag & 16 else "forward"] += 1
            k["pe_lead_clip"] += bool(paired and re.match(rb"\d+S", cigar))
            k["gapped"] += bool(re.search(rb"[ID]", cigar))
    return k


def _enable(aln, which):
    aln.snp_enable("snp" in which, MIN_MAPQ)
    aln.depth_enable("depth" in which, MIN_MAPQ)
    aln.errprof_enable("errprof" in which, MIN_MAPQ)


def _reset(aln):
    aln.snp_counts(reset=True)
    aln.depth_reset()
    aln.errprof_table(reset=True)


def _tables(aln):
    E, R = aln.errprof_table()
    return {"snp": aln.snp_counts(), "depth": aln.depth_fetch(0, REF_LEN + 1), "errprof": np.concatenate([E.ravel(), R.ravel()])}


def test_all_three_on_equal_each_alone_and_uncount_moves_one_table():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=8192, max_bases=8192 * 160)
    try:
        aln.set_contigs(ix)
        opt_se, opt_pe = (salt_amd.AlnOpt.from_argv(list(a), ix.l_seed)[0] for a in (SE[0], PE[0]))
        fq, fq1, fq2 = _fq(SE[1][0]), _fq(PE[1][0]), _fq(PE[1][1])
        _enable(aln, TALLIES)                                          # the first enable of each allocates its table
        # each alone: after the single-end call, and after the paired-end call behind it
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
        # the condition: the calls' own SAM holds every kind of row
        k_se, k_pe = row_kinds(sams[0], False), row_kinds(sams[1], True)
        assert all(k_se[k] > 0 for k in ("forward", "reverse", "gapped", "unmapped", "below_floor")), k_se
        assert all(v > 0 for v in k_pe.values()), k_pe
        # all three on
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
        # the paired-end call is taken back, one tally at a time
        uncount = {"errprof": aln.errprof_uncount, "snp": lambda: salt_amd.gpu_lib().salt_gpu_ws_snp_uncount(aln._ws), "depth": aln.depth_uncount}
        for t in TALLIES:
            assert uncount[t]() in (None, 0)
            want[t] = alone_se[t][t]
            got = _tables(aln)
            for other in TALLIES:
                assert np.array_equal(got[other], want[other]), (t, other)
    finally:
        _enable(aln, ())
        aln.close()
        ix.destroy()
