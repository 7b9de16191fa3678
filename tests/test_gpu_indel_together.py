"""The seven row tallies -- SNP counts, depth, the error profile, the genotype sums, the SNP candidates, the summary, the indel table -- on at
once.  Through the library: every table equals the one the same calls leave with only that tally on, and taking the last call back from
the indel table moves it alone.  Through `salt`: the indel file is byte for byte the file it writes alone, the six other files are what they are without
`--indels`, and stdout is what it is with none of them.  Beside test_gpu_discover_together.py, which covers the first five."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import gap_cases
from bgzf_check import strip_pg
from conftest import LAMBDA, ROOT

pytestmark = pytest.mark.gpu

MIN_MAPQ, REF_LEN = 20, 97004
SE = (gap_cases.GAP_CASES["gap_se_mid"][0], ["reads_gap_se_mid.fq.gz"])
PE = (gap_cases.GAP_CASES["gap_pe_short"][0], ["reads_gap_pe_short_1.fq.gz", "reads_gap_pe_short_2.fq.gz"])
TALLIES = ("indel", "stats", "disc", "gt", "errprof", "snp", "depth")


def _fq(name):
    return gzip.decompress(open(os.path.join(LAMBDA, name), "rb").read())


def _enable(aln, which):
    aln.snp_enable("snp" in which, MIN_MAPQ)
    aln.depth_enable("depth" in which, MIN_MAPQ)
    aln.errprof_enable("errprof" in which, MIN_MAPQ)
    aln.gt_enable("gt" in which, MIN_MAPQ)
    aln.disc_enable("disc" in which, MIN_MAPQ, 20)
    aln.stats_enable("stats" in which, MIN_MAPQ)
    aln.indel_enable("indel" in which, MIN_MAPQ, 16)


def _reset(aln):
    aln.snp_counts(reset=True)
    aln.depth_reset()
    aln.errprof_table(reset=True)
    aln.gt_reset()
    aln.disc_reset()
    aln.stats_tables(reset=True)
    aln.indel_reset()


def _tables(aln):
    E, R = aln.errprof_table()
    cells, ct = aln.stats_tables()
    return {"snp": aln.snp_counts(), "depth": aln.depth_fetch(0, REF_LEN + 1), "errprof": np.concatenate([E.ravel(), R.ravel()]), "gt": aln.gt_fetch(),
            "disc": np.concatenate([aln.disc_fetch(0, 0, REF_LEN), aln.disc_fetch(1, 0, REF_LEN + 1).astype(np.uint64)]),
            "stats": np.concatenate([cells, ct.ravel()]),
            "indel": np.concatenate([aln.indel_fetch().ravel(), aln.indel_fetch_diff(0, REF_LEN + 1).astype(np.uint64), aln.indel_stats()])}


def test_all_seven_on_equal_each_alone_and_uncount_moves_one_table():
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
        entries, diff, stats, _ = salt_amd.indel_add_sam(ix, [sams[0], sams[1]], MIN_MAPQ)
        assert np.array_equal(alone_both["indel"]["indel"], np.concatenate([entries.ravel(), diff.astype(np.uint64), stats]))
        assert np.array_equal(diff, alone_both["depth"]["depth"])      # the tally's own diff under the same floor is the coverage's
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
        aln.indel_uncount()                                            # the paired-end call leaves the indel table, and only it
        want["indel"] = alone_se["indel"]["indel"]
        got = _tables(aln)
        for t in TALLIES:
            assert np.array_equal(got[t], want[t]), t
    finally:
        _enable(aln, ())
        aln.close()
        ix.destroy()


def test_salt_with_all_seven_writes_each_file_as_without_the_seventh_and_stdout_as_with_none(tmp_path):
    salt, salt_idx = os.path.join(ROOT, "salt_amd", "bin", "salt"), os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True, stderr=subprocess.DEVNULL, timeout=600)
    reads = gap_cases.plain_paths("gap_se_mid", tmp_path)[0]
    opts = {"snp-counts": [], "depth": [], "error-profile": [], "genotype": [], "stats": [],
            "discover": ["--discover-min-mapq", "0", "--discover-min-alt", "1", "--discover-min-pct", "0", "--discover-all"],
            "indels": ["--indels-min-mapq", "0", "--indels-min-alt", "1", "--indels-min-pct", "0", "--indels-slots", "65536"]}

    def run(which, tag):
        extra = []
        for t in which:
            extra += ["--" + t, str(tmp_path / (tag + "_" + t))] + opts[t]
        p = subprocess.run([salt, "-d", "-c"] + extra + [prefix, reads], capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr[-600:]
        return strip_pg(p.stdout)

    # four runs (a run is some five seconds of start-up, and the runs cannot share the card's memory side by side): none, the six
    # older tallies, all seven, the indels alone.  That the six together write what each writes alone is their own tests' matter.
    six = tuple(t for t in opts if t != "indels")
    none = run((), "none")
    assert none == gap_cases.golden("gap_se_mid")
    assert run(six, "six") == none and run(tuple(opts), "all") == none and run(("indels",), "alone") == none
    for t in opts:
        before, together = (tmp_path / (("alone_" if t == "indels" else "six_") + t)).read_bytes(), (tmp_path / ("all_" + t)).read_bytes()
        assert before == together and len(together) > 1000, t
