"""The gapped pass of the aligner (k_heavy -> k_gap -> k_gapfin -> k_cigar, the inline wave route, the overflow pass) on reads that all
need it: the gap fixture the real reference answered (tests/golden/make_gap_fixture.py, tests/gap_cases.py) through the library, the
`salt` binary and every switched shape of the pass; reads inside a tandem repeat against the CPU oracle; and the Landau-Vishkin units on
the shape vectors of oracle/ref_harness.c --shapes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_check
import gap_cases
from bgzf_check import strip_pg
from conftest import GOLDEN, LAMBDA, ROOT

pytestmark = pytest.mark.gpu

SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=4096)
    yield salt_amd, idx, aln
    aln.close()
    idx.destroy()


@pytest.mark.parametrize("case", sorted(gap_cases.GAP_CASES))
def test_gpu_sam_matches_reference_on_the_gap_fixture(case, lam):
    """(a) alnse_core1 / alnpe_core1 + sam_text / sam_text_pe: the golden bytes, band by band."""
    salt_amd, idx, aln = lam
    got, want = gap_cases.align_case(salt_amd, idx, aln, case), gap_cases.golden(case)
    n, n_gap, _, _ = gap_cases.census(want)
    print("%s: %d records compared, %d of them gapped" % (case, n, n_gap))
    assert got == want, gap_cases.diff_message(got, want)


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("gapidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


@pytest.mark.parametrize("case", sorted(gap_cases.GAP_CASES))
def test_cli_sam_and_bam_match_reference_on_the_gap_fixture(case, lambda_cli_index, tmp_path):
    """(b) The `salt` binary on the FASTQ files through the device text path (the SAM kernels' general MD walk, ^ deletions, XA
    CIGARs, soft clips), and `salt --bam` decoded by tests/bam_check.py: the golden records."""
    args, _ = gap_cases.GAP_CASES[case]
    want, fqs = gap_cases.golden(case), gap_cases.plain_paths(case, tmp_path)
    out = subprocess.run([SALT] + args + [lambda_cli_index] + fqs, capture_output=True, timeout=300)
    assert out.returncode == 0 and b"text path" in out.stderr, out.stderr[-600:]
    assert strip_pg(out.stdout) == want, gap_cases.diff_message(strip_pg(out.stdout), want)
    bam = subprocess.run([SALT] + args + ["--bam", lambda_cli_index] + fqs, capture_output=True, timeout=300)
    assert bam.returncode == 0 and b"BAM output: device records" in bam.stderr, bam.stderr[-600:]
    text, lines, _ = bam_check.decode_stream(bam.stdout)
    assert strip_pg(text) == bam_check.sam_header(want)
    assert lines == bam_check.sam_records(want), gap_cases.diff_message(lines, bam_check.sam_records(want))


ROUTE_CASES = gap_cases.SE_CASES + ["gap_pe_short"]
GAP_SLOTS = 16


@pytest.mark.parametrize("env", [{"SALT_GPU_GAP_SLOTS": str(GAP_SLOTS)}, {"SALT_GPU_NO_GAP_DEFER": "1"}, {"SALT_GPU_HEAVY_BIG": "1"},
                                 {"SALT_GPU_GAP_PER_CU": "1"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_gpu_gap_fixture_through_every_switched_shape(env, tmp_path):
    """(c) The single-end bands and the short-mate pairs with 16 k_gap slots (every other read of the lane band finds none and takes
    the overflow pass), without deferral (the gapped pass inside k_heavy), in k_heavy's all-in-one shape, and with one k_gap block per
    CU.  A leg is a fresh child process (the switches are read once), which aligns and writes the SAM bytes; the comparison is here."""
    child_env = {k: v for k, v in os.environ.items() if k not in ("SALT_GPU_GAP_SLOTS", "SALT_GPU_NO_GAP_DEFER", "SALT_GPU_HEAVY_BIG", "SALT_GPU_GAP_PER_CU")}
    child_env.update(env)
    try:
        p = subprocess.run([sys.executable, gap_cases.__file__, str(tmp_path)] + ROUTE_CASES, env=child_env, capture_output=True, text=True,
                           timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail("the child did not finish in %ds" % e.timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    counts = json.load(open(str(tmp_path / "counts.json")))
    print(env, counts)
    for case in ROUTE_CASES:
        got, want = open(str(tmp_path / (case + ".sam")), "rb").read(), gap_cases.golden(case)
        assert got == want, (case, gap_cases.diff_message(got, want))
    if "SALT_GPU_GAP_SLOTS" in env:
        # the lane band (L <= 129) and the short mates (k = 3, L <= 164) are the reads that ask for a slot: far more than there are
        for case in ("gap_se_lane", "gap_pe_short"):
            assert counts[case]["gap_slots_asked"] > 10 * GAP_SLOTS, counts
    if "SALT_GPU_NO_GAP_DEFER" in env:
        assert all(c["gap_slots_asked"] == 0 and c["gap_items"] == 0 for c in counts.values()), counts
    assert counts["gap_se_lane"]["heavy_reads"] >= gap_cases.MINIMA["gap_se_lane"][1]


@pytest.fixture(scope="module")
def repeat(tmp_path_factory, oracle_cli):
    """The tandem-repeat genome of gap_cases.repeat_genome indexed by the product's builder, 400 indel reads from inside the block, the
    oracle's rows for them (default options; -m 5000 on the first 100) and, per read, the rows the oracle located."""
    from salt_amd import workload
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    tmp = tmp_path_factory.mktemp("repeat")
    genome, pos, mask = gap_cases.repeat_genome()
    fa, snp, prefix = str(tmp / "g.fa"), str(tmp / "s.txt"), str(tmp / "idx")
    workload.write_fasta(fa, "tandem", genome)
    workload.write_snps(snp, "tandem", genome, pos, mask)
    subprocess.run([SALT_IDX, "-k", "21", fa, snp, prefix], check=True, stderr=subprocess.DEVNULL, timeout=600)
    seqs, offs = gap_cases.repeat_reads(genome, 400, seed=3)
    ora = oracle_py.Oracle(prefix)
    want = ora.align(ora.opt(), seqs, offs, n_threads=8)
    want_m = ora.align(ora.opt(max_locate=5000), seqs[:offs[100]], offs[:101], n_threads=8)
    rows = np.zeros(400, dtype=np.int64)
    for i in range(400):
        _, c = ora.align(ora.opt(), seqs[offs[i]:offs[i + 1]], np.array([0, offs[i + 1] - offs[i]], dtype=np.uint32), counters=True)
        rows[i] = c["n_saC"] + c["n_saR"]
    ora.close()
    # what the reads are for, on the oracle's rows alone
    assert int((want["is_gap"] == 1).sum()) >= 200
    assert int((want["n_hits"].sum(axis=1) >= 2).sum()) >= 100
    assert int((rows > 128).sum()) >= 50                      # more than 128 located rows in all: more than 64 on one strand at the least
    fq = str(tmp / "reads.fq")
    workload.write_fastq(fq, seqs, offs)
    want_sam = subprocess.run([os.path.join(ROOT, "oracle", "salt_oracle"), "-d", "-c", prefix, fq], check=True, capture_output=True).stdout
    assert gap_cases.xa_gapped(want_sam) >= 50                # records whose XA list has a hit with an I or D in its own CIGAR
    return prefix, seqs, offs, want, want_m, fq, want_sam


@pytest.mark.parametrize("slots", [None, 4], ids=["default", "gap_slots_4"])
def test_gpu_gapped_reads_inside_a_tandem_repeat_equal_the_oracle(repeat, slots, monkeypatch):
    """(d) Indel reads of 100 / 129 / 130 / 164 bases inside 4 000 diverged copies of a 30-base unit: hundreds of located rows a strand
    (several k_gap chunks per strand, the strand bit of an item), XA lists of gapped hits; -m 5000 is above the LDS list and takes
    k_heavy_glob.  Once more with 4 k_gap slots, whose pool is too small for a read's rows at -m 5000 (the "pool exhausted" arm).
    Every field and CIGAR against the CPU oracle."""
    import salt_amd
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    prefix, seqs, offs, want, want_m, fq, want_sam = repeat
    if slots:
        monkeypatch.setenv("SALT_GPU_GAP_SLOTS", str(slots))
    idx = salt_amd.Index.reload(prefix)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1, max_bases=int(offs[-1]) + 64)
    try:
        opt, _ = salt_amd.AlnOpt.from_argv(["-d", "-c"], idx.l_seed)
        res = aln.alnse_core1(opt, seqs, offs)
        bad = oracle_py.compare(res, want)
        assert len(bad) == 0, (len(bad), bad[:10])
        names, fseqs, foffs, quals = salt_amd.read_fastq(fq)          # the alternative hits' own CIGARs: the XA lists of the SAM text
        got = salt_amd.sam_text(idx, opt, names, fseqs, foffs, quals, res)
        assert got == want_sam, gap_cases.diff_message(got, want_sam)
        opt, _ = salt_amd.AlnOpt.from_argv(["-m", "5000"], idx.l_seed)
        bad = oracle_py.compare(aln.alnse_core1(opt, seqs[:offs[100]], offs[:101]), want_m)
        assert len(bad) == 0, ("-m 5000", len(bad), bad[:10])
    finally:
        aln.close()
        idx.destroy()


def test_gpu_lv_units_match_reference_shape_vectors():
    """(e) mismatch_capped, lv_wave, lv_cigar and -- staged by lane_text, 64 different cases to the 64 lanes where the file has them --
    lv_lanes on the shape vectors: exact answers within the lane kernel's limits (LLV_K, LLV_TW), -2 beyond them."""
    n, n_lane = gap_cases.run_lv_units(os.path.join(GOLDEN, "lv_vectors_shapes.txt.gz"))
    assert n == 3000 and n_lane >= 1500
