"""The paired-end kernels on the designed fixture (tests/golden/make_pe_geometry_fixture.py; classes and census in tests/pe_geometry.py):
pairs at the exact edges of the insert window, same-strand and outward pairs, overlapping mates, rescue windows that clamp at base 0 and at
l_pac or are one column wide, windows across the contig boundary, cross-copy and chimeric pairs, clipped rescues, unmapped mates -- against
the SAM the real reference printed under two option rows, and field by field against the CPU oracle (which
tests/test_pe_geometry_golden.py pins on the same files).  k_pair, k_swf / k_swf1 / k_swr / k_swtb, k_pe_final, the paired-end SAM and BAM
formatters and the depth / SNP-count / error-profile hooks all see these pairs here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_check
import depth_check
import errprof_check as ec
import pe_geometry as pg
import snp_check
from bgzf_check import strip_pg
from conftest import LAMBDA, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "oracle"))
SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
ROW_NAMES = sorted(pg.ROWS)
FIELDS = ("pos", "strand", "n_diff", "is_gap", "mapq", "b0", "b1", "seq_start", "seq_end")


def _paths(files):
    return [os.path.join(LAMBDA, f) for f in files]


def _diff_report(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
    msg = "\n".join("line %d\n  got  %r\n  want %r" % (i, g[i][:400], w[i][:400]) for i in bad[:6])
    return "%d differing lines (of %d / %d)\n%s" % (len(bad), len(g), len(w), msg)


@pytest.fixture(scope="module")
def geom():
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=4096)
    reads = salt_amd.interleave_pairs(*[salt_amd.read_fastq(p) for p in pg.read_paths()])
    noref = salt_amd.interleave_pairs(*[salt_amd.read_fastq(p) for p in _paths(pg.NOREF)])
    yield salt_amd, idx, aln, reads, noref
    aln.close()
    idx.destroy()


def _opt(salt_amd, idx, row):
    opt, _ = salt_amd.AlnOpt.from_argv(list(pg.ROWS[row][0]), idx.l_seed)
    assert opt.paired and (opt.min_tlen, opt.max_tlen) == pg.ROWS[row][1:]
    return opt


@pytest.fixture(scope="module")
def oracle_rows(geom):
    """row -> (oracle rows of the fixture, of the noref pairs): computed once, shared, never written to."""
    import oracle_py
    salt_amd, idx, _, (_, seqs, offs, _), (_, nseqs, noffs, _) = geom
    ora = oracle_py.Oracle(os.path.join(LAMBDA, "idx"))
    out = {}
    for row in pg.ROWS:
        opt = _opt(salt_amd, idx, row)
        oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
        out[row] = (ora.align_pe(oo, seqs, offs, opt.min_tlen, opt.max_tlen, n_threads=16), ora.align_pe(oo, nseqs, noffs, opt.min_tlen, opt.max_tlen, n_threads=4))
    ora.close()
    return out


@pytest.mark.parametrize("max_reads", [4096, 64], ids=["one_batch", "batches_of_64_mates"])
@pytest.mark.parametrize("row", ROW_NAMES)
def test_alnpe_core1_and_the_host_formatter_give_the_reference_sam(row, max_reads, geom):
    """(a) every pair of the fixture through alnpe_core1 and sam_text_pe: the reference's SAM byte for byte.  With a workspace of 64 mates the
    rescue requests get their queue bases in many small batches (k_pair's atomicAdd on a counter that starts at 0 twenty times)."""
    salt_amd, idx, aln, (names, seqs, offs, quals), _ = geom
    opt = _opt(salt_amd, idx, row)
    small = salt_amd.GpuAligner(idx, device=0, max_reads=max_reads) if max_reads != aln.max_reads else aln
    try:
        res = small.alnpe_core1(opt, idx, seqs, offs)
        assert small.pe_counts()[4] == 0
    finally:
        if small is not aln:
            small.close()
    got, want = salt_amd.sam_text_pe(idx, opt, names, seqs, offs, quals, res), pg.golden(row)
    if got != want:
        pytest.fail(_diff_report(got, want))


@pytest.fixture(scope="module")
def plain_reads(tmp_path_factory):
    return pg.plain_reads(tmp_path_factory.mktemp("geomfq"))


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("lamidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True, stderr=subprocess.DEVNULL,
                   timeout=600)
    return prefix


@pytest.mark.parametrize("row", ROW_NAMES)
def test_cli_text_path_and_host_pipeline_give_the_reference_sam(row, lambda_cli_index, plain_reads):
    """(b) `salt -p`: device formatters (k_sam_*) with chunks of ~13 pairs and with one chunk, and the host pipeline."""
    want = pg.golden(row)
    for env in (dict(os.environ, SALT_CHUNK_BYTES="4000"), dict(os.environ, SALT_CHUNK_BYTES="250000"), dict(os.environ, SALT_HOST_PIPELINE="1")):
        out = subprocess.run([SALT] + pg.ROWS[row][0] + ["-t", "8", lambda_cli_index] + plain_reads, capture_output=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-400:]
        assert strip_pg(out.stdout) == want, (row, env.get("SALT_CHUNK_BYTES"), _diff_report(strip_pg(out.stdout), want))
        assert (b"text path (paired end)" in out.stderr) == ("SALT_HOST_PIPELINE" not in env)


@pytest.mark.parametrize("row", ROW_NAMES)
def test_cli_bam_decodes_to_the_golden(row, lambda_cli_index, plain_reads, geom):
    """(c) `salt -p --bam` (k_bam_*): the stream decodes to the golden's records, its record bytes are the host encoder's over the golden, and
    the records at POS 1 and on the genome's last base carry the golden's FLAG, RNEXT, PNEXT and TLEN and the bin of their interval."""
    salt_amd, idx, _, _, _ = geom
    want = pg.golden(row)
    out = subprocess.run([SALT] + pg.ROWS[row][0] + ["--bam", lambda_cli_index] + plain_reads, capture_output=True, env=dict(os.environ), timeout=300)
    assert out.returncode == 0, out.stderr[-600:]
    assert b"text path" in out.stderr and b"[salt] BAM output: device records, " in out.stderr, out.stderr[-600:]
    text, lines, recs = bam_check.decode_stream(out.stdout)
    assert strip_pg(text) == bam_check.sam_header(want) and lines == bam_check.sam_records(want)
    assert b"".join(r["bytes"] for r in recs) == salt_amd.bam_from_sam(idx, bam_check.sam_records(want))
    glines = [l.split(b"\t") for l in bam_check.sam_records(want).split(b"\n") if l]
    assert len(glines) == len(recs)
    names = [b"lambdaA", b"lambdaB_div2pct"]
    n_first = n_last = 0
    for g, r in zip(glines, recs):
        if int(g[1]) & 4:
            continue
        span = pg.ref_span(g[5].decode())
        first, last = g[2] == names[0] and g[3] == b"1", g[2] == names[1] and int(g[3]) - 1 + span == pg.LEN_B
        if not (first or last):
            continue
        n_first, n_last = n_first + first, n_last + last
        assert (r["ref_id"], r["pos"]) == ((0, 0) if first else (1, pg.LEN_B - span))
        assert r["flag"] == int(g[1]) and r["tlen"] == int(g[8]) and r["next_pos"] == int(g[7]) - 1
        assert r["next_ref"] == (-1 if g[6] == b"*" else r["ref_id"] if g[6] == b"=" else names.index(g[6]))
        assert r["bin"] == bam_check.reg2bin(r["pos"], r["pos"] + span)
    assert n_first >= 2 * pg.MIN_PER_ORDER and n_last >= 2 * pg.MIN_PER_ORDER, (n_first, n_last)


def _bad_rows(res, want):
    import oracle_py
    bad = oracle_py.compare(res, want, pe=True)
    return len(bad), [(int(i), [(f, res[f][i].tolist(), want[f][i].tolist()) for f in FIELDS]) for i in bad[:4]]


@pytest.mark.parametrize("row", ROW_NAMES)
def test_every_field_of_both_mates_equals_the_oracle(row, geom, oracle_rows):
    """(d) pos, strand, n_diff, is_gap, mapq, SW scores, soft clips, alternative hits and CIGAR of every mate against the oracle; no rescue
    overflowed.  Then the rescue windows: the pairs of the classes in pe_geometry.WINDOWS_OF_CLASS alone -- a random mate is unmapped and a
    designed damaged mate is unmapped on its own (the generator kept only such damage), so each of these pairs reaches pairing_singleton with
    one mapped mate, for which k_pair queues exactly one window, and a pair of two random mates queues none.  pe_counts()[0] of that batch must
    be the sum of the table's entries.  (Pairs of two clean mates queue none or two, depending on their alternative hits: not counted here.)"""
    salt_amd, idx, aln, (names, seqs, offs, _), _ = geom
    opt = _opt(salt_amd, idx, row)
    res = aln.alnpe_core1(opt, idx, seqs, offs)
    pc = aln.pe_counts()
    n_bad, detail = _bad_rows(res, oracle_rows[row][0])
    assert n_bad == 0, (n_bad, detail)
    assert pc[4] == 0 and pc[0] > 0, pc
    table = pg.class_table()
    keep = [p for p in range(len(names) // 2) if table[names[2 * p].decode()][0] in pg.WINDOWS_OF_CLASS]
    expect = sum(pg.WINDOWS_OF_CLASS[table[names[2 * p].decode()][0]] for p in keep)
    assert len(keep) >= 150 and 0 < expect < len(keep)
    pieces = [seqs[offs[2 * p]:offs[2 * p + 2]] for p in keep]
    lens = np.array([int(offs[m + 1] - offs[m]) for p in keep for m in (2 * p, 2 * p + 1)], dtype=np.uint32)
    sub_offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    sub = aln.alnpe_core1(opt, idx, np.concatenate(pieces), sub_offs)
    pc = aln.pe_counts()
    rows = np.array([m for p in keep for m in (2 * p, 2 * p + 1)])
    assert _bad_rows(sub, oracle_rows[row][0][rows])[0] == 0
    assert pc[0] == expect and pc[4] == 0, (pc, expect)


@pytest.mark.parametrize("row", ROW_NAMES)
def test_pairs_the_reference_exits_on_equal_the_oracle(row, geom, oracle_rows):
    """(e) a clean forward mate within min_isize + L of the genome's end whose mate maps elsewhere: the both-mapped rescue window starts at or
    past l_pac.  The reference exits there (alnpe.c:266); the oracle refuses the window and goes on, and so do the kernels (`sane`): the call
    succeeds, nothing overflows, every field equals the oracle's."""
    salt_amd, idx, aln, _, (names, seqs, offs, _) = geom
    assert len(names) >= 4 * pg.MIN_PER_ORDER
    opt = _opt(salt_amd, idx, row)
    res = aln.alnpe_core1(opt, idx, seqs, offs)                  # raises SaltError unless the library returned SALT_OK
    pc = aln.pe_counts()
    want = oracle_rows[row][1]
    n_bad, detail = _bad_rows(res, want)
    assert n_bad == 0, (n_bad, detail)
    assert pc[4] == 0 and pc[0] == 2 * (len(names) // 2), pc     # both mates map, none pairs: two windows each
    past = sum(1 for p in range(len(names) // 2) for m in (2 * p, 2 * p + 1)
               if want["strand"][m] == 0 and int(want["pos"][m]) + max(opt.min_tlen, 200) - 200 + 100 >= pg.L_PAC)
    assert past >= (2 * pg.MIN_PER_ORDER if row == "a350" else 2), past


def test_depth_snp_counts_and_error_profile_equal_their_twins_over_the_golden(geom, plain_reads):
    """(f) one paired-end text call under row a350 with all three hooks on: its SAM is the golden's records, and each table equals the host
    twin and the Python statement over the golden.  Soft-clipped rescued rows and rows ending on the genome's last base are where the hooks
    cut their runs."""
    salt_amd, idx, _, _, _ = geom
    golden = pg.golden("a350")
    recs = bam_check.sam_records(golden)
    assert snp_check.census(golden)[1] >= 40 and snp_check.census(golden)[0] >= 40
    fq1, fq2 = (open(p, "rb").read() for p in plain_reads)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=4096)
    try:
        aln.set_contigs(idx)
        aln.depth_enable(True, 0)
        aln.depth_reset()
        aln.snp_enable(True, 0)
        aln.snp_counts(reset=True)
        aln.errprof_enable(True, 0)
        aln.errprof_table(reset=True)
        sam, n = aln.align_pe_text(_opt(salt_amd, idx, "a350"), idx, fq1, fq2)
        diff, counts, (E, R) = aln.depth_fetch(0, pg.L_PAC + 1), aln.snp_counts(), aln.errprof_table()
    finally:
        aln.close()
    assert bam_check.sam_records(sam) == recs and n == len(pg.records(golden))
    want = salt_amd.depth_add_sam(idx, golden, 0)[0]
    assert np.array_equal(want, depth_check.diff_of_sam(depth_check.lambda_contigs(), golden, 0)[0]) and want.any()
    assert np.array_equal(diff, want), np.flatnonzero(diff != want)[:8]
    sites, _ = snp_check.sites_of_ref(os.path.join(LAMBDA, "idx.ref"))
    want = salt_amd.snp_count_sam(idx, golden, 0)
    assert np.array_equal(want, snp_check.count_sam(sites, snp_check.contig_offsets(os.path.join(LAMBDA, "idx.C.ann")), golden, 0)[0]) and want.sum() > 0
    assert np.array_equal(counts, want), np.flatnonzero((counts != want).any(axis=1))[:8]
    tE, tR, _ = salt_amd.errprof_add_sam(idx, golden, 0)
    mE, mR, _ = ec.tables_of_sam(ec.lambda_masks(), ec.lambda_offsets(), golden, 0)
    assert np.array_equal(tE, mE) and np.array_equal(tR, mR) and tE[0].any() and tE[1].any()
    assert not R[:, 1].any() and not R[:, 7].any() and np.array_equal(R, tR), (R.tolist(), tR.tolist())
    assert np.array_equal(E, tE), np.argwhere(E != tE)[:4].tolist()
