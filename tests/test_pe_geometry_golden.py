"""The designed paired-end fixture (tests/golden/make_pe_geometry_fixture.py, tests/pe_geometry.py) without a GPU: the CPU oracle and the
host formatter twin against the SAM the real reference printed for it, the census of that SAM re-asserted from the committed files, and
the integer MAPQ form against the reference's double expression.  tests/test_gpu_pe_geometry.py holds the device side."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pe_geometry as pg
from conftest import LAMBDA, ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))


def _paths(files):
    return [os.path.join(LAMBDA, f) for f in files]


@pytest.mark.parametrize("row", sorted(pg.ROWS))
def test_oracle_pe_sam_matches_reference_on_the_geometry_fixture(row, oracle_cli, tmp_path):
    """The checker of the GPU field tests on these classes: window edges, same-strand and outward pairs, overlaps, rescue windows clamped at
    base 0 and at l_pac, windows across the contig boundary, cross-copy and chimeric pairs, clipped rescues, unmapped mates."""
    out = subprocess.run([oracle_cli] + pg.ROWS[row][0] + [os.path.join(LAMBDA, "idx")] + pg.plain_reads(tmp_path), check=True, capture_output=True).stdout
    want = pg.golden(row)
    if out != want:
        g, w = out.split(b"\n"), want.split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        pytest.fail("%d differing lines; first: %r / %r" % (len(bad), g[bad[0]][:300], w[bad[0]][:300]))


def _cigar_ops(text):
    return [(int(n) << 4) | "MID".index(op) for n, op in re.findall(r"(\d+)([MID])", text)]


def rows_from_oracle(salt_amd, want, golden_rows):
    """Oracle rows as salt_result_t rows.  The oracle's rows do not carry the CIGARs of gapped alternative hits (its own formatter derives
    them); those, and only those, are read from the XA field of the golden record, in the order put_xa prints them."""
    res = np.zeros(len(want), dtype=salt_amd.RESULT_DTYPE)
    for f in ("pos", "strand", "n_diff", "is_gap", "mapq", "b0", "b1", "n_hits"):
        res[f] = want[f]
    res["seq_start"] = want["seq_start"].astype(np.uint16)          # whatever an unmapped row holds there is never printed
    res["seq_end"] = want["seq_end"].astype(np.uint16)
    for f in ("pos", "n_diff", "is_gap", "strand"):
        res["hits"][f] = want["hits"][f]
    for i in range(len(want)):
        ops = _cigar_ops(want["cigar"][i].decode()) if want["pos"][i] != 0xFFFFFFFF else []
        res["n_cigar"][i] = len(ops)
        res["cigar"][i, :len(ops)] = ops
        xa = [t for t in golden_rows[i][11:] if t.startswith("XA:Z:")]
        entries = xa[0][5:].rstrip(";").split(";") if xa else []
        h = k = 0
        for s in range(2):
            for j in range(int(want["n_hits"][i, s])):
                hit = want["hits"][i, s, j]
                if hit["pos"] != want["pos"][i]:
                    if hit["is_gap"]:
                        ops = _cigar_ops(entries[k].split(",")[2])
                        res["hit_n_cigar"][i, h] = len(ops)
                        res["hit_cigar"][i, h, :len(ops)] = ops
                    k += 1
                h += 1
    return res


@pytest.mark.parametrize("row", sorted(pg.ROWS))
def test_host_formatter_gives_the_golden_from_the_oracle_rows(row, oracle_lib):
    """salt_sam_pe (salt_host.cc), the twin of the device formatters: TLEN from q[1].seq_start in both arms, the proper bit from TLEN alone,
    the REVERSE bit of an unmapped mate, RNEXT '=' or a contig name, the sign of TLEN by >=."""
    import oracle_py
    import salt_amd
    args, lo, hi = pg.ROWS[row]
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    try:
        names, seqs, offs, quals = salt_amd.interleave_pairs(*[salt_amd.read_fastq(p) for p in pg.read_paths()])
        opt, _ = salt_amd.AlnOpt.from_argv(list(args), idx.l_seed)
        ora = oracle_py.Oracle(os.path.join(LAMBDA, "idx"))
        oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
        want = ora.align_pe(oo, seqs, offs, lo, hi, n_threads=8)
        ora.close()
        golden = pg.golden(row)
        grows = [r for _, r1, r2 in pg.records(golden) for r in (r1, r2)]
        got = salt_amd.sam_text_pe(idx, opt, names, seqs, offs, quals, rows_from_oracle(salt_amd, want, grows))
    finally:
        idx.destroy()
    assert got == golden


@pytest.mark.parametrize("row", sorted(pg.ROWS))
def test_host_bam_encoder_decodes_to_the_golden(row):
    """salt_bam_from_sam, the checker of the GPU test of `--bam` on this fixture: its records decode (tests/bam_check.py, which checks each
    bin against reg2bin) to the golden's lines, the rows at POS 1 and on the genome's last base among them."""
    import bam_check
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    try:
        want = bam_check.sam_records(pg.golden(row))
        refs = [(nm, ln) for _, ln, nm in idx.contigs()]
        assert bam_check.decode_records(salt_amd.bam_from_sam(idx, want), refs) == want
    finally:
        idx.destroy()


def test_census_of_the_committed_geometry_fixture():
    """Every property the classes are designed for is shown by at least 4 pairs in either file order, under the row it belongs to: an
    edited fixture cannot lose a class unnoticed.  The FASTQ files, the class table and both goldens list the same pairs."""
    table = pg.class_table()
    import salt_amd
    n1 = salt_amd.read_fastq(pg.read_paths()[0])[0]
    nr = salt_amd.read_fastq(_paths(pg.NOREF)[0])[0]
    assert [n.decode() for n in n1 + nr] == list(table)
    assert all(table[n.decode()][0].startswith("noref_") for n in nr) and not any(table[n.decode()][0].startswith("noref_") for n in n1)
    assert len(nr) >= 2 * pg.MIN_PER_ORDER and 300 <= len(n1) <= 650
    for row in pg.ROWS:
        sam = pg.golden(row)
        assert [name for name, _, _ in pg.records(sam)] == [n.decode() for n in n1]
        pg.check_census(sam, table, row)
        assert not any(l.startswith(b"@PG") for l in sam.split(b"\n"))
    counts = pg.class_counts(pg.golden("a350"), table)
    assert all(counts[c] >= 2 * pg.MIN_PER_ORDER for c in pg.WINDOWS_OF_CLASS), counts
    for f in [f + ".gz" for f in pg.READS] + pg.NOREF + [pg.CLASSES] + ["expect_pe_geom_%s.sam.gz" % r for r in pg.ROWS]:
        assert os.path.getsize(os.path.join(LAMBDA, f)) < 600_000, f


def test_integer_mapq_equals_the_double_expression():
    """gen_mapq (query.c:270-281): (uint32_t)(255.0 * ((double)|b0 - b1| / (double)b0)), capped at 254, against the integer form the
    kernels use, min(254, 255 * |b0 - b1| // b0), for every b0 in 1..4096 and every b1 in 0..4096 or equal to 100000 (the 'no second best'
    value of the gap-free path); b0 == 0 gives 0.  4096 covers the Smith-Waterman scores of 512-base mates (k_pe_final)."""
    b0 = np.arange(1, 4097, dtype=np.int64)[:, None]
    b1 = np.concatenate([np.arange(0, 4097, dtype=np.int64), [100000]])[None, :]
    d = np.abs(b0 - b1)
    integer = np.minimum(254, 255 * d // b0)
    double = np.minimum(254, (255.0 * (d.astype(np.float64) / b0.astype(np.float64))).astype(np.uint32).astype(np.int64))
    assert int((integer != double).sum()) == 0
    assert integer.min() == 0 and integer.max() == 254 and (integer[:, -1] == 254).all()
