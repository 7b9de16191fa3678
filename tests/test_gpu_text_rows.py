"""The text kernels of salt_amd/csrc/salt_text.hip -- the FASTQ scan, k_pack's records as k_sam_len reads them, k_sam_len / k_sam_write and
k_bam_len / k_bam_write -- on result rows built in tests/text_rows.py and handed over by GpuAligner.text_from_rows / text_from_rows_pe
(salt_gpu_diag_text_rows): every code path the aligner's own rows reach only by luck.  Expected bytes: the host twins (Index.samse /
Index.sampe per record, salt_amd.bam_from_sam of that text; for the scan blocks the line written out from the Python parse).  Every
comparison is byte for byte; tests/test_text_rows_model.py counts, on the CPU, that every class of record is among the cases."""
import numpy as np
import pytest

import bgzf_check
import text_rows as tr

pytestmark = pytest.mark.gpu

BAM_BLOCKS = [n for n in tr.ROW_BLOCKS + tr.SCAN_BLOCKS if n not in tr.SAM_ONLY]


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp("built") / "idx")
    tr.build_index(prefix)
    out = {"dense": tr.dense_ref(), "built": tr.Ref(prefix)}
    yield out
    for r in out.values():
        r.ix.destroy()


@pytest.fixture(scope="module")
def aligners(refs):
    import salt_amd
    out = {}
    for name, ref in refs.items():
        aln = salt_amd.GpuAligner(ref.ix, device=0, max_reads=tr.MAX_READS)
        aln.set_contigs(ref.ix)
        aln.set_pac(ref.ix)
        out[name] = aln
    yield out
    for aln in out.values():
        aln.close()


@pytest.fixture(scope="module")
def cases(refs):
    """name -> (block, expected SAM): built once, left unchanged"""
    return {b.name: (b, tr.expected_sam(refs[b.ref], b)) for b in tr.all_blocks(refs["dense"], refs["built"])}


def device(aln, ref, blk, rows=None):
    rows = blk.rows if rows is None else rows
    if blk.paired:
        return aln.text_from_rows_pe(blk.opt(ref), ref.ix, blk.fq1, blk.fq2, rows)
    return aln.text_from_rows(blk.opt(ref), blk.fq1, rows)


def bam_records(b):
    out, at = [], 0
    while at + 4 <= len(b):
        n = 4 + int.from_bytes(b[at:at + 4], "little")
        out.append(b[at:at + n])
        at += n
    return out


def same(got, want, blk, split):
    if got == want:
        return
    g, w = split(got), split(want)
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            pytest.fail("%s: record %d of %d differs\n got %r\nwant %r" % (blk.name, i, len(w), a[:1500], b[:1500]))
    pytest.fail("%s: %d records for %d (%d bytes for %d)" % (blk.name, len(g), len(w), len(got), len(want)))


def sam_lines(blk):
    return lambda text: text.split(b"\n\n" if blk.paired else b"\n")


@pytest.mark.parametrize("name", tr.ROW_BLOCKS + tr.SCAN_BLOCKS)
def test_sam(name, cases, refs, aligners):
    blk, want = cases[name]
    got, n = device(aligners[blk.ref], refs[blk.ref], blk)
    assert n == len(blk.rows)
    same(got, want, blk, sam_lines(blk))


@pytest.mark.parametrize("name", BAM_BLOCKS)
def test_bam(name, cases, refs, aligners):
    blk, sam = cases[name]
    want = tr.expected_bam(refs[blk.ref], sam)
    aln = aligners[blk.ref]
    aln.set_sam_bam(True)
    try:
        got, n = device(aln, refs[blk.ref], blk)
    finally:
        aln.set_sam_bam(False)
    assert n == len(blk.rows)
    same(got, want, blk, bam_records)


@pytest.mark.parametrize("name", tr.SAM_ONLY)
def test_bam_refuses_a_name_of_more_than_254_bytes(name, cases, refs, aligners):
    import salt_amd
    blk, sam = cases[name]
    aln = aligners[blk.ref]
    aln.set_sam_bam(True)
    try:
        with pytest.raises(salt_amd.SaltError, match="BAM: a read name in this block is longer than 254 bytes"):
            device(aln, refs[blk.ref], blk)
    finally:
        aln.set_sam_bam(False)
    same(device(aln, refs[blk.ref], blk)[0], sam, blk, sam_lines(blk))


@pytest.mark.parametrize("name,bam", [("md_words_se_0", False), ("pe_matrix", True)])
def test_bgzf_members_inflate_to_the_same_bytes(name, bam, cases, refs, aligners):
    blk, sam = cases[name]
    want = tr.expected_bam(refs[blk.ref], sam) if bam else sam
    aln = aligners[blk.ref]
    aln.set_sam_bgzf(True)
    aln.set_sam_bam(bam)
    try:
        got, n = device(aln, refs[blk.ref], blk)
    finally:
        aln.set_sam_bam(False)
        aln.set_sam_bgzf(False)
    assert n == len(blk.rows) and len(got) < len(want)
    same(b"".join(t for _, t in bgzf_check.members(got)), want, blk, bam_records if bam else sam_lines(blk))


# ---- the host checks in front of the kernels ----
def small_block(ref, paired):
    b = tr.Block("refusals", "dense", paired=paired)
    for k, (pos, strand) in enumerate(((10, 0), (200, 1), (2950, 0), (77, 1))):
        cig = tr.ops(("M", 20), ("I", 2), ("M", 10), ("D", 3), ("M", 8))
        hits = [(0, 5, 1, None), (1, 2999, 2, tr.ops(("M", 40)))]

        def setter(rows, i, pos=pos, strand=strand, cig=cig, hits=hits):
            tr.set_mapped(rows, i, pos, strand, cig, seq_start=3)
            tr.set_hits(rows, i, hits)
        b.add_read(tr.aligned_read(ref, pos, cig, (4,), True, 3, 2, salt=k), strand, setter)
    return b.finish()


def spoil(rows, i, field, value, sub=None):
    rows = rows.copy()
    if sub is None:
        rows[i][field] = value
    else:
        rows[i][field][sub] = value
    return rows


# read length 45 = 3 + (20 + 2 + 10 + 8) + 2; on the genome 41; row 2 lies at 2950, ref_len = 3000
REFUSALS = {
    "n_cigar": (lambda r: spoil(r, 1, "n_cigar", 65), "row 1: n_cigar is more than SALT_MAX_CIGAR_OPS"),
    "n_hits": (lambda r: spoil(r, 3, "n_hits", 5, 0), "row 3: n_hits[0] + n_hits[1] = 6 is more than SALT_MAX_HITS"),
    "n_hits_unmapped": (lambda r: spoil(spoil(r, 2, "pos", tr.UNMAPPED), 2, "n_hits", 200, 1), "row 2: n_hits[0] + n_hits[1] = 201 is more than SALT_MAX_HITS"),
    "hit_n_cigar": (lambda r: spoil(r, 0, "hit_n_cigar", 65, 1), "row 0: hit_n_cigar[1] is more than SALT_MAX_CIGAR_OPS"),
    "pos": (lambda r: spoil(r, 2, "pos", 3000), "row 2: pos lies beyond the genome"),
    "hit_pos": (lambda r: spoil(r, 1, "hits", (3000, 0, 0, 1), (1, 0)), "row 1: the pos of hit 1 lies beyond the genome"),
    "pos_plus_cigar": (lambda r: spoil(r, 2, "pos", 2960), "row 2: pos + the CIGAR's M and D operations end beyond the genome"),
    "seq_start_plus_cigar": (lambda r: spoil(r, 0, "seq_start", 6), "row 0: seq_start + the CIGAR's M and I operations end beyond the read"),
    "seq_end": (lambda r: spoil(r, 3, "seq_end", 45), "row 3: seq_end lies beyond the read"),
    "n_rows": (lambda r: r[:3], None),
}


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_rows_the_host_refuses(what, paired, refs, aligners):
    import salt_amd
    ref, aln = refs["dense"], aligners["dense"]
    blk = small_block(ref, paired)
    want = tr.expected_sam(ref, blk)
    bad, message = REFUSALS[what]
    if message is None:
        message = "%d rows for 4 parsed records" % len(bad(blk.rows))
    with pytest.raises(salt_amd.SaltError) as e:
        device(aln, ref, blk, bad(blk.rows))
    assert str(e.value).endswith("salt_gpu error -1: text rows: " + message), str(e.value)
    assert device(aln, ref, blk) == (want, 4)
    aln.set_sam_bam(True)
    try:
        with pytest.raises(salt_amd.SaltError):
            device(aln, ref, blk, bad(blk.rows))
        assert device(aln, ref, blk) == (tr.expected_bam(ref, want), 4)
    finally:
        aln.set_sam_bam(False)


SKIPPED_AND = {
    "pos": (lambda r: spoil(r, 2, "pos", 3000), "row 2: pos lies beyond the genome"),
    "pos_plus_cigar": (lambda r: spoil(r, 2, "pos", 2960), "row 2: pos + the CIGAR's M and D operations end beyond the genome"),
    "seq_start_plus_cigar": (lambda r: spoil(r, 2, "seq_start", 6), "row 2: seq_start + the CIGAR's M and I operations end beyond the read"),
    "n_cigar": (lambda r: spoil(r, 2, "n_cigar", 255), "row 2: n_cigar is more than SALT_MAX_CIGAR_OPS"),
}


@pytest.mark.parametrize("what", sorted(SKIPPED_AND))
def test_skipped_excuses_a_row_of_a_single_read_only(what, refs, aligners):
    """the paired-end kernels never read `skipped`: a mate's row is checked whatever it says; a single read's gives an empty line"""
    import salt_amd
    ref, aln = refs["dense"], aligners["dense"]
    bad, message = SKIPPED_AND[what]
    pe = small_block(ref, True)
    with pytest.raises(salt_amd.SaltError) as e:
        device(aln, ref, pe, bad(spoil(pe.rows, 2, "skipped", 1)))
    assert str(e.value).endswith("salt_gpu error -1: text rows: " + message), str(e.value)
    assert device(aln, ref, pe) == (tr.expected_sam(ref, pe), 4)
    se = small_block(ref, False)
    rows = bad(spoil(se.rows, 2, "skipped", 1))
    se.rows = rows
    want = tr.expected_sam(ref, se)
    assert want.split(b"\n")[2] == b"" and device(aln, ref, se) == (want, 4)


def test_a_read_of_513_bases_and_polish_are_refused(refs, aligners):
    import salt_amd
    ref, aln = refs["dense"], aligners["dense"]
    blk = small_block(ref, False)
    long_one = tr.Block("too_long", "dense")
    long_one.add_read(tr.aligned_read(ref, 0, tr.ops(("M", 513))), 0, None)
    long_one.add_read(tr.aligned_read(ref, 0, tr.ops(("M", 512))), 0, None)
    long_one.finish()
    with pytest.raises(salt_amd.SaltError, match=r"read longer than SALT_MAX_READ_LEN \(512\)"):
        device(aln, ref, long_one)
    ws = aln.fork()
    try:
        ws.set_polish("lv")
        with pytest.raises(salt_amd.SaltError, match="text rows: the polish stage is not driven from rows"):
            device(ws, ref, blk)
        ws.set_polish(0)
        assert device(ws, ref, blk) == (tr.expected_sam(ref, blk), 4)
    finally:
        ws.close()
    assert device(aln, ref, blk) == (tr.expected_sam(ref, blk), 4)


def test_the_production_entry_gives_the_rows_text(refs, aligners):
    """both ways through the shared stages on one workspace: reads the aligner places itself, then the same rows handed back in"""
    ref, aln = refs["dense"], aligners["dense"]
    blk = tr.Block("aligned", "dense")
    for k in range(64):
        L, strand = 60 + k, k & 1
        pos = (k * 43) % (ref.ref_len - L)
        blk.add_read(tr.aligned_read(ref, pos, tr.ops(("M", L)), (7,) if k % 3 else (), True, salt=k), strand, None)
    blk.finish()
    opt = blk.opt(ref)
    sam, n = aln.align_se_text(opt, blk.fq1)
    assert n == 64
    codes = [c for _, c, _ in blk.reads()]
    seqs, offs = np.concatenate(codes), np.cumsum([0] + [len(c) for c in codes]).astype(np.uint32)
    rows = aln.alnse_core1(opt, seqs, offs)
    assert int((rows["pos"] != tr.UNMAPPED).sum()) >= 32
    assert aln.text_from_rows(opt, blk.fq1, rows) == (sam, 64)
