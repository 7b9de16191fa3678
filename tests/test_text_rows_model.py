"""The case sets of tests/text_rows.py, on the CPU: every block builds, the Python statement of the FASTQ rules agrees with
salt_amd.read_fastq on the scan blocks, and the census finds every class of record the text kernels treat differently -- counted from
the expected bytes, the rows and the blocks, so that a builder that goes empty fails here and not silently on the GPU."""
import numpy as np
import pytest

import text_rows as tr


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp("built") / "idx")
    seconds = tr.build_index(prefix)
    print("built index: %.2f s" % seconds)
    out = {"dense": tr.dense_ref(), "built": tr.Ref(prefix)}
    yield out
    for r in out.values():
        r.ix.destroy()


def test_built_index_is_the_one_the_cases_assume(refs):
    b = refs["built"]
    assert [(ln, nm.decode()) for _, ln, nm in b.contigs] == list(zip(tr.LENS, tr.NAMES))
    assert b.ref_len == sum(tr.LENS) and [o for o, _, _ in b.contigs] == [0, tr.LENS[0], tr.LENS[0] + tr.LENS[1]]
    assert (np.concatenate([tr.CODE[g] for g in tr.built_genome()]) == b.base).all()
    sites = np.nonzero(b.mask & (b.mask - 1))[0]
    assert len(sites) == 16 and ((b.mask >> b.base) & 1).all()
    d = refs["dense"]
    assert d.ref_len == 3000 and len(d.contigs) == 1 and int(((d.mask & (d.mask - 1)) != 0).sum()) == 434
    assert len(tr.densest_window(d)[1]) == 93


def test_python_parser_agrees_with_read_fastq_on_the_scan_blocks(tmp_path):
    import salt_amd
    for blk in tr.scan_blocks():
        for k, text in enumerate((blk.fq1, blk.fq2) if blk.paired else (blk.fq1,)):
            path = str(tmp_path / ("%s_%d.fq" % (blk.name, k)))
            with open(path, "wb") as f:
                f.write(text)
            names, seqs, offs, quals = salt_amd.read_fastq(path)
            mine = tr.fq_parse(text)
            assert names == [m[0] for m in mine], blk.name
            assert quals == [m[2] for m in mine], blk.name
            assert np.array_equal(seqs, np.concatenate([m[1] for m in mine])) and list(np.diff(offs)) == [len(m[1]) for m in mine], blk.name


def test_every_block_builds_and_the_census_is_complete(refs):
    blocks = tr.all_blocks(refs["dense"], refs["built"])
    assert sorted(b.name for b in blocks) == sorted(tr.ROW_BLOCKS + tr.SCAN_BLOCKS) and len({b.name for b in blocks}) == len(blocks)
    assert sorted(b.name for b in blocks if not tr.bam_able(b)) == sorted(tr.SAM_ONLY)
    pairs = []
    for blk in blocks:
        assert len(blk.rows) <= tr.MAX_READS, blk.name
        sam = tr.expected_sam(refs[blk.ref], blk)
        pairs.append((blk, sam))
        if tr.bam_able(blk):
            bam = tr.expected_bam(refs[blk.ref], sam)
            n_rec = sum(1 for l in sam.split(b"\n") if l)
            at, n = 0, 0
            while at < len(bam):
                at += 4 + int.from_bytes(bam[at:at + 4], "little")
                n += 1
            assert at == len(bam) and n == n_rec, blk.name
    tr.census_check(tr.census(refs, pairs))
