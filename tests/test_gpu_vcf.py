"""The device's VCF parser (salt_amd/csrc/salt_vcf.hip behind salt_amd.vcf_snps(gpu_device=0)) against its host twin, which
test_vcf_host.py holds against the Python statement of the rule: the built texts of the five fixtures and the edge list, chunk cuts, the
borders of the line finder's and the compaction's tiles, the malformed-line number across chunks, and one `salt-idx --gpu --vcf` run."""
import os
import subprocess

import numpy as np
import pytest

import vcf_check as vc
from conftest import LAMBDA
from vcf_check import SALT_IDX, SEED_LEN, same_index

pytestmark = pytest.mark.gpu
EDGES = vc.edge_texts()
TILE = 1024                     # positions per compaction tile (salt_vcf.hip), bytes per tile of the line finder (salt_text.hip)


def host(contigs, text, **kw):
    import salt_amd
    return salt_amd.vcf_snps(vc.api_contigs(contigs), text, **kw)


def gpu(contigs, text, **kw):
    import salt_amd
    return salt_amd.vcf_snps(vc.api_contigs(contigs), text, gpu_device=0, **kw)


def both_refuse_the_same_line(contigs, text, **kw):
    import salt_amd
    with pytest.raises(salt_amd.SaltError, match=r"VCF line \d+ is malformed") as h:
        host(contigs, text)
    with pytest.raises(salt_amd.SaltError, match=r"VCF line \d+ is malformed") as g:
        gpu(contigs, text, **kw)
    line = lambda e: str(e.value).split("VCF line ")[1].split()[0]
    assert line(g) == line(h)
    return int(line(h))


@pytest.fixture(scope="module")
def built():
    """case -> (contigs, VCF text, the host twin's result and its result with pass_only), made once"""
    out = {}
    for k, case in enumerate(sorted(vc.FIXTURES)):
        contigs, snps = vc.fixture(case)
        text = vc.build_vcf(contigs, snps, seed=k + 1, extra_filtered=True)
        out[case] = (contigs, text, host(contigs, text), host(contigs, text, pass_only=True))
    return out


# ---- 1. the device equals the host twin ----

@pytest.mark.parametrize("case", sorted(vc.FIXTURES))
def test_device_equals_twin_on_fixtures(built, case):
    contigs, text, want, want_pass = built[case]
    assert vc.same(gpu(contigs, text), want) and vc.same(gpu(contigs, text, pass_only=True), want_pass)
    assert want[1]["sites"] > want_pass[1]["sites"] > 0 and want[1]["unknown_contig"] > 0


def test_device_equals_twin_on_edges():
    for name in sorted(EDGES):
        text, bad = EDGES[name]
        for pass_only in (False, True):
            if bad is None:
                assert vc.same(gpu(vc.EDGE_CONTIGS, text, pass_only=pass_only), host(vc.EDGE_CONTIGS, text, pass_only=pass_only)), name
            else:
                assert both_refuse_the_same_line(vc.EDGE_CONTIGS, text, pass_only=pass_only) == bad, name


def test_rename_map_on_the_device():
    text = b"1\t2\t.\tC\tT\nab\t2\t.\tA\tC\na\t3\t.\tG\tT\nx\t1\t.\tC\tA\n"
    for rename in ({"1": "a", "x": "b"}, {"1": "a", "a": "nowhere"}, {"a": "ab", "ab": "a"}):
        assert vc.same(gpu(vc.EDGE_CONTIGS, text, rename=rename), host(vc.EDGE_CONTIGS, text, rename=rename))


# ---- 2. chunk cuts: at 64 bytes most lines outgrow the chunk, so the buffers grow too ----

@pytest.mark.parametrize("case", ["dense", "lambda"])
@pytest.mark.parametrize("chunk", [64, 257, 4096, None])
def test_result_does_not_depend_on_the_chunks(built, case, chunk):
    contigs, text, want, _ = built[case]
    assert max(len(l) for l in text.split(b"\n")) > 4096 > 64
    assert vc.same(gpu(contigs, text, chunk_bytes=chunk), want)


# ---- 3. the line finder's tile borders ----

@pytest.mark.parametrize("at", [255, 256, 257, TILE - 1, TILE, TILE + 1])
def test_newline_on_a_tile_border(at):
    """the first line's newline is byte `at` of the chunk: the last byte of a wave's share, the first of the next, and the same at a tile's end"""
    rec = lambda p, ref, alt, pad="": "a\t%d\t%s\t%s\t%s\n" % (p, pad, ref, alt)
    first = rec(2, "C", "T")
    first = rec(2, "C", "T", "i" * (at + 1 - len(first)))
    assert first.index("\n") == at
    text = (first + rec(3, "G", "A") + "\n" + rec(4, "T", "C") + "zz\t1\t.\tA\tC\n" + rec(5, "A", "G").rstrip("\n")).encode()
    want = host(vc.EDGE_CONTIGS, text)
    assert want[1]["sites"] == 4 and want[1]["first_unknown_line"] == 5
    assert vc.same(gpu(vc.EDGE_CONTIGS, text), want)
    bad = text.replace(b"\t4\t", b"\t4x\t")
    assert both_refuse_the_same_line(vc.EDGE_CONTIGS, bad) == 4


def test_more_lines_in_a_tile_than_threads():
    """1 025 lines of a one-character contig name and nothing else: 512 lines in a tile of 256 threads, every one malformed, the first is named;
    the same number of comment lines in front of records: every line is skipped and still counted in the line numbers"""
    assert both_refuse_the_same_line(vc.EDGE_CONTIGS, b"b\n" * 1025) == 1
    text = b"#\n" * 1025 + b"a\t2\t.\tC\tT\nq\t2\t.\tC\tT\n"
    want = host(vc.EDGE_CONTIGS, text)
    assert want[1]["lines"] == 2 and want[1]["first_unknown_line"] == 1027
    assert vc.same(gpu(vc.EDGE_CONTIGS, text), want) and vc.same(gpu(vc.EDGE_CONTIGS, text, chunk_bytes=100), want)
    assert both_refuse_the_same_line(vc.EDGE_CONTIGS, text + b"a\t3\t.\n", chunk_bytes=100) == 1028


# ---- 4. the compaction's tile borders ----

def test_sites_on_the_compaction_borders():
    rng = np.random.default_rng(7)
    lens = [40000, 1, 29999]
    contigs = [(n, bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), l))) for n, l in zip(("x", "one", "y"), lens)]
    assert sum(lens) == 70000
    pos = {"x": [0, 63, 64, TILE - 1, TILE, lens[0] - 1] + list(range(2 * TILE, 4 * TILE)),          # two whole tiles of sites
           "one": [0],
           "y": [0, 1, 40 * TILE - 40001 - 1, 40 * TILE - 40001, lens[2] - 1]}                      # y starts at genome offset 40 001: the tile border at 40 960
    lines = []
    for n, seq in contigs:
        for p in pos[n]:
            r = chr(seq[p])
            lines.append("%s\t%d\t.\t%s\t%s" % (n, p + 1, r, "ACGT"[("ACGT".index(r) + 1 + p % 3) % 4]))
    random_order = rng.permutation(len(lines))
    text = ("\n".join(lines[i] for i in random_order) + "\n").encode()
    want = host(contigs, text)
    assert [g[1].tolist() for g in want[0]] == [sorted(pos["x"]), [0], pos["y"]] and want[1]["kept"] == len(lines)
    assert vc.same(vc.model(contigs, text), want)
    assert vc.same(gpu(contigs, text), want) and vc.same(gpu(contigs, text, chunk_bytes=1000), want)


# ---- 5. the malformed line's number when the bad lines sit in different chunks ----

def test_malformed_line_number_across_chunks(built):
    contigs, text, _, _ = built["dense"]
    lines = text.split(b"\n")
    a, b = len(lines) // 3, 2 * len(lines) // 3
    lines[a] = b"d\t12a\t.\tA\tC"
    lines[b] = b"d\t7\t.\tA"
    bad = b"\n".join(lines)
    assert len(b"\n".join(lines[a:b])) > 2 * 1024
    for chunk in (1024, 300, None):
        assert both_refuse_the_same_line(contigs, bad, chunk_bytes=chunk) == a + 1


# ---- 6. the tool, once ----

def test_salt_idx_gpu_vcf_on_lambda(built, tmp_path):
    contigs = built["lambda"][0]
    snps = vc.read_snps(os.path.join(LAMBDA, "snps.txt"))
    text = vc.build_vcf(contigs, snps, seed=2)
    (tmp_path / "in.vcf").write_bytes(text)
    p = subprocess.run([SALT_IDX, "-k", str(SEED_LEN), "--gpu", "--vcf", os.path.join(LAMBDA, "genome.fa"), str(tmp_path / "in.vcf"), str(tmp_path / "idx")],
                       capture_output=True, text=True, env=dict(os.environ, SALT_VCF_DEVICE="1"))
    assert p.returncode == 0, p.stderr
    assert "vcf (device): lines=" in p.stderr and " sites=%d " % len(snps) in p.stderr
    same_index(str(tmp_path / "idx"), LAMBDA, sa_slack=0)
