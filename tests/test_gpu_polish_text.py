"""`polish` over text on the device: salt_gpu_polish_text (through salt_amd.Polisher) and the binary's device path against the outputs of
the REAL reference `polish` committed under tests/golden/lambda (make_polish_fixture.py, make_polish_text_fixture.py), against the
product's own host path (SALT_POLISH_HOST=1) where the reference itself cannot run the input, and the loud errors."""
import os
import re
import subprocess
import sys

import pytest

import polish_text_cases as ptc
from conftest import GOLDEN, LAMBDA, ROOT

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)
from make_polish_fixture import CASES, EDGE_CASES, polish_input          # noqa: E402

POLISH = os.path.join(ROOT, "salt_amd", "bin", "polish")
DEVICE, HOST = {"SALT_POLISH_DEVICE": "1"}, {"SALT_POLISH_HOST": "1"}


def golden(name):
    return ptc.expected(name)


def all_inputs():
    """name of the expected output -> (polish arguments, input bytes): the five CASES and four EDGE_CASES of make_polish_fixture.py and every
    new fixture"""
    d = {out: (list(args), polish_input(os.path.join(LAMBDA, src), "-p" in args)) for out, args, src in CASES}
    d.update({out: (list(args), golden("polish_edge_in.sam")) for out, args in EDGE_CASES})
    d.update({exp: (list(args), data) for exp, args, data in ptc.fixtures()})
    return d


INPUTS = all_inputs()
NO_GOLDEN = ptc.no_golden_cases()


def body(data):
    """the record lines: the header is the caller's (sam_skipHeader, samParser.c:43-55)"""
    lines = data.split(b"\n")
    k = 0
    while k < len(lines) and lines[k].startswith(b"@"):
        k += 1
    return b"\n".join(lines[k:])


@pytest.fixture(scope="module")
def lam_index(tmp_path_factory):
    prefix = str(tmp_path_factory.mktemp("poltidx") / "idx")
    subprocess.run([os.path.join(ROOT, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return prefix


@pytest.fixture(scope="module")
def polisher():
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    p = salt_amd.Polisher(idx, device=0)
    yield p
    p.close()
    idx.destroy()


def run(lam_index, args, data, tmp_path, env):
    sam = tmp_path / "in.sam"
    sam.write_bytes(data)
    return subprocess.run([POLISH] + list(args) + [lam_index, str(sam)], capture_output=True, env=dict(os.environ, **env), timeout=120)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_the_library_call_equals_the_reference(name, polisher):
    args, data = INPUTS[name]
    got = polisher.polish_text(body(data), paired="-p" in args, sw="-s" in args)
    want = golden(name)
    g, w = got.split(b"\n"), want.split(b"\n")
    bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
    assert len(g) == len(w) and not bad, (len(g), len(w), len(bad), [(g[i][:160], w[i][:160]) for i in bad[:2]])
    st = polisher.stats()
    assert st[0] == want.count(b"\n") and st[6] == len(want) and st[7] == 0
    if "edge" in name:
        assert st[3] > 0                                         # windows clipped at the genome end went through the device path


def count(data, paired):
    """records, hits as parsed, unique hits per (strand, contig, position): a few lines of Python over well-formed records"""
    recs = [l.split(b"\t") for l in body(data).split(b"\n") if l]
    if paired:
        recs = recs[:len(recs) & ~1]
    parsed = unique = 0
    for f in recs:
        hits = [(int(f[1]) >> 4 & 1, f[2], int(f[3]))] if not int(f[1]) & 4 and f[2] != b"*" else []
        for xa in [o for o in f[11:] if o.startswith(b"XA:Z:")][:1]:
            hits += [(int(m.group(2) == b"-"), m.group(1), int(m.group(3))) for m in re.finditer(rb"([^,;:]+),([+-])(\d+),[^;]*;", xa[5:])]
        parsed += len(hits)
        unique += len(set(hits))
    return len(recs), parsed, unique


@pytest.mark.parametrize("name", ["polish_text_manyhits_se.sam", "polish_text_manyhits_pe.sam", "expect_polish_edge_se.sam", "polish_text_ragged_pe_lv.sam",
                                  "expect_polish_se_r1_lv.sam"])
def test_the_stats_equal_a_python_count(name, polisher):
    args, data = INPUTS[name]
    polisher.polish_text(body(data), paired="-p" in args, sw="-s" in args)
    assert tuple(polisher.stats()[:3]) == count(data, "-p" in args)


@pytest.mark.parametrize("chunk", [300, 4096, 65536])
@pytest.mark.parametrize("name", ["polish_text_manyhits_se.sam", "polish_text_ragged_pe_lv.sam"])
def test_blocks_of_any_size_give_the_golden_bytes(name, chunk, lam_index, tmp_path):
    """a 1 000-item record is about 25 KB: the smallest value forces the one-record rule; pairs stay together across cuts"""
    args, data = INPUTS[name]
    p = run(lam_index, args, data, tmp_path, dict(DEVICE, SALT_POLISH_CHUNK=str(chunk)))
    assert p.returncode == 0, p.stderr[-300:]
    assert p.stdout == golden(name)
    blocks = int(re.search(rb"device path: (\d+) block", p.stderr).group(1))
    assert blocks > 1 if chunk < len(data) else blocks == 1


@pytest.mark.parametrize("name", sorted(INPUTS) + sorted(NO_GOLDEN))
def test_the_device_path_equals_the_host_path(name, lam_index, tmp_path):
    """Both paths of the binary, byte for byte.  For the three inputs without a golden -- an earlier optional field that contains "XA", an XA
    field without its final ';' followed by another field (the reference dies on both with a segmentation fault) and reads with N (the
    reference prints memory garbage for them) -- the product's own host path is the yardstick."""
    args, data = INPUTS[name] if name in INPUTS else NO_GOLDEN[name]
    d, h = run(lam_index, args, data, tmp_path, DEVICE), run(lam_index, args, data, tmp_path, HOST)
    assert b"device path" in d.stderr and b"host path" in h.stderr
    assert d.returncode == 0 and h.returncode == 0, (d.stderr[-300:], h.stderr[-300:])
    assert d.stdout == h.stdout and len(d.stdout) > 200
    if name in INPUTS:
        assert d.stdout == golden(name)


def ragged():
    args, data = INPUTS["polish_text_ragged_default_lv.sam"]
    return [l for l in body(data).split(b"\n") if l], golden("polish_text_ragged_default_lv.sam").split(b"\n")


def test_a_ten_field_record_in_the_third_block_fails_behind_the_earlier_blocks(lam_index, tmp_path):
    recs, want = ragged()
    ends, size = [], 0                                           # a block is cut behind the first record that takes it to 4 096 bytes
    for i, r in enumerate(recs):
        size += len(r) + 1
        if size >= 4096:
            ends.append(i + 1)
            size = 0
    bad = ends[1] + 1                                            # the second record of the third block
    assert bad < ends[2]
    recs[bad] = b"\t".join(recs[bad].split(b"\t")[:10])
    p = run(lam_index, [], ptc.HDR + b"\n".join(recs) + b"\n", tmp_path, dict(DEVICE, SALT_POLISH_CHUNK="4096"))
    assert p.returncode == 1
    assert b"malformed SAM record 1 of the block: fewer than 11 fields" in p.stderr
    assert p.stdout == b"\n".join(want[:ends[1]]) + b"\n"


def test_an_unknown_contig_is_named(lam_index, tmp_path):
    recs, _ = ragged()
    f = recs[3].split(b"\t")
    recs[3] = b"\t".join(f[:2] + [b"chrNope"] + f[3:])
    p = run(lam_index, [], ptc.HDR + b"\n".join(recs[:20]) + b"\n", tmp_path, DEVICE)
    assert p.returncode == 1 and p.stdout == b""
    assert b"sequence chrNope is not in the index" in p.stderr


def test_a_513_base_read_is_refused(lam_index, tmp_path):
    recs, _ = ragged()
    f = recs[2].split(b"\t")
    recs[2] = b"\t".join(f[:9] + [(f[9] * 30)[:513], (f[10] * 30)[:513]] + f[11:])
    p = run(lam_index, [], ptc.HDR + b"\n".join(recs[:20]) + b"\n", tmp_path, DEVICE)
    assert p.returncode == 1 and p.stdout == b""
    assert b"polish item: read length / window / bound outside the kernel's range" in p.stderr


def test_an_error_returns_no_records_from_the_library(polisher):
    import salt_amd
    recs, _ = ragged()
    with pytest.raises(salt_amd.SaltError, match="malformed SAM record 5 of the block"):
        polisher.polish_text(b"\n".join(recs[:5] + [b"only\tthree\tfields"] + recs[5:9]) + b"\n")
    assert polisher.polish_text(b"\n".join(recs[:5]) + b"\n").count(b"\n") == 5          # the handle goes on working


def test_an_empty_line_ends_the_block(polisher):
    args, data = ptc.parser_cases()["empty_line"]
    got = polisher.polish_text(body(data))
    assert polisher.stopped and polisher.n_records == 1
    assert got == golden("polish_text_parse_empty_line.sam") and got.count(b"\n") == 1
    polisher.polish_text(body(ptc.parser_cases()["no_header"][1]))
    assert not polisher.stopped and polisher.n_records == 2
