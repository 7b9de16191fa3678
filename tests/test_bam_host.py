"""The host BAM encoder (salt_bam_header / salt_bam_from_sam behind api.bam_header / api.bam_from_sam) on every golden SAM file that `salt`
itself produces: the records decode back to the same lines (tests/bam_check.py, a reader written from the specification), and every record
is compared field by field with its SAM line, parsed here once more."""
import glob
import os
import struct

import pytest

import bam_check
from conftest import LAMBDA

GOLDENS = sorted(os.path.basename(f)[len("expect_"):-len(".sam")] for f in glob.glob(os.path.join(LAMBDA, "expect_*.sam")) if "polish" not in f)
NIBBLE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 15}
OPS = {"M": 0, "I": 1, "D": 2, "S": 4}


@pytest.fixture(scope="module")
def index():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield ix
    ix.destroy()


def _golden(case):
    return open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()


def _cigar_words(text):
    if text == "*":
        return ()
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | OPS[ch])
            n = ""
    return tuple(out)


def _check_fields(line, rec, names):
    f = line.decode().split("\t")
    rid = -1 if f[2] == "*" else names.index(f[2])
    assert rec["name"].decode() == f[0] and rec["bytes"][36 + len(f[0])] == 0 and rec["bytes"][12] == len(f[0]) + 1
    assert rec["flag"] == int(f[1]) and rec["ref_id"] == rid and rec["pos"] == int(f[3]) - 1 and rec["mapq"] == int(f[4])
    assert rec["cigar"] == _cigar_words(f[5])
    ref_len = sum(w >> 4 for w in rec["cigar"] if (w & 15) in (0, 2)) or 1
    assert rec["bin"] == (4680 if int(f[3]) == 0 else bam_check.reg2bin(int(f[3]) - 1, int(f[3]) - 1 + ref_len))
    assert rec["next_ref"] == (rid if f[6] == "=" else -1 if f[6] == "*" else names.index(f[6]))
    assert rec["next_pos"] == int(f[7]) - 1 and rec["tlen"] == int(f[8]) and rec["l_seq"] == len(f[9])
    nib = [NIBBLE[c] for c in f[9]] + [0]
    assert rec["packed"] == bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(f[9]), 2))
    assert rec["qual"] == bytes(ord(c) - 33 for c in f[10])
    # the tags, byte for byte
    want = b""
    for t in f[11:]:
        tag, typ, val = t.split(":", 2)
        if tag == "XV":
            items = [int(v) for v in val.split(",")]
            want += b"XVBI" + struct.pack("<i%dI" % len(items), len(items), *items)
        elif typ == "Z":
            want += tag.encode() + b"Z" + val.encode() + b"\x00"
        else:
            assert tag == "NM" and 0 <= int(val) < 256
            want += b"NMC" + bytes([int(val)])
    assert rec["bytes"].endswith(want) and len(rec["bytes"]) == 36 + len(f[0]) + 1 + 4 * len(rec["cigar"]) + (len(f[9]) + 1) // 2 + len(f[9]) + len(want)
    assert struct.unpack_from("<i", rec["bytes"], 0)[0] == len(rec["bytes"]) - 4


@pytest.mark.parametrize("case", GOLDENS)
def test_records_of_every_golden_decode_back_and_match_field_by_field(case, index):
    import salt_amd
    sam = _golden(case)
    lines = [l for l in sam.split(b"\n") if l and not l.startswith(b"@")]
    header = salt_amd.bam_header(index, bam_check.sam_header(sam))
    text, refs, at = bam_check.parse_header(header)
    assert text == bam_check.sam_header(sam) and at == len(header)
    assert [(nm, ln) for _, ln, nm in index.contigs()] == refs
    body = salt_amd.bam_from_sam(index, bam_check.sam_records(sam))
    assert body == salt_amd.bam_from_sam(index, b"".join(l for l in sam.splitlines(keepends=True) if not l.startswith(b"@"))), "empty lines must leave no record"
    recs = bam_check.records(body, 0, refs)
    assert len(recs) == len(lines)
    assert b"".join(r["sam"] + b"\n" for r in recs) == bam_check.sam_records(sam)
    names = [nm.decode() for nm, _ in refs]
    for line, rec in zip(lines, recs):
        _check_fields(line, rec, names)


def test_the_goldens_hold_the_shapes_the_format_is_awkward_for(index):
    """What the field check above is worth: deletion-leading CIGARs, XA:Z, reads with N, soft clips, unmapped mates (MAPQ 255), XV lists of one
    and of several offsets, odd read lengths and mapped records without a CIGAR are all among the records it has looked at."""
    seen = set()
    for case in GOLDENS:
        for l in _golden(case).split(b"\n"):
            if not l or l.startswith(b"@"):
                continue
            f = l.split(b"\t")
            if f[5].lstrip(b"0123456789")[:1] == b"D":
                seen.add("leading D")
            if b"S" in f[5]:
                seen.add("soft clip")
            if b"N" in f[9]:
                seen.add("N")
            if len(f[9]) & 1:
                seen.add("odd length")
            if f[4] == b"255" and int(f[1]) & 4:
                seen.add("unmapped mate")
            if f[2] == b"*":
                seen.add("no reference")
            for t in f[11:]:
                if t.startswith(b"XA:Z:"):
                    seen.add("XA")
                if t.startswith(b"XV:i:"):
                    seen.add("XV several" if b"," in t else "XV one")
    assert seen == {"leading D", "soft clip", "N", "odd length", "unmapped mate", "no reference", "XA", "XV several", "XV one"}


def test_a_single_xv_offset_is_an_array_too(index):
    import salt_amd
    line = b"r\t0\tlambdaA\t11\t37\t4M\t*\t0\t0\tACGT\tIIII\tMD:Z:2A1\tNM:i:1\tXV:i:2\n"
    rec = salt_amd.bam_from_sam(index, line)
    assert rec.endswith(b"MDZ2A1\x00NMC\x01XVBI\x01\x00\x00\x00\x02\x00\x00\x00")
    refs = [(nm, ln) for _, ln, nm in index.contigs()]
    assert bam_check.decode_records(rec, refs) == line


def test_names_up_to_254_bytes_and_no_further(index):
    import salt_amd
    line = b"\t4\t*\t0\t0\t*\t*\t0\t0\tACGTN\tIIII!\n"
    ok = salt_amd.bam_from_sam(index, b"n" * 254 + line)
    assert ok[12] == 255 and ok[36:36 + 255] == b"n" * 254 + b"\x00" and ok[-8:] == bytes([0x12, 0x48, 0xF0, 40, 40, 40, 40, 0])
    with pytest.raises(salt_amd.SaltError, match="at most 254 bytes"):
        salt_amd.bam_from_sam(index, b"n" * 255 + line)


def test_lines_that_are_no_records_are_refused(index):
    import salt_amd
    for bad in (b"r\t0\tnowhere\t1\t0\t4M\t*\t0\t0\tACGT\tIIII\n", b"r\t0\tlambdaA\t1\t0\t4Q\t*\t0\t0\tACGT\tIIII\n",
                b"r\t0\tlambdaA\t1\t0\t4M\t*\t0\t0\tACGT\tIII\n", b"@HD\tVN:1\n", b"r\t0\tlambdaA\t1\t0\t4M\t*\t0\t0\tACGT\tIIII\tXX:f:1.5\n"):
        with pytest.raises(salt_amd.SaltError, match="BAM:"):
            salt_amd.bam_from_sam(index, bad)


def test_bin_comes_from_the_zero_based_position(index):
    """POS 16384 is position 16383, the last base of the first 16-kb bin; worked out by hand from the specification's reg2bin."""
    import salt_amd
    for pos1, cigar, n, want in ((16384, "1M", 1, 4681), (16385, "1M", 1, 4682), (16285, "100M", 100, 4681), (16384, "100M", 100, 585),
                                 (16285, "50M1D50M", 100, 585), (16384, "*", 100, 4681), (0, "*", 100, 4680)):
        line = b"r\t0\t%s\t%d\t9\t%s\t*\t0\t0\t%s\t%s\n" % (b"lambdaA" if pos1 else b"*", pos1, cigar.encode(), b"A" * n, b"I" * n)
        rec = salt_amd.bam_from_sam(index, line)
        assert int.from_bytes(rec[14:16], "little") == want, (pos1, cigar)
