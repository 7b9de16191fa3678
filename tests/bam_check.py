"""A BAM reader in plain Python, written from the SAM specification (4.2: the BAM format; 5.3: the bin of a region) and sharing no code
with the encoders, for the `salt --bam` tests: gzip members by bgzf_check, records by struct.  Every record is checked on the way (the
block_size arithmetic, l_read_name and the NUL behind the name, bin against POS and the CIGAR, the reference ids) and printed as the SAM
line it stands for.  One stated difference: `salt --bam` writes XV as an array, XV:B:I,a,b; it is printed the way `salt` prints it in SAM,
XV:i:a,b."""
import struct

from bgzf_check import stream_text

SEQ_CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
ARRAY_TYPES = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


def reg2bin(beg, end):
    """SAM spec 5.3: the bin of the zero-based half-open interval [beg, end)."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def parse_header(data):
    """(header text, [(name, length)], offset of the first record)"""
    assert data[:4] == b"BAM\x01", "no BAM magic"
    l_text, = struct.unpack_from("<i", data, 4)
    text = data[8:8 + l_text]
    assert len(text) == l_text and b"\x00" not in text, "header text: short, or padded with NUL"
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, at)
        name = data[at + 4:at + 4 + l_name]
        assert l_name >= 2 and len(name) == l_name and name[-1:] == b"\x00" and b"\x00" not in name[:-1], "reference name"
        l_ref, = struct.unpack_from("<i", data, at + 4 + l_name)
        refs.append((name[:-1], l_ref))
        at += 8 + l_name
    sq = [l.split(b"\t") for l in text.split(b"\n") if l.startswith(b"@SQ")]
    assert [(f[1][3:], int(f[2][3:])) for f in sq] == refs, "the reference list is not the @SQ lines"
    return text, refs, at


def _tag_text(data, at, end):
    """one tag at data[at:] -> (its SAM text, offset behind it)"""
    tag = data[at:at + 2].decode()
    typ = chr(data[at + 2])
    at += 3
    if typ == "Z":
        z = data.index(b"\x00", at, end)
        return "%s:Z:%s" % (tag, data[at:z].decode()), z + 1
    if typ == "A":
        return "%s:A:%s" % (tag, chr(data[at])), at + 1
    if typ == "B":
        sub = chr(data[at])
        n, = struct.unpack_from("<i", data, at + 1)
        fmt = ARRAY_TYPES[sub]
        size = struct.calcsize(fmt)
        vals = [struct.unpack_from(fmt, data, at + 5 + k * size)[0] for k in range(n)]
        assert at + 5 + n * size <= end, "array tag runs past its record"
        if tag == "XV":
            assert sub == "I" and n >= 1, "XV must be an array of uint32 with at least one offset"
            return "XV:i:" + ",".join(str(v) for v in vals), at + 5 + n * size
        return "%s:B:%s,%s" % (tag, sub, ",".join(str(v) for v in vals)), at + 5 + n * size
    assert tag != "XV", "XV must be an array (B:I), found type %s" % typ
    fmt = ARRAY_TYPES[typ]
    v, = struct.unpack_from(fmt, data, at)
    return "%s:%s:%s" % (tag, "f" if typ == "f" else "i", v), at + struct.calcsize(fmt)


def records(data, at, refs):
    """[dict of the decoded fields + 'sam': the line] of the records in data[at:], every one checked."""
    out = []
    while at < len(data):
        assert at + 36 <= len(data), "a record's fixed part runs past the stream"
        block_size, = struct.unpack_from("<i", data, at)
        ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", data, at + 4)
        end = at + 4 + block_size
        assert block_size >= 32 and end <= len(data), "block_size %d at byte %d" % (block_size, at)
        p = at + 36
        assert 2 <= l_name <= 255, "l_read_name %d" % l_name
        name = data[p:p + l_name]
        assert name[-1:] == b"\x00" and b"\x00" not in name[:-1], "read name not NUL-terminated (or holds a NUL)"
        p += l_name
        cig = struct.unpack_from("<%dI" % n_cig, data, p)
        p += 4 * n_cig
        assert all((c & 15) < len(CIGAR_OPS) for c in cig), "CIGAR operation code"
        packed = data[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(SEQ_CODES[b >> 4] + SEQ_CODES[b & 15] for b in packed)[:l_seq]
        if l_seq & 1:
            assert packed[-1] & 15 == 0, "the unused last nibble of SEQ is not zero"
        qual = data[p:p + l_seq]
        p += l_seq
        assert p <= end, "the fixed-length fields run past block_size"
        assert -1 <= ref_id < len(refs) and -1 <= next_ref < len(refs), "reference id out of range"
        assert pos >= -1 and next_pos >= -1
        ref_len = sum(c >> 4 for c in cig if CIGAR_OPS[c & 15] in "MDN=X")
        want_bin = 4680 if pos < 0 else reg2bin(pos, pos + (ref_len if ref_len > 0 else 1))
        assert bin_ == want_bin, "bin %d, reg2bin gives %d (pos %d, reference length %d)" % (bin_, want_bin, pos, ref_len)
        if cig:
            assert sum(c >> 4 for c in cig if CIGAR_OPS[c & 15] in "MIS=X") == l_seq, "CIGAR and l_seq disagree"
        if l_seq and qual[0] == 0xFF:
            assert qual == b"\xff" * l_seq
            qual_text = "*"
        else:
            assert all(q <= 93 for q in qual), "a quality above 93: not Phred, the + 33 was kept?"
            qual_text = "".join(chr(q + 33) for q in qual)
        tags = []
        while p < end:
            t, p = _tag_text(data, p, end)
            tags.append(t)
        assert p == end, "tags do not end where block_size says"
        rname = refs[ref_id][0].decode() if ref_id >= 0 else "*"
        rnext = "*" if next_ref < 0 else "=" if next_ref == ref_id else refs[next_ref][0].decode()
        cigar_text = "".join("%d%s" % (c >> 4, CIGAR_OPS[c & 15]) for c in cig) or "*"
        fields = [name[:-1].decode(), str(flag), rname, str(pos + 1), str(mapq), cigar_text, rnext, str(next_pos + 1), str(tlen), seq or "*", qual_text] + tags
        out.append(dict(name=name[:-1], flag=flag, ref_id=ref_id, pos=pos, mapq=mapq, bin=bin_, cigar=cig, l_seq=l_seq, next_ref=next_ref, next_pos=next_pos,
                        tlen=tlen, packed=packed, qual=qual, tags=tags,
                        bytes=data[at:end], sam="\t".join(fields).encode()))
        at = end
    return out


def decode_records(data, refs):
    """raw record bytes (no header) -> their SAM lines, one b"...\\n" each"""
    return b"".join(r["sam"] + b"\n" for r in records(data, 0, refs))


def decode_stream(stream):
    """A complete BAM file (BGZF members, the end-of-file block last) -> (header text, the records as SAM lines, the record dicts)."""
    data = stream_text(stream)
    text, refs, at = parse_header(data)
    recs = records(data, at, refs)
    return text, b"".join(r["sam"] + b"\n" for r in recs), recs


def sam_records(sam):
    """What the BAM of a SAM output must decode to: its record lines, the empty ones (skipped reads, the paired-end driver's) dropped."""
    return b"".join(l + b"\n" for l in sam.split(b"\n") if l and not l.startswith(b"@"))


def sam_header(sam):
    return b"".join(l + b"\n" for l in sam.split(b"\n") if l.startswith(b"@"))


def boundary_reads(genome_fa):
    """FASTQ text of 100-base reads cut from the first contig so that they end on, start one base before and start on a multiple of
    16 384 (both strands): where bin computed from POS and bin computed from POS - 1 differ.  (The goldens' genome is 48 kb; among two
    thousand random reads almost none lies there.)"""
    seq = []
    for l in open(genome_fa):
        if l.startswith(">"):
            if seq:
                break
            continue
        seq.append(l.strip())
    seq = "".join(seq).upper()
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    out = []
    for edge in (16384, 32768):
        for start in (edge - 100, edge - 1, edge, edge - 50):
            for strand in "+-":
                r = seq[start:start + 100]
                if strand == "-":
                    r = "".join(comp[c] for c in reversed(r))
                out.append("@edge_%d_%s\n%s\n+\n%s\n" % (start, strand, r, "".join(chr(40 + (k * 7) % 50) for k in range(100))))
    return "".join(out).encode()
