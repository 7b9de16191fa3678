"""What a BGZF stream must look like (SAM spec 4.1; htslib bgzf.c), shared by the `salt --bgzf` tests: every member is a gzip member with
the 'BC' extra field whose BSIZE is the member's length - 1, holds at most 65 280 bytes of text, and carries the CRC-32 and ISIZE of that
text; a complete stream ends with the 28-byte empty block."""
import struct
import zlib

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_ISIZE = 65280


def members(stream):
    """[(member bytes, its text)] of a run of BGZF blocks, every field checked."""
    out = []
    at = 0
    while at < len(stream):
        h = stream[at:at + 18]
        assert len(h) == 18 and h[:4] == b"\x1f\x8b\x08\x04", "no gzip member with an extra field at byte %d" % at
        assert h[10:16] == b"\x06\x00BC\x02\x00", "no BC field at byte %d" % at
        bsize = struct.unpack("<H", h[16:18])[0] + 1
        m = stream[at:at + bsize]
        assert len(m) == bsize and bsize <= 65536, "member at byte %d: BSIZE %d" % (at, bsize)
        crc, isize = struct.unpack("<II", m[-8:])
        d = zlib.decompressobj(-15)
        text = d.decompress(m[18:-8])
        assert d.eof and not d.unused_data, "member at byte %d: deflate stream does not end with the member" % at
        assert len(text) == isize <= MAX_ISIZE and zlib.crc32(text) == crc, "member at byte %d: ISIZE / CRC" % at
        out.append((m, text))
        at += bsize
    return out


def stream_text(stream):
    """The text of a COMPLETE stream: members as above, the end-of-file block last and nowhere else."""
    ms = members(stream)
    assert stream[-28:] == EOF and ms and ms[-1][0] == EOF, "no end-of-file block"
    assert all(t for _, t in ms[:-1]), "an empty block inside the stream"
    return b"".join(t for _, t in ms)


def strip_pg(text):
    return b"".join(l for l in text.splitlines(keepends=True) if not l.startswith(b"@PG"))
