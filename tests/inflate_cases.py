"""BGZF streams for the inflate tests (the host model: test_inflate_model.py; the kernel: test_gpu_inflate.py), made with Python's zlib
(raw deflate, wbits = -15) and, where zlib cannot make them, bit by bit from RFC 1951.  Valid ones come with the text they hold; damaged
ones are valid members with one thing wrong."""
import functools
import os
import random
import struct
import subprocess
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDA = os.path.join(HERE, "golden", "lambda")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

SETTINGS = {"level1": (1, zlib.Z_DEFAULT_STRATEGY), "level6": (6, zlib.Z_DEFAULT_STRATEGY), "level9": (9, zlib.Z_DEFAULT_STRATEGY),
            "level0_stored": (0, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "rle": (6, zlib.Z_RLE), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY)}


def member(payload, text=None, crc=None, isize=None, bsize=None):
    """One BGZF member around a raw deflate payload; crc / isize / bsize override what the text and the payload give."""
    crc = zlib.crc32(text) & 0xFFFFFFFF if crc is None else crc
    isize = len(text) if isize is None else isize
    bsize = 18 + len(payload) + 8 if bsize is None else bsize
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize - 1)
            + payload + struct.pack("<II", crc, isize))


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(text) + c.flush()


def bgzf(data, block=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """Blocked gzip as bgzip writes it: a member per `block` bytes, the empty end-of-file member last."""
    out = b"".join(member(deflate(data[o:o + block], level, strategy), data[o:o + block]) for o in range(0, len(data), block))
    return out + (EOF if eof else b"")


class Bits:
    """A deflate bit stream: fields lowest bit first, Huffman codes highest bit first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def fixed_litlen(b, sym):
    """The fixed code of RFC 1951 3.2.6."""
    if sym < 144:
        b.code(0x30 + sym, 8)
    elif sym < 256:
        b.code(0x190 + sym - 144, 9)
    elif sym < 280:
        b.code(sym - 256, 7)
    else:
        b.code(0xC0 + sym - 280, 8)


def far_distance_member():
    """What zlib cannot produce (its distances stop at 32 506): a stored block of 32 768 random bytes, then a fixed block of 126 matches of
    length 258 (symbol 285) at distance 32 768 (code 29, extra bits 8 191), then end-of-block.  65 276 bytes of text."""
    head = random.Random(29).randbytes(32768)
    b = Bits()
    b.put(0, 1); b.put(0, 2); b.align()
    b.put(32768, 16); b.put(32768 ^ 0xFFFF, 16)
    b.out += head
    b.put(1, 1); b.put(1, 2)
    for _ in range(126):
        fixed_litlen(b, 285)
        b.code(29, 5); b.put(8191, 13)
    fixed_litlen(b, 256)
    text = bytearray(head)
    for _ in range(126 * 258):
        text.append(text[-32768])
    return member(b.bytes(), bytes(text)), bytes(text)


def flushed_member(text):
    """Level 6 in pieces of 5 000 bytes, Z_SYNC_FLUSH and Z_FULL_FLUSH in turn: many deflate blocks in one member, empty stored blocks between."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    payload = b""
    for i, o in enumerate(range(0, len(text), 5000)):
        payload += c.compress(text[o:o + 5000]) + c.flush(zlib.Z_SYNC_FLUSH if i % 2 == 0 else zlib.Z_FULL_FLUSH)
    payload += c.flush()
    return member(payload, text)


def fibonacci_text():
    """The 28 656 bytes of tests/test_bgzf_model.py: byte counts that are the first 21 Fibonacci numbers (a plain Huffman tree 20 deep)."""
    r = random.Random(11)
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    skew = bytearray(b"".join(bytes([65 + i]) * f for i, f in enumerate(fib)))
    r.shuffle(skew)
    return bytes(skew)


def reads():
    return open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read()


@functools.lru_cache(maxsize=None)
def valid_cases(bgzf_model_exe=None):
    """name -> (stream, text).  With the path of a built tools/bgzf_model: also what the project's own deflater makes of 3 * 32 640 + 17 bytes of SAM."""
    fq = reads()
    block = fq[:65280]
    cases = {name: (bgzf(block, 65280, lv, st), block) for name, (lv, st) in SETTINGS.items()}
    cases["flushed"] = (flushed_member(block) + EOF, block)
    cases["whole_file_blocks_of_700"] = (bgzf(fq, 700), fq)
    cases["whole_file_blocks_of_65280"] = (bgzf(fq, 65280), fq)
    cases["zeros_65536"] = (bgzf(bytes(65536), 65536), bytes(65536))
    rnd = random.Random(17).randbytes(65280)
    cases["random_65280"] = (bgzf(rnd), rnd)
    cases["fibonacci"] = (bgzf(fibonacci_text()), fibonacci_text())
    cases["empty"] = (member(deflate(b""), b""), b"")
    cases["one_byte"] = (bgzf(b"x"), b"x")
    cases["eof_block_alone"] = (EOF, b"")
    far, far_text = far_distance_member()
    cases["distance_32768"] = (far + EOF, far_text)
    if bgzf_model_exe:
        sam = open(os.path.join(LAMBDA, "expect_pe_default.sam"), "rb").read()[:3 * 32640 + 17]
        cases["own_deflater"] = (subprocess.run([bgzf_model_exe], input=sam, capture_output=True, check=True).stdout, sam)
    return cases


def level6_block():
    """(payload, text) of the block the damaged cases start from."""
    text = reads()[:65280]
    return deflate(text), text


def flip_offsets(payload):
    return list(range(0, len(payload), 97))


def flipped(payload, text, at):
    p = bytearray(payload)
    p[at] ^= 0x55
    return member(bytes(p), text)


def zlib_rejects(stream):
    """Does zlib's inflate plus the CRC-32 and ISIZE check refuse this single member?"""
    payload, (crc, isize) = stream[18:-8], struct.unpack("<II", stream[-8:])
    try:
        d = zlib.decompressobj(-15)
        text = d.decompress(payload)
        if not d.eof or d.unused_data:
            return True
    except zlib.error:
        return True
    return zlib.crc32(text) & 0xFFFFFFFF != crc or len(text) != isize


@functools.lru_cache(maxsize=None)
def damaged_cases():
    """name -> stream; every one must be refused."""
    payload, text = level6_block()
    crc = zlib.crc32(text) & 0xFFFFFFFF
    cases = {}
    cases["crc_bit"] = member(payload, text, crc=crc ^ (1 << 13))
    cases["isize_minus_1"] = member(payload, text, isize=len(text) - 1)
    cases["isize_plus_1"] = member(payload, text, isize=len(text) + 1)
    cases["bsize_past_the_end"] = member(payload, text, bsize=18 + len(payload) + 8 + 100)
    cases["stored_len_nlen"] = member(b"\x01" + struct.pack("<HH", 5, (5 ^ 0xFFFF) ^ 0x0100) + b"hello", b"hello")
    b = Bits()                                                  # fixed block: a match of length 3 at distance 1 as the first symbol
    b.put(1, 1); b.put(1, 2); fixed_litlen(b, 257); b.code(0, 5); fixed_litlen(b, 256)
    cases["distance_in_front_of_the_block"] = member(b.bytes(), b"aaa")
    b = Bits()                                                  # dynamic block, HLIT = 31: 288 literal/length codes
    b.put(1, 1); b.put(2, 2); b.put(31, 5); b.put(0, 5); b.put(0, 4); b.put(0, 64)
    cases["hlit_31"] = member(b.bytes(), b"a")
    b = Bits()                                                  # all 19 code-length codes one bit long
    b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    b.put(0, 64)
    cases["oversubscribed_code_lengths"] = member(b.bytes(), b"a")
    b = Bits()                                                  # code-length code {16: 1 bit, 0: 1 bit}; the first length sent is "repeat the previous"
    b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(0, 5); b.put(0, 4)
    for l in (1, 0, 0, 1):
        b.put(l, 3)
    b.code(1, 1); b.put(0, 2); b.put(0, 64)
    cases["repeat_without_previous"] = member(b.bytes(), b"a")
    cases["truncated_by_1"] = member(payload[:-1], text)
    cases["truncated_by_half"] = member(payload[:len(payload) // 2], text)
    return cases
