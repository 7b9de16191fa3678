"""The trimming rule stated plainly in Python -- a loop per position, no packing, nothing shared with
salt_amd/csrc/salt_trim_rule.h -- and the cases the trim tests share: test_trim_host.py (the host twin), test_trim_model.py (the header
under the sanitizers), test_gpu_trim.py (k_fq_trim).  A case is (options, mate, seq, qual); options are the keywords of
salt_amd.trim_fastq / GpuAligner.set_trim."""
import os
import random

import numpy as np

from conftest import LAMBDA

COUNTERS = ("reads", "bases_in", "bases_out", "reads_qual", "bases_qual", "reads_adapter", "bases_adapter", "reads_floored")
DEFAULTS = dict(adapter=None, adapter2=None, qual=0, front=0, tail=0, min_overlap=5, error_pct=10)
ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"          # 33 letters (the TruSeq read-1 adapter's head)
ADAPTER2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"


def opts(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def model_span(o, mate, seq, qual, counts=None):
    """-> (beg, end); counts: a (2, 8) array the read's counters are added to."""
    L = len(seq)
    assert L >= 1 and len(qual) == L
    # 1. fixed clips, saturating
    beg = min(o["front"], L)
    end = max(L - o["tail"], beg)
    e1 = end
    # 2. 3' quality: partial sums of Q - q from the end; the cut is where the sum was largest before it first went negative
    if o["qual"]:
        s, best, cut = 0, 0, end
        for i in range(end - 1, beg - 1, -1):
            s += o["qual"] - max(qual[i] - 33, 0)
            if s < 0:
                break
            if s > best:
                best, cut = s, i
        end = cut
    e2 = end
    # 3. 3' adapter: the leftmost start whose overlap has few enough mismatches
    ad = o["adapter"] if mate == 0 or not o["adapter2"] else o["adapter2"]
    if ad:
        ad = ad.upper()
        for p in range(beg, end):
            ov = min(len(ad), end - p)
            if ov < o["min_overlap"]:
                break
            mm = 0
            for j in range(ov):
                c = chr(seq[p + j]).upper()
                if c not in "ACGT" or c != ad[j]:
                    mm += 1
            if 100 * mm <= o["error_pct"] * ov:
                end = p
                break
    e3 = end
    # 4. floor: never an empty read
    floored = end <= beg
    if floored:
        beg = min(beg, L - 1)
        end = beg + 1
    if counts is not None:
        counts[mate] += np.array([1, L, end - beg, e2 < e1, e1 - e2, e3 < e2, e2 - e3, floored], dtype=np.uint64)
    return beg, end


def model_fastq(o, mate, fastq, counts=None):
    """The block trimmed by the model: 4-line records, LF or CR LF in, LF out."""
    lines = fastq.split(b"\n")
    assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
    out = []
    for k in range(0, len(lines) - 1, 4):
        h, s, p, q = (x.rstrip(b"\r") for x in lines[k:k + 4])
        b, e = model_span(o, mate, s, q, counts)
        out += [h, s[b:e], p, q[b:e]]
    return b"\n".join(out) + b"\n"


def key(o):
    return tuple(o[k] for k in sorted(DEFAULTS))


def group(cases):
    """[(options, mate, [(seq, qual), ...])]: the cases that one call with one set of options can take, in order of first appearance."""
    groups = {}
    for o, mate, seq, qual in cases:
        groups.setdefault((key(o), mate), (o, mate, []))[2].append((seq, qual))
    return list(groups.values())


def fastq_of(reads, cr=False):
    nl = b"\r\n" if cr else b"\n"
    return b"".join(b"@r%d" % i + nl + s + nl + b"+" + nl + q + nl for i, (s, q) in enumerate(reads))


ADAPTER_LENS = (1, 5, 12, 31, 32, 33, 63, 64)
READ_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 150, 512)


def _rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _adapter(rng, n):
    """n letters in which no letter repeats its neighbour, so that a shifted copy of it mismatches often"""
    s = [rng.choice("ACGT")]
    while len(s) < n:
        s.append(rng.choice([c for c in "ACGT" if c != s[-1]]))
    return "".join(s)


def _other(c):
    return {"A": "C", "C": "G", "G": "T", "T": "A"}[c.upper()]


def _with_adapter(rng, L, p, ad, mism=(), repl=None):
    """a read of L letters with the adapter laid over it from p on (cut at the read's end), the overlap's letters at `mism` changed"""
    ov = list(ad[:max(0, L - p)])
    for j in mism:
        ov[j] = repl if repl else _other(ov[j])
    s = _rand_seq(rng, p) + "".join(ov)
    s += _rand_seq(rng, L - len(s))
    return s[:L]


def edge_cases():
    """The edge-case set of the trim tests: [(options, mate, seq bytes, qual bytes)]."""
    rng = random.Random(20260421)
    cases = []

    def add(o, seq, qual=None, mate=0):
        seq = seq.encode() if isinstance(seq, str) else seq
        qual = b"I" * len(seq) if qual is None else (qual.encode() if isinstance(qual, str) else qual)
        cases.append((o, mate, seq, qual))

    ads = {A: _adapter(rng, A) for A in ADAPTER_LENS}
    # ---- adapter: every adapter length against every read length, the adapter whole (or cut by the read's end) at the ends and in the middle
    for A, ad in ads.items():
        o = opts(adapter=ad, min_overlap=min(5, A))
        for L in READ_LENS:
            for p in sorted({0, 1, L // 2, max(L - A - 1, 0), max(L - A, 0), L - 1}):
                if p < L:
                    add(o, _with_adapter(rng, L, p, ad))
            add(o, _rand_seq(rng, L))
    # the adapter whole at every start, 0 (where the floor applies) included
    for A, ad in ads.items():
        o = opts(adapter=ad, min_overlap=min(5, A))
        for L in (A, 100, 150):
            for p in range(0, L - A + 1):
                add(o, _with_adapter(rng, L, p, ad))
    # every partial overlap 1 .. A at the read's end, M on both sides of it
    for A, ad in ads.items():
        for ov in range(1, A + 1):
            for M in {ov, ov + 1} & set(range(1, 65)):
                add(opts(adapter=ad, min_overlap=M, error_pct=0), _with_adapter(rng, 150, 150 - ov, ad))
    # exactly floor(E ov / 100) mismatches and one more, placed at the first base, the last base and on both sides of base 32 of the overlap
    for A, E in ((64, 10), (64, 50), (64, 0), (63, 10), (33, 10), (33, 50), (32, 10), (12, 10), (12, 50), (5, 50), (5, 0), (1, 50), (1, 0)):
        ad = ads[A]
        for ov in sorted({A, max(A - 1, 1), (A + 1) // 2}):
            allowed = E * ov // 100
            anchors = [j for j in (0, ov - 1, 31, 32) if j < ov]
            for n_mm in (allowed, allowed + 1):
                if n_mm > ov:
                    continue
                for first in anchors:
                    rest = [j for j in anchors if j != first] + [j for j in rng.sample(range(ov), ov) if j not in anchors]
                    mism = ([first] + rest)[:n_mm]
                    L = 150
                    p = L - ov if ov < A else rng.randrange(0, L - A + 1)
                    add(opts(adapter=ad, min_overlap=1, error_pct=E), _with_adapter(rng, L, p, ad, mism))
    # an N and a lower-case letter inside the overlap: N is a mismatch, case is ignored
    for A in (12, 33, 64):
        ad = ads[A]
        for E in (0, 10):
            o = opts(adapter=ad, error_pct=E)
            add(o, _with_adapter(rng, 100, 40, ad, [A // 2], "N"))
            add(o, _with_adapter(rng, 100, 40, ad, [0], "N"))
            s = _with_adapter(rng, 100, 40, ad)
            add(o, s[:40] + s[40:].lower())
            add(o, s.lower())
            add(opts(adapter=ad.lower(), error_pct=E), s)
            add(o, "N" * 100)
    # two acceptable starts: the leftmost wins, also where the left one is the worse match
    ad = ads[12]
    s = _rand_seq(rng, 20) + ad + _rand_seq(rng, 10) + ad + _rand_seq(rng, 30)
    add(opts(adapter=ad), s)
    bad = ad[:5] + _other(ad[5]) + ad[6:]
    add(opts(adapter=ad, error_pct=10), _rand_seq(rng, 20) + bad + _rand_seq(rng, 10) + ad + _rand_seq(rng, 30))
    add(opts(adapter=ad, error_pct=0), _rand_seq(rng, 20) + bad + _rand_seq(rng, 10) + ad + _rand_seq(rng, 30))
    # a homopolymer read against a homopolymer adapter, and against another letter's
    for A in (1, 5, 33, 64):
        for L in (1, 5, 64, 65, 150):
            add(opts(adapter="A" * A, min_overlap=min(5, A)), "A" * L)
            add(opts(adapter="C" * A, min_overlap=min(5, A), error_pct=50), "A" * L)
            add(opts(adapter="A" * A, min_overlap=min(5, A), error_pct=50), "AC" * (L // 2) + "A" * (L % 2))
    # ---- quality
    hi, lo = "I", "#"                                            # 40 and 2
    for L in (1, 2, 63, 64, 65, 100, 128, 129, 150, 512):
        s = _rand_seq(rng, L)
        for Q in (1, 20, 93):
            add(opts(qual=Q), s, hi * L)
            add(opts(qual=Q), s, lo * L)                         # all low: the floor
            add(opts(qual=Q), s, "~" * L)                        # byte 126
            add(opts(qual=Q), s, "!" * L)                        # byte 33: quality 0
        for t in sorted({1, L // 3, L // 2, L - 1} - {0}):
            add(opts(qual=20), s, hi * (L - t) + lo * t)
    for L in (100, 150, 200):
        s = _rand_seq(rng, L)
        # low, high, low: the best cut is not the first base below Q
        add(opts(qual=20), s, hi * (L - 30) + lo * 10 + hi * 5 + lo * 15)
        add(opts(qual=20), s, hi * (L - 30) + lo * 2 + hi * 20 + lo * 8)      # the high stretch outweighs the tail: the walk stops
        add(opts(qual=20), s, hi * (L - 70) + "5" * 3 + lo * 67)               # a cut in the second 64 positions from the end
        add(opts(qual=20), s, hi * (L - 66) + lo * 1 + "4" * 1 + lo * 64)
        add(opts(qual=20), s, hi * (L - 64) + lo * 64)
        add(opts(qual=20), s, hi * (L - 65) + lo * 65)
        # equal sums at two places: the one nearer the end stays
        add(opts(qual=20), s, hi * (L - 4) + "5" + "+" + "?" + "+")
        # bytes 33, 126 and one below 33 (counts as quality 0)
        add(opts(qual=20), s, (hi * (L - 6)).encode() + bytes([33, 126, 32, 9, 126, 33]))
        add(opts(qual=5), s, (hi * (L - 6)).encode() + bytes([33, 126, 32, 9, 34, 33]))
        add(opts(qual=20), s, bytes(rng.choice((33, 35, 45, 53, 60, 73, 126, 200, 255)) for _ in range(L)))
    # ---- clips, alone and meeting or passing each other
    for L in (1, 2, 10, 100, 511, 512, 600):
        s = _rand_seq(rng, L)
        for f, t in ((1, 0), (0, 1), (3, 4), (L // 2, L - L // 2), (L // 2, L // 2 + 1), (L, 0), (0, L), (L + 5, 0), (0, L + 5), (511, 511), (L - 1, 0), (0, L - 1)):
            if f <= 511 and t <= 511:
                add(opts(front=f, tail=t), s)
    # ---- all three steps, in their order: the tail clip takes bases off before the quality rule sees them, the quality cut shortens what the adapter search sees
    ad = ADAPTER
    for L in (100, 150):
        for p in (0, 3, 4, 30, 60):
            s = _with_adapter(rng, L, p, ad)
            q = hi * (L - 20) + lo * 20
            for o in (opts(adapter=ad, qual=20, front=3, tail=2), opts(adapter=ad, qual=20), opts(adapter=ad, front=5), opts(qual=20, tail=25), opts(adapter=ad, qual=20, front=3, tail=2, min_overlap=3, error_pct=20)):
                add(o, s, q)
                add(o, s, hi * L)
                add(o, s, lo * L)
        # an adapter the quality cut leaves a partial overlap of
        s = _with_adapter(rng, L, L - 33, ad)
        add(opts(adapter=ad, qual=20), s, hi * (L - 25) + lo * 25)
        add(opts(adapter=ad, qual=20, min_overlap=9), s, hi * (L - 25) + lo * 25)
    # ---- mate 2: its own adapter, and mate 1's by default
    for L in (100, 150):
        s1, s2 = _with_adapter(rng, L, 50, ADAPTER), _with_adapter(rng, L, 50, ADAPTER2)
        for o in (opts(adapter=ADAPTER, adapter2=ADAPTER2), opts(adapter=ADAPTER), opts(adapter=ADAPTER, adapter2=ADAPTER2, qual=20, front=1)):
            for mate in (0, 1):
                add(o, s1, None, mate)
                add(o, s2, None, mate)
                add(o, s2, hi * (L - 10) + lo * 10, mate)
    return cases


def random_block(n=20000, seed=7):
    """(options, reads): n records of ragged lengths 1 .. 512 -- adapters whole, partial and damaged, low-quality tails, N and lower case."""
    rng = random.Random(seed)
    o = opts(adapter=ADAPTER, adapter2=ADAPTER2, qual=20, front=1, tail=1)
    reads = []
    for _ in range(n):
        L = rng.choice((1, 2, 3, 31, 63, 64, 65, 100, 150, 151, 250, 512)) if rng.random() < 0.3 else rng.randint(1, 512)
        s = list(_rand_seq(rng, L))
        kind = rng.random()
        if kind < 0.5:
            ad = list(ADAPTER if rng.random() < 0.6 else ADAPTER2)
            for _ in range(rng.choice((0, 0, 1, 2, 3, 5))):
                j = rng.randrange(len(ad))
                ad[j] = rng.choice("ACGTN")
            p = rng.randint(0, L)
            s[p:p + len(ad)] = ad[:L - p]
        if rng.random() < 0.1:
            s[rng.randrange(L)] = "N"
        seq = "".join(s)
        if rng.random() < 0.1:
            seq = seq.lower()
        q = [rng.choice("?FI5") for _ in range(L)]
        if rng.random() < 0.5:
            t = rng.randint(0, L)
            q[L - t:] = [rng.choice("#$%&'()*+5I") for _ in range(t)]
        reads.append((seq.encode(), "".join(q).encode()))
    return o, reads


def _records(path):
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    return [lines[k:k + 4] for k in range(0, len(lines) - 1, 4)]


def constructed(fastq_name, adapter, seed, limit=None):
    """The adapter-carrying reads of the CLI and output tests, from a golden FASTQ: a third cut to a random insert of 1 to 99 bases and filled
    up with the adapter and then random bases, a third given a tail of qualities 2 to 10, the rest as it is."""
    rng = random.Random(seed)
    out = []
    for h, s, p, q in _records(os.path.join(LAMBDA, fastq_name))[:limit]:
        L = len(s)
        k = rng.randrange(3)
        if k == 0:
            ins = min(rng.randint(1, 99), L)
            s = (s[:ins] + adapter.encode() + _rand_seq(rng, L).encode())[:L]
        elif k == 1:
            t = rng.randint(1, L)
            q = q[:L - t] + bytes(33 + rng.randint(2, 10) for _ in range(t))
        out += [h, s, p, q]
    return b"\n".join(out) + b"\n"
