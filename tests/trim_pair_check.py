"""Step 2p of the trimming rule (the adapters found from the mates' overlap) and the whole pair rule stated plainly in Python
-- loops over candidates and columns, nothing shared with salt_amd/csrc/salt_trim_rule.h -- and the cases the pair tests share:
test_trim_pair_host.py (the host twin), test_trim_pair_model.py (the header under the sanitizers), test_gpu_trim_pair.py (k_fq_trim_pair).
A case is (options, pair options, (seq1, qual1), (seq2, qual2)); options are trim_check's, pair options dict(min_overlap, error_pct) or None.

The layout is stated twice: model_layout walks every candidate I and every column of mate 1 against letter I - 1 - j of mate 2; the quick
form lays mate 1 over the reverse complement of mate 2 and counts all shifts at once by correlation.  The tests hold one against the other."""
import random

import numpy as np

import trim_check as tc

COUNTERS = ("pairs", "overlapping", "trimmed", "reads1", "bases1", "reads2", "bases2", "skipped_long")
PAIR_DEFAULTS = dict(min_overlap=20, error_pct=10)
MAX_LEN = 512
_CODE = {c: i for i, c in enumerate("ACGT")}
_CODE.update({c.lower(): i for c, i in list(_CODE.items())})


def popts(**kw):
    p = dict(PAIR_DEFAULTS)
    p.update(kw)
    return p


def _codes(seq):
    return [_CODE.get(chr(c), 4) for c in seq]


def clip_qual(o, seq, qual):
    """steps 1 and 2 -> (beg, end behind the clips, end behind the quality rule)"""
    L = len(seq)
    beg = min(o["front"], L)
    end = max(L - o["tail"], beg)
    e1 = end
    if o["qual"]:
        s, best, cut = 0, 0, end
        for i in range(end - 1, beg - 1, -1):
            s += o["qual"] - max(qual[i] - 33, 0)
            if s < 0:
                break
            if s > best:
                best, cut = s, i
        end = cut
    return beg, e1, end


def adapter_end(o, mate, seq, beg, end):
    """step 3 -> end"""
    ad = o["adapter"] if mate == 0 or not o["adapter2"] else o["adapter2"]
    if ad:
        ad = ad.upper()
        for p in range(beg, end):
            ov = min(len(ad), end - p)
            if ov < o["min_overlap"]:
                break
            mm = sum(1 for j in range(ov) if chr(seq[p + j]).upper() not in "ACGT" or chr(seq[p + j]).upper() != ad[j])
            if 100 * mm <= o["error_pct"] * ov:
                return p
    return end


def model_layout(po, s1, b1, e1, s2, b2, e2):
    """step 2p, candidate by candidate and column by column -> I*, or 0"""
    P, Ep = po["min_overlap"], po["error_pct"]
    c1 = _codes(s1)
    c2c = [3 - c if c < 4 else 4 for c in _codes(s2)]                 # mate 2's letters complemented, in mate 2's order
    for I in range(e1 + e2 - P, 0, -1):
        j0, j1 = max(b1, I - e2), min(e1, I - b2)
        ov = max(j1 - j0, 0)
        if ov < P:
            continue
        # column j faces letter I - 1 - j: j0 .. j1 - 1 against I - 1 - j0 down to I - j1
        facing = c2c[I - j1:I - j0][::-1]
        mm = sum(1 for x, y in zip(c1[j0:j1], facing) if x != y or x == 4)
        if 100 * mm <= Ep * ov:
            return I
    return 0


def quick_layout(po, s1, b1, e1, s2, b2, e2):
    """the same by correlation of mate 1 with R, the reverse complement of mate 2: entry I - 1 of a full correlation is the shift L2 - I"""
    P, Ep = po["min_overlap"], po["error_pct"]
    L1, L2 = len(s1), len(s2)
    if e1 + e2 - P < 1:
        return 0
    c1 = np.array(_codes(s1))
    cR = np.array([3 - c if c < 4 else 4 for c in _codes(s2)][::-1])
    v1 = np.zeros(L1, dtype=np.int64)
    v1[b1:e1] = 1
    vR = np.zeros(L2, dtype=np.int64)
    vR[L2 - e2:L2 - b2] = 1
    ov = np.correlate(v1, vR, "full")
    match = np.zeros_like(ov)
    for x in range(4):
        match += np.correlate(v1 * (c1 == x), vR * (cR == x), "full")
    mm = ov - match
    top = min(e1 + e2 - P, L1 + L2 - 1)
    ok = (ov[:top] >= P) & (100 * mm[:top] <= Ep * ov[:top])
    hit = np.flatnonzero(ok)
    return int(hit[-1]) + 1 if len(hit) else 0


def model_pair_span(o, po, r1, r2, counts=None, pair_counts=None, layout=quick_layout):
    """The whole rule on one pair -> (b1, e1, b2, e2); counts: a (2, 8) array, pair_counts: an (8,) array the pair's counters are added to."""
    reads = (r1, r2)
    beg, e1, e2 = [0, 0], [0, 0], [0, 0]
    for m, (s, q) in enumerate(reads):
        assert len(s) >= 1 and len(q) == len(s)
        beg[m], e1[m], e2[m] = clip_qual(o, s, q)
    end = list(e2)
    if po:
        skipped = len(r1[0]) > MAX_LEN or len(r2[0]) > MAX_LEN
        I = 0 if skipped else layout(po, r1[0], beg[0], end[0], r2[0], beg[1], end[1])
        t = [end[m] - min(end[m], I) if I else 0 for m in (0, 1)]
        if pair_counts is not None:
            pair_counts += np.array([1, I != 0, t[0] + t[1] != 0, t[0] != 0, t[0], t[1] != 0, t[1], skipped], dtype=np.uint64)
        if I:
            end = [min(e, I) for e in end]
    out = []
    for m, (s, q) in enumerate(reads):
        L, e2p = len(s), end[m]
        e3 = adapter_end(o, m, s, beg[m], e2p)
        b, e = beg[m], e3
        floored = e <= b
        if floored:
            b = min(b, L - 1)
            e = b + 1
        if counts is not None:
            counts[m] += np.array([1, L, e - b, e2[m] < e1[m], e1[m] - e2[m], e3 < e2p, e2p - e3, floored], dtype=np.uint64)
        out += [b, e]
    return tuple(out)


def model_fastq_pair(o, po, fastq1, fastq2, counts=None, pair_counts=None):
    """Two blocks trimmed by the model: 4-line records, LF or CR LF in, LF out."""
    recs = []
    for fq in (fastq1, fastq2):
        lines = fq.split(b"\n")
        assert lines[-1] == b"" and (len(lines) - 1) % 4 == 0
        recs.append([[x.rstrip(b"\r") for x in lines[k:k + 4]] for k in range(0, len(lines) - 1, 4)])
    assert len(recs[0]) == len(recs[1])
    out = ([], [])
    for a, b in zip(*recs):
        span = model_pair_span(o, po, (a[1], a[3]), (b[1], b[3]), counts, pair_counts)
        for m, r in enumerate((a, b)):
            out[m].extend([r[0], r[1][span[2 * m]:span[2 * m + 1]], r[2], r[3][span[2 * m]:span[2 * m + 1]]])
    return tuple(b"\n".join(x) + b"\n" if x else b"" for x in out)


def key(o, po):
    return tc.key(o), (po["min_overlap"], po["error_pct"]) if po else None


def group(cases):
    """[(options, pair options, [(read1, read2), ...])]: the cases one call can take, in order of first appearance"""
    groups = {}
    for o, po, r1, r2 in cases:
        groups.setdefault(key(o, po), (o, po, []))[2].append((r1, r2))
    return list(groups.values())


def fastq_of_pairs(pairs, cr=False):
    return tc.fastq_of([p[0] for p in pairs], cr), tc.fastq_of([p[1] for p in pairs], cr)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "a": "t", "c": "g", "g": "c", "t": "a", "n": "n"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def mates_of(rng, insert, L1, L2, ad1=tc.ADAPTER, ad2=tc.ADAPTER2):
    """the two mates of an insert: each reads its strand from its own end, through its adapter and into a random tail"""
    m1 = (insert + ad1 + tc._rand_seq(rng, L1))[:L1]
    m2 = (revcomp(insert) + ad2 + tc._rand_seq(rng, L2))[:L2]
    return m1, m2


def true_overlap(I, L1, L2):
    """the columns of mate 1 that mate 2 reads too, both untrimmed"""
    return max(min(L1, I) - max(0, I - L2), 0)


def _sub(s, j, to=None):
    return s[:j] + (to if to else tc._other(s[j])) + s[j + 1:]


LENS = (1, 19, 20, 21, 63, 64, 65, 127, 128, 129, 150, 511, 512)


def edge_cases():
    """The edge-case set of the pair tests: [(options, pair options, (seq1, qual1), (seq2, qual2))]."""
    rng = random.Random(20261021)
    cases = []
    off, P0 = tc.opts(), popts()

    def add(o, po, s1, s2, q1=None, q2=None):
        def rd(s, q):
            s = s.encode() if isinstance(s, str) else s
            return s, (b"I" * len(s) if q is None else (q.encode() if isinstance(q, str) else q))
        cases.append((o, po, rd(s1, q1), rd(s2, q2)))

    def pair(L1, L2, I, **kw):
        return mates_of(rng, tc._rand_seq(rng, I), L1, L2, **kw)

    # ---- every length against another, the insert at every place where something changes
    combos = sorted({(LENS[i], LENS[(i + k) % len(LENS)]) for i in range(len(LENS)) for k in (1, 4, 9)})
    for L1, L2 in combos:
        P = P0["min_overlap"]
        top = max(L1, L2)
        for I in sorted({1, P - 1, P, 63, 64, 65, 128, L2 - 1, L2, L2 + 1, L1 - 1, L1 + 1, top - 1, top, L1 + L2 - P, L1 + L2 - P + 1} - set(range(-600, 1))):
            add(off, P0, *pair(L1, L2, I))
    # equal lengths too, the usual shape
    for L in (100, 150):
        for I in (1, 19, 20, 21, 30, 64, 99, 100, 101, 149, 150, 151, 2 * L - 21, 2 * L - 20, 2 * L - 19, 2 * L, 400):
            add(off, P0, *pair(L, L, I))
    # ---- exactly floor(Ep ov / 100) mismatches and one more: at the first compared column, the last, and either side of a word boundary
    for L1, L2, I, Ep in ((150, 150, 100, 10), (150, 150, 200, 10), (100, 150, 130, 10), (150, 100, 129, 50), (150, 150, 140, 0), (129, 65, 150, 10), (70, 200, 66, 20)):
        po = popts(error_pct=Ep)
        j0, j1 = max(0, I - L2), min(L1, I)
        ov = j1 - j0
        allowed = Ep * ov // 100
        anchors = [j for j in (j0, j1 - 1, 63, 64, 127, 128) if j0 <= j < j1]
        for n_mm in (allowed, allowed + 1):
            for first in anchors:
                rest = [j for j in anchors if j != first] + [j for j in rng.sample(range(j0, j1), ov) if j not in anchors]
                m1, m2 = pair(L1, L2, I)
                for j in ([first] + rest)[:n_mm]:
                    m1 = _sub(m1, j)
                add(off, po, m1, m2)
                m1, m2 = pair(L1, L2, I)
                for j in ([first] + rest)[:n_mm]:                  # the same in mate 2: column j faces its letter I - 1 - j
                    m2 = _sub(m2, I - 1 - j)
                add(off, po, m1, m2)
    # ---- N in mate 1, in mate 2 and in both at a compared column; lower case
    for Ep in (0, 10):
        po = popts(error_pct=Ep)
        for L1, L2, I in ((100, 100, 60), (150, 120, 200), (65, 64, 64)):
            j = max(0, I - L2) + 5
            m1, m2 = pair(L1, L2, I)
            add(off, po, _sub(m1, j, "N"), m2)
            add(off, po, m1, _sub(m2, I - 1 - j, "N"))
            add(off, po, _sub(m1, j, "N"), _sub(m2, I - 1 - j, "N"))
            add(off, po, _sub(m1, j, "n"), _sub(m2, I - 1 - j, "n"))
            add(off, po, m1.lower(), m2)
            add(off, po, m1, m2.lower())
            add(off, po, m1.lower(), m2.lower())
            add(off, po, "N" * L1, "N" * L2)
    # ---- a tandem repeat: several layouts are accepted, the largest wins
    for unit, k, L1, L2 in ((10, 8, 60, 60), (7, 10, 50, 64), (3, 40, 100, 100), (25, 4, 70, 65), (10, 4, 60, 60), (2, 100, 150, 150)):
        ins = tc._rand_seq(rng, unit) * k
        add(off, P0, *mates_of(rng, ins, L1, L2))
        add(off, popts(error_pct=0), *mates_of(rng, ins, L1, L2))
    # ---- homopolymers: A against T is a match at every layout, A against A at none
    for L1, L2 in ((1, 1), (19, 20), (20, 20), (64, 65), (150, 150), (512, 511), (512, 512)):
        add(off, P0, "A" * L1, "T" * L2)
        add(off, P0, "A" * L1, "A" * L2)
        add(off, popts(error_pct=50), "AC" * (L1 // 2) + "A" * (L1 % 2), "T" * L2)
    # ---- the smallest and the largest P
    for L1, L2, I in ((1, 1, 1), (5, 3, 2), (30, 30, 10), (100, 100, 250)):
        add(off, popts(min_overlap=1, error_pct=0), *pair(L1, L2, I))
    for L1, L2, I in ((512, 512, 512), (512, 512, 511), (512, 511, 512), (512, 512, 300)):
        add(off, popts(min_overlap=512), *pair(L1, L2, I))
        add(off, popts(min_overlap=400), *pair(L1, L2, I))
    # ---- spans moved by the clips, and by a quality cut on one mate only
    hi, lo = "I", "#"
    for L1, L2, I in ((100, 100, 60), (150, 150, 149), (150, 150, 200), (100, 150, 40), (129, 64, 100)):
        m1, m2 = pair(L1, L2, I)
        for o in (tc.opts(front=3, tail=2), tc.opts(front=10), tc.opts(tail=30), tc.opts(qual=20), tc.opts(qual=20, front=2, tail=1)):
            add(o, P0, m1, m2)
            add(o, P0, m1, m2, hi * (L1 - L1 // 3) + lo * (L1 // 3), None)
            add(o, P0, m1, m2, None, hi * (L2 - L2 // 2) + lo * (L2 // 2))
            add(o, P0, m1, m2, lo * L1, None)                        # mate 1 cut to nothing: no column is compared
    # ---- a front clip larger than I*: the floor catches it
    for L, I, f in ((100, 30, 31), (100, 30, 60), (150, 64, 65), (60, 25, 59)):
        m1, m2 = pair(L, L, I)
        add(tc.opts(front=f), P0, m1, m2)
        add(tc.opts(front=f), popts(min_overlap=1), m1, m2)
    # ---- the pair step, then an adapter hit in what it left
    for L, I, p in ((150, 100, 40), (150, 149, 60), (100, 200, 50), (150, 100, 0)):
        ins = tc._rand_seq(rng, I)
        ins = (ins[:p] + tc.ADAPTER + ins[p + len(tc.ADAPTER):])[:I]
        m1, m2 = mates_of(rng, ins, L, L)
        for o in (tc.opts(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2), tc.opts(adapter=tc.ADAPTER, qual=20, front=1)):
            add(o, P0, m1, m2)
            add(o, None, m1, m2)
    # read-through pairs with the known adapters searched for as well: step 3 finds nothing more, or finds what step 2p missed
    for L, I in ((150, 100), (150, 10), (150, 25), (100, 99)):
        m1, m2 = pair(L, L, I)
        add(tc.opts(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2), P0, m1, m2)
        add(tc.opts(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2), None, m1, m2)
    # ---- a mate of more than 512 letters: the pair step is skipped, the others run
    for L1, L2 in ((513, 100), (100, 513), (513, 513), (600, 512)):
        m1, m2 = pair(L1, L2, 80)
        add(off, P0, m1, m2)
        add(tc.opts(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2, qual=20, tail=1), P0, m1, m2, None, hi * (L2 - 9) + lo * 9)
    return cases


def constructed_pairs(n=600, seed=4, L=100):
    """(fastq1, fastq2): n pairs cut from the lambda genome of the goldens for the CLI and output tests -- a third read through a short insert
    into their adapters, a third overlap without reading through, the rest lie 400 to 600 bases apart; 1 % substitutions, some low tails."""
    from conftest import LAMBDA
    import os
    rng = random.Random(seed)
    genome = "".join(l.strip() for l in open(os.path.join(LAMBDA, "genome.fa")).read().split(">")[1].split("\n")[1:]).upper()
    pairs = []
    for i in range(n):
        I = (rng.randint(20, L - 1), rng.randint(L, 2 * L - 1), rng.randint(400, 600))[i % 3]
        at = rng.randrange(0, len(genome) - I)
        ins = genome[at:at + I]
        if rng.random() < 0.5:
            ins = revcomp(ins)
        mates, quals = list(mates_of(rng, ins, L, L)), []
        for m in (0, 1):
            s = list(mates[m])
            for j in range(L):
                if rng.random() < 0.01:
                    s[j] = rng.choice("ACGT")
            mates[m] = "".join(s)
            t = rng.randint(1, 30) if rng.random() < 0.2 else 0
            quals.append("I" * (L - t) + "".join(chr(33 + rng.randint(2, 10)) for _ in range(t)))
        pairs.append(((mates[0].encode(), quals[0].encode()), (mates[1].encode(), quals[1].encode())))
    return fastq_of_pairs(pairs)


def random_pairs(n=20000, seed=9, sub_pct=1, with_truth=False):
    """(options, pair options, pairs): ragged lengths 1 .. 300, inserts 1 .. 500, sub_pct % substitutions, some low-quality tails, N and lower
    case.  with_truth: a fourth value, the true insert length of every pair."""
    rng = random.Random(seed)
    o = tc.opts(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2, qual=20, front=1, tail=1) if sub_pct else tc.opts()
    pairs, truth = [], []
    for _ in range(n):
        L1, L2 = rng.randint(1, 300), rng.randint(1, 300)
        if rng.random() < 0.5:
            L2 = L1
        I = rng.randint(1, 500) if rng.random() < 0.8 else rng.randint(1, 60)
        mates = list(mates_of(rng, tc._rand_seq(rng, I), L1, L2))
        quals = []
        for m in (0, 1):
            s = list(mates[m])
            if sub_pct:
                for j in range(len(s)):
                    if rng.random() * 100 < sub_pct:
                        s[j] = rng.choice("ACGT")
                if rng.random() < 0.05:
                    s[rng.randrange(len(s))] = "N"
            mates[m] = "".join(s)
            if sub_pct and rng.random() < 0.05:
                mates[m] = mates[m].lower()
            q = [rng.choice("?FI5") for _ in s]
            if sub_pct and rng.random() < 0.3:
                t = rng.randint(0, len(s))
                q[len(s) - t:] = [rng.choice("#$%&'()*+5I") for _ in range(t)]
            quals.append("".join(q))
        pairs.append(((mates[0].encode(), quals[0].encode()), (mates[1].encode(), quals[1].encode())))
        truth.append(I)
    return (o, popts(), pairs, truth) if with_truth else (o, popts(), pairs)
