"""The host twins of k_fq_trim_pair (salt_trim_pair_span, salt_trim_fastq_pair: salt_amd/csrc/salt_trim_rule.h compiled for the host)
against the plain Python statement of the pair rule in trim_pair_check.py, on the edge-case set and on 20 000 seeded random pairs.  No GPU."""
import numpy as np
import pytest

import salt_amd
import trim_check as tc
import trim_pair_check as pc


def _kw(o, po):
    kw = dict(adapter=o["adapter"], adapter2=o["adapter2"], front=o["front"], tail=o["tail"], adapter_min_overlap=o["min_overlap"], adapter_error_pct=o["error_pct"])
    kw.update(dict(pair=True, min_overlap=po["min_overlap"], error_pct=po["error_pct"]) if po else dict(pair=False))
    return kw


def _twin_span(o, po, r1, r2, counts=None, pair_counts=None):
    return salt_amd.trim_pair_span(r1[0], r1[1], r2[0], r2[1], qual_min=o["qual"], counts=counts, pair_counts=pair_counts, **_kw(o, po))


def _new_counts():
    return np.zeros((2, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)


@pytest.fixture(scope="module")
def cases():
    return pc.edge_cases()


@pytest.fixture(scope="module")
def random_pairs():
    return pc.random_pairs(20000, seed=9)


def test_the_edge_case_set_is_what_it_is_meant_to_be(cases):
    """Both statements of the layout agree on every case, and the set reaches every outcome: a layout that trims, one that only counts, none,
    the floor for a mate its qualities cut to nothing, an adapter hit behind the pair step, a pair too long."""
    counts, pairs = _new_counts()
    for o, po, r1, r2 in cases:
        span = pc.model_pair_span(o, po, r1, r2, counts, pairs)
        assert span == pc.model_pair_span(o, po, r1, r2, layout=pc.model_layout), (o, po, r1, r2)
        assert 0 <= span[0] < span[1] <= len(r1[0]) and 0 <= span[2] < span[3] <= len(r2[0])
    c = dict(zip(pc.COUNTERS, (int(v) for v in pairs)))
    assert len(cases) > 800 and len(pc.group(cases)) < 40
    assert c["pairs"] > c["overlapping"] > c["trimmed"] > 100 and c["reads1"] > 100 and c["reads2"] > 100 and c["skipped_long"] == 8
    assert c["pairs"] < len(cases)                                # some cases run with the pair rule off
    for m in (0, 1):
        assert counts[m][tc.COUNTERS.index("reads_adapter")] > 0 and counts[m][tc.COUNTERS.index("reads_qual")] > 0
    assert counts[0][tc.COUNTERS.index("reads_floored")] > 5


def test_span_equals_the_model_on_every_edge_case(cases):
    want_c, want_p = _new_counts()
    got_c, got_p = _new_counts()
    bad = []
    for i, (o, po, r1, r2) in enumerate(cases):
        want, got = pc.model_pair_span(o, po, r1, r2, want_c, want_p, layout=pc.model_layout), _twin_span(o, po, r1, r2, got_c, got_p)
        if want != got:
            bad.append((i, o, po, r1[0], r2[0], want, got))
    assert not bad, (len(bad), bad[:3])
    assert (want_c == got_c).all() and (want_p == got_p).all(), (want_c, got_c, want_p, got_p)


def test_span_equals_the_model_on_the_random_pairs(random_pairs):
    o, po, pairs = random_pairs
    want_c, want_p = _new_counts()
    got_c, got_p = _new_counts()
    for i, (r1, r2) in enumerate(pairs):
        want, got = pc.model_pair_span(o, po, r1, r2, want_c, want_p), _twin_span(o, po, r1, r2, got_c, got_p)
        assert want == got, (i, r1, r2, want, got)
        if i < 300:
            assert want == pc.model_pair_span(o, po, r1, r2, layout=pc.model_layout)
    assert (want_c == got_c).all() and (want_p == got_p).all(), (want_c, got_c, want_p, got_p)
    c = dict(zip(pc.COUNTERS, (int(v) for v in want_p)))
    assert c["pairs"] == len(pairs) and c["trimmed"] > 2000 and c["overlapping"] > c["trimmed"] and c["overlapping"] < len(pairs) - 2000


@pytest.mark.parametrize("cr", [False, True])
def test_trim_fastq_pair_equals_the_model(cases, random_pairs, cr):
    groups = pc.group(cases) + [(random_pairs[0], random_pairs[1], random_pairs[2][:3000])]
    for o, po, pairs in groups:
        fq1, fq2 = pc.fastq_of_pairs(pairs, cr=cr)
        want_c, want_p = _new_counts()
        got_c, got_p = _new_counts()
        want = pc.model_fastq_pair(o, po, fq1, fq2, want_c, want_p)
        got = salt_amd.trim_fastq_pair(fq1, fq2, qual=o["qual"], counts=got_c, pair_counts=got_p, **_kw(o, po))
        assert got == want and b"\r" not in got[0] + got[1], (o, po)
        assert (want_c == got_c).all() and (want_p == got_p).all()


def test_error_free_pairs_give_the_true_insert():
    """Error-free constructed pairs, no other step: every pair whose mates truly share P columns or more is laid out at its true insert, every
    pair whose mates share none gets no layout.  No cap, no exclusions."""
    o, po, pairs, truth = pc.random_pairs(4000, seed=31, sub_pct=0, with_truth=True)
    n_found = n_none = 0
    for (r1, r2), I in zip(pairs, truth):
        L1, L2 = len(r1[0]), len(r2[0])
        got = pc.quick_layout(po, r1[0], 0, L1, r2[0], 0, L2)
        shared = pc.true_overlap(I, L1, L2)
        if shared >= po["min_overlap"]:
            assert got == I, (r1[0], r2[0], I, got)
            n_found += 1
        elif shared == 0:
            assert got == 0, (r1[0], r2[0], I, got)
            n_none += 1
    assert n_found > 1500 and n_none > 300


def test_known_layouts():
    """A few spans worked out by hand, so that the twin and the model are not merely alike."""
    ins = "ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATTCAGG"               # 40 letters
    m1, m2 = ins + "AGATCGGAAG", pc.revcomp(ins) + "CTGTCTCTTA"
    q = b"I" * 50
    span = lambda **kw: salt_amd.trim_pair_span(m1.encode(), q, m2.encode(), q, **kw)
    assert span() == (0, 40, 0, 40)
    assert span(pair=False) == (0, 50, 0, 50)
    assert span(min_overlap=40) == (0, 40, 0, 40) and span(min_overlap=41) == (0, 50, 0, 50)
    assert span(front=5) == (5, 40, 5, 40)                          # 30 columns are compared: 5 .. 34
    assert span(front=5, min_overlap=31) == (5, 50, 5, 50)
    assert span(front=45) == (45, 50, 45, 50)                       # at most five columns are compared
    # an insert longer than the mates: counted, nothing cut
    long_ins = ins + "TTGACCATGCAGTCAAGCTT"                         # 60
    pcnt = np.zeros(8, dtype=np.uint64)
    assert salt_amd.trim_pair_span(long_ins[:50].encode(), q, pc.revcomp(long_ins)[:50].encode(), q, pair_counts=pcnt) == (0, 50, 0, 50)
    assert dict(zip(pc.COUNTERS, pcnt)) == dict(pairs=1, overlapping=1, trimmed=0, reads1=0, bases1=0, reads2=0, bases2=0, skipped_long=0)
    # two mismatches in 40 columns pass 10 % and fail 4 %
    bad = m1[:3] + tc._other(m1[3]) + m1[4:20] + tc._other(m1[20]) + m1[21:]
    assert salt_amd.trim_pair_span(bad.encode(), q, m2.encode(), q) == (0, 40, 0, 40)
    assert salt_amd.trim_pair_span(bad.encode(), q, m2.encode(), q, error_pct=4) == (0, 50, 0, 50)
    # unequal mates: mate 2 of 30 letters shares columns 10 .. 39 with mate 1
    assert salt_amd.trim_pair_span(m1.encode(), q, m2[:30].encode(), q[:30]) == (0, 40, 0, 30)
    # mate 1 cut to nothing by its qualities: no column is compared, the floor keeps one base of it
    assert salt_amd.trim_pair_span(m1.encode(), b"#" * 50, m2.encode(), q, qual_min=20) == (0, 1, 0, 50)
    # homopolymers: every layout matches, the largest is taken and nothing is cut
    assert salt_amd.trim_pair_span(b"A" * 50, q, b"T" * 50, q) == (0, 50, 0, 50)


def test_the_counters_of_both_kinds():
    ins = "ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATTCAGG"
    ad = "AGATCGGAAGAGC"
    m1, m2 = ins + ad[:10], pc.revcomp(ins)[:35]
    counts, pcnt = _new_counts()
    # mate 1: L 50, the pair step takes 10; mate 2: L 35, nothing to take; the adapter step then finds nothing in either
    assert salt_amd.trim_pair_span(m1.encode(), b"I" * 50, m2.encode(), b"I" * 35, adapter=ad, counts=counts, pair_counts=pcnt) == (0, 40, 0, 35)
    assert dict(zip(pc.COUNTERS, pcnt)) == dict(pairs=1, overlapping=1, trimmed=1, reads1=1, bases1=10, reads2=0, bases2=0, skipped_long=0)
    assert dict(zip(tc.COUNTERS, counts[0])) == dict(reads=1, bases_in=50, bases_out=40, reads_qual=0, bases_qual=0, reads_adapter=0, bases_adapter=0, reads_floored=0)
    assert dict(zip(tc.COUNTERS, counts[1])) == dict(reads=1, bases_in=35, bases_out=35, reads_qual=0, bases_qual=0, reads_adapter=0, bases_adapter=0, reads_floored=0)
    # the pair rule off: the adapter step takes the ten itself
    counts, pcnt = _new_counts()
    assert salt_amd.trim_pair_span(m1.encode(), b"I" * 50, m2.encode(), b"I" * 35, pair=False, adapter=ad, counts=counts, pair_counts=pcnt) == (0, 40, 0, 35)
    assert pcnt.sum() == 0 and counts[0][tc.COUNTERS.index("bases_adapter")] == 10
    assert salt_amd.TRIM_PAIR_COUNTERS == pc.COUNTERS


def test_with_the_pair_rule_off_each_mate_is_trim_spans():
    o, reads = tc.random_block(400, seed=2)
    kw = dict(adapter=o["adapter"], adapter2=o["adapter2"], front=o["front"], tail=o["tail"])
    a, b = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
    for r1, r2 in zip(reads[0::2], reads[1::2]):
        span = salt_amd.trim_pair_span(r1[0], r1[1], r2[0], r2[1], pair=False, qual_min=o["qual"], counts=a, **kw)
        assert span == salt_amd.trim_span(r1[0], r1[1], mate=0, qual_min=o["qual"], counts=b, **kw) + salt_amd.trim_span(r2[0], r2[1], mate=1, qual_min=o["qual"], counts=b, **kw)
    assert (a == b).all()


@pytest.mark.parametrize("kw, word", [(dict(min_overlap=0), "min_overlap"), (dict(min_overlap=513), "min_overlap"), (dict(error_pct=51), "error_pct"),
                                      (dict(min_overlap=0, error_pct=0), "min_overlap"), (dict(front=512), "front"), (dict(adapter="ACGN"), "adapter holds")])
def test_options_out_of_range_are_refused_by_name(kw, word):
    with pytest.raises(salt_amd.SaltError, match=word):
        salt_amd.trim_fastq_pair(b"@r\nACGT\n+\nIIII\n", b"@r\nACGT\n+\nIIII\n", **kw)
    with pytest.raises(salt_amd.SaltError, match=word):
        salt_amd.trim_pair_span(b"ACGT", b"IIII", b"ACGT", b"IIII", **kw)


@pytest.mark.parametrize("b1, b2, word", [(b"@r\nACGT\n+\nIII\n", b"@r\nACGT\n+\nIIII\n", "block 1: sequence and quality lengths differ"),
                                          (b"@r\nACGT\n+\nIIII\n", b"r\nACGT\n+\nIIII\n", "block 2: a record does not start"),
                                          (b"@r\nACGT\n+\nIIII\n", b"@r\nACGT\n+\nIIII\n@s\nA\n+\nI\n", "different numbers"),
                                          (b"@r\nACGT\n+\nIIII\n", b"", "different numbers"), (b"@r\nACGT\n+\nIIII", b"@r\nACGT\n+\nIIII\n", "whole 4-line")])
def test_trim_fastq_pair_refuses_what_is_not_paired_four_line_fastq(b1, b2, word):
    with pytest.raises(salt_amd.SaltError, match=word):
        salt_amd.trim_fastq_pair(b1, b2)


def test_trim_fastq_pair_keeps_header_and_plus_lines():
    ins = "ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATTCAGG"
    b1 = b"@p1 x/1\n" + (ins + "AGATC").encode() + b"\n+p1\n" + b"I" * 45 + b"\n"
    b2 = b"@p1 x/2\n" + (pc.revcomp(ins) + "CTGTC").encode() + b"\n+\n" + b"F" * 45 + b"\n"
    assert salt_amd.trim_fastq_pair(b1, b2, pair=False) == (b1, b2)
    assert salt_amd.trim_fastq_pair(b1, b2) == (b"@p1 x/1\n" + ins.encode() + b"\n+p1\n" + b"I" * 40 + b"\n", b"@p1 x/2\n" + pc.revcomp(ins).encode() + b"\n+\n" + b"F" * 40 + b"\n")
    assert salt_amd.trim_fastq_pair(b"", b"") == (b"", b"")
