"""The host twin of the trim kernel (salt_trim_span, salt_trim_fastq: salt_amd/csrc/salt_trim_rule.h compiled for the host) against the
plain Python statement of the rule in trim_check.py, on the edge-case set and on a seeded random block.  No GPU."""
import numpy as np
import pytest

import salt_amd
import trim_check as tc


def _twin_spans(o, mate, reads, counts=None):
    return [salt_amd.trim_span(s, q, mate=mate, adapter=o["adapter"], adapter2=o["adapter2"], qual_min=o["qual"], front=o["front"], tail=o["tail"],
                               min_overlap=o["min_overlap"], error_pct=o["error_pct"], counts=counts) for s, q in reads]


@pytest.fixture(scope="module")
def groups():
    return tc.group(tc.edge_cases())


def test_the_edge_case_set_is_what_it_is_meant_to_be(groups):
    """The set reaches every step and the floor, on both mates, and the model's spans are spans."""
    counts = np.zeros((2, 8), dtype=np.uint64)
    n = 0
    for o, mate, reads in groups:
        for s, q in reads:
            b, e = tc.model_span(o, mate, s, q, counts)
            assert 0 <= b < e <= len(s)
            n += 1
    assert n > 3000 and len(groups) < 400
    for mate in (0, 1):
        c = dict(zip(tc.COUNTERS, counts[mate]))
        assert c["reads_adapter"] > 0 and c["reads_qual"] > 0 and c["bases_in"] > c["bases_out"] > 0
    assert counts[0][tc.COUNTERS.index("reads_floored")] > 50


def test_span_equals_the_model_on_every_edge_case(groups):
    want_counts, got_counts = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
    for o, mate, reads in groups:
        want = [tc.model_span(o, mate, s, q, want_counts) for s, q in reads]
        got = _twin_spans(o, mate, reads, got_counts)
        bad = [(i, reads[i], want[i], got[i]) for i in range(len(reads)) if want[i] != got[i]]
        assert not bad, (o, mate, bad[:3])
    assert (want_counts == got_counts).all(), (want_counts, got_counts)


def test_span_equals_the_model_on_the_random_block():
    o, reads = tc.random_block(4000, seed=11)
    for mate in (0, 1):
        want_counts, got_counts = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
        want = [tc.model_span(o, mate, s, q, want_counts) for s, q in reads]
        assert _twin_spans(o, mate, reads, got_counts) == want
        assert (want_counts == got_counts).all()
        assert want_counts[mate][0] == len(reads) and want_counts[1 - mate].sum() == 0


def test_known_spans():
    """A few spans worked out by hand, so that the twin and the model are not merely alike."""
    ad = "AGATCGGAAGAGC"
    read = b"ACGTACGTAC" + ad.encode() + b"TTT"
    assert salt_amd.trim_span(read, b"I" * 26, adapter=ad) == (0, 10)
    assert salt_amd.trim_span(read, b"I" * 26, adapter=ad, front=2, tail=1) == (2, 10)
    assert salt_amd.trim_span(ad.encode() + b"ACGT", b"I" * 17, adapter=ad) == (0, 1)               # adapter at 0: the floor
    assert salt_amd.trim_span(b"ACGTACGTAC" + b"AGATC", b"I" * 15, adapter=ad) == (0, 10)            # an overlap of 5 = M
    assert salt_amd.trim_span(b"ACGTACGTAC" + b"AGAT", b"I" * 14, adapter=ad) == (0, 14)             # of 4: below M
    assert salt_amd.trim_span(b"ACGTACGTAC" + b"AGAT", b"I" * 14, adapter=ad, min_overlap=4) == (0, 10)
    one_off = b"ACGTACGTAC" + b"AGATCGGTAGAGC"                                                         # 1 of 13: 100 > 130 is false
    assert salt_amd.trim_span(one_off, b"I" * 23, adapter=ad) == (0, 10)
    assert salt_amd.trim_span(one_off, b"I" * 23, adapter=ad, error_pct=7) == (0, 23)                # 100 <= 91 is false
    assert salt_amd.trim_span(b"ACGTACGTAC", b"IIIII#####", qual_min=20) == (0, 5)
    assert salt_amd.trim_span(b"ACGTACGTAC", b"IIII##I###", qual_min=20) == (0, 4)                   # 18 x 3 - 20 + 18 x 2 > 18 x 3: past the high base
    assert salt_amd.trim_span(b"ACGTACGTAC", b"##########", qual_min=20) == (0, 1)
    assert salt_amd.trim_span(b"ACGTACGTAC", b"IIIIIIIIII", front=7, tail=7) == (7, 8)
    assert salt_amd.trim_span(b"ACGTACGTAC", b"IIIIIIIIII", front=300) == (9, 10)


def test_mate_2_takes_its_own_adapter_or_mate_1s():
    s1, s2 = b"ACGTACGTAC" + tc.ADAPTER.encode(), b"ACGTACGTAC" + tc.ADAPTER2.encode()
    q = b"I" * len(s1)
    both = dict(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2)
    assert salt_amd.trim_span(s1, q, mate=0, **both) == (0, 10) and salt_amd.trim_span(s2, q, mate=1, **both) == (0, 10)
    assert salt_amd.trim_span(s1, q, mate=1, error_pct=0, **both) == (0, 43) and salt_amd.trim_span(s2, q, mate=0, error_pct=0, **both) == (0, 43)
    assert salt_amd.trim_span(s1, q, mate=1, adapter=tc.ADAPTER) == (0, 10)


def test_the_sixteen_counters():
    counts = np.zeros((2, 8), dtype=np.uint64)
    ad = "AGATCGGAAGAGC"
    salt_amd.trim_span(b"ACGTACGTAC" + ad.encode() + b"TTT", b"I" * 21 + b"#" * 5, adapter=ad, qual_min=20, front=1, tail=1, counts=counts)
    # L 26; clips leave [1, 25); quality takes the four '#' left: end 21; the adapter at 10: end 10
    assert dict(zip(tc.COUNTERS, counts[0])) == dict(reads=1, bases_in=26, bases_out=9, reads_qual=1, bases_qual=4, reads_adapter=1, bases_adapter=11, reads_floored=0)
    assert counts[1].sum() == 0
    salt_amd.trim_span(ad.encode(), b"I" * 13, mate=1, adapter=ad, counts=counts)
    assert dict(zip(tc.COUNTERS, counts[1])) == dict(reads=1, bases_in=13, bases_out=1, reads_qual=0, bases_qual=0, reads_adapter=1, bases_adapter=13, reads_floored=1)
    assert counts[0][0] == 1 and salt_amd.TRIM_COUNTERS == tc.COUNTERS


@pytest.mark.parametrize("cr", [False, True])
def test_trim_fastq_equals_the_model(cr):
    o, reads = tc.random_block(600, seed=3)
    block = tc.fastq_of(reads, cr=cr)
    for mate in (0, 1):
        want_counts, got_counts = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
        want = tc.model_fastq(o, mate, block, want_counts)
        got = salt_amd.trim_fastq(block, mate=mate, counts=got_counts, **o)
        assert got == want and b"\r" not in got
        assert (want_counts == got_counts).all()


def test_trim_fastq_keeps_header_and_plus_lines_and_without_options_the_reads():
    block = b"@r1 some comment/1\nACGTACGTACGT\n+r1\nIIIIIIII####\n@r2\nAC\n+\nII\n"
    assert salt_amd.trim_fastq(block) == block
    assert salt_amd.trim_fastq(block, qual=20) == b"@r1 some comment/1\nACGTACGT\n+r1\nIIIIIIII\n@r2\nAC\n+\nII\n"
    assert salt_amd.trim_fastq(b"") == b""


@pytest.mark.parametrize("kw, word", [
    (dict(adapter="ACGN"), "adapter holds a letter"), (dict(adapter="A" * 65), "adapter longer"), (dict(adapter="ACGT", adapter2="AC-T"), "adapter2 holds"),
    (dict(adapter2="ACGT"), "adapter2 without adapter"), (dict(adapter="ACGT", min_overlap=0), "min_overlap"), (dict(adapter="ACGT", min_overlap=65), "min_overlap"),
    (dict(adapter="ACGT", error_pct=51), "error_pct"), (dict(qual=94), "qual"), (dict(front=512), "front"), (dict(tail=512), "tail")])
def test_options_out_of_range_are_refused_by_name(kw, word):
    with pytest.raises(salt_amd.SaltError, match=word):
        salt_amd.trim_fastq(b"@r\nACGT\n+\nIIII\n", **kw)


@pytest.mark.parametrize("block, word", [(b"@r\nACGT\n+\nIII\n", "lengths differ"), (b"r\nACGT\n+\nIIII\n", "'@'"), (b"@r\nACGT\n-\nIIII\n", "'\\+'"),
                                         (b"@r\n\n+\n\n", "empty read"), (b"@r\nACGT\n+\nIIII", "whole 4-line"), (b"@r\nACGT\n+\n", "whole 4-line")])
def test_trim_fastq_refuses_what_is_not_four_line_fastq(block, word):
    with pytest.raises(salt_amd.SaltError, match=word):
        salt_amd.trim_fastq(block, qual=20)
