"""Indel candidates without a GPU: the host twin and its printer (salt_indel_add_sam, salt_indel_text, salt_indel_header) against the Python
statement (tests/indel_check.py) on the lambda goldens, on hand-made SAM lines over the two_contigs index that hold every case of the
event rule and of the left shift, on a synthetic genome that is one long run (the shift's cap), and on hand-made entries that hold every
case of the call rule and of the line."""
import os
import random

import numpy as np
import pytest

import gap_cases
import indel_check
import snp_check
from conftest import GOLDEN

PLAIN = {"se_default": "expect_se_default.sam", "pe_default": "expect_pe_default.sam", "span_default": "expect_span_default.sam"}
GAP = ("gap_se_lane", "gap_se_mid", "gap_se_long", "gap_pe_short", "gap_pe_long")
# golden -> per floor (0, 20): (tabled, long, unanchored, distinct alleles), from the statement under the project's contig rule, as counted
# when the test was written (the issue's census, which read the two contigs as one string, had gap_se_mid at 1 220 / 0 / 155 / 1 194 and
# se_default at 267 / 46)
COUNTS = {
    "se_default": ((267, 0, 46, 267), (260, 0, 42, 260)), "pe_default": ((117, 0, 12, 117), (114, 0, 12, 114)), "span_default": ((7, 0, 1, 7), (7, 0, 1, 7)),
    "gap_se_lane": ((973, 0, 160, 956), (813, 0, 128, 796)), "gap_se_mid": ((1220, 0, 155, 1200), (1087, 0, 129, 1068)),
    "gap_se_long": ((801, 0, 81, 775), (635, 0, 62, 609)), "gap_pe_short": ((358, 0, 22, 358), (329, 0, 14, 329)), "gap_pe_long": ((354, 0, 25, 354), (336, 0, 15, 336)),
}


def golden_sam(case):
    return snp_check.golden_sam(PLAIN[case]) if case in PLAIN else gap_cases.golden(case)


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    from conftest import LAMBDA
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield salt_amd, ix, indel_check.Genome()
    ix.destroy()


@pytest.fixture(scope="module")
def two():
    import salt_amd
    prefix = os.path.join(GOLDEN, "index_cases", "two_contigs", "idx")
    ix = salt_amd.Index.reload(prefix)
    yield salt_amd, ix, indel_check.Genome(prefix)
    ix.destroy()


def test_the_defaults_are_the_definitions():
    import salt_amd
    assert salt_amd.INDEL_DEFAULTS == indel_check.DEFAULTS == dict(min_mapq=20, min_alt=3, min_pct=20, log2_slots=24)
    assert (salt_amd.INDEL_MAX_INS, salt_amd.INDEL_MAX_DEL, salt_amd.INDEL_MAX_SHIFT, salt_amd.INDEL_PROBE) == (12, 63, 4096, 128)
    assert (indel_check.MAX_INS, indel_check.MAX_DEL, indel_check.MAX_SHIFT, indel_check.PROBE) == (12, 63, 4096, 128)
    assert salt_amd.INDEL_STATS == ("tabled", "dropped", "long", "unanchored")


@pytest.mark.parametrize("case", sorted(COUNTS))
def test_twin_and_printer_equal_the_python_statement(case, lam):
    salt_amd, ix, genome = lam
    sam = golden_sam(case)
    for k, mq in enumerate((0, 20, 255)):
        cs = {}
        table, stats, diff, n = indel_check.add_sam(genome, sam, mq, cs)
        got, got_diff, got_stats, got_n = salt_amd.indel_add_sam(ix, sam, mq)
        want = indel_check.entries(table)
        print(case, mq, n, stats, len(table), cs)
        assert got_n == n and got_stats.tolist() == stats and np.array_equal(got, want) and np.array_equal(got_diff, diff)
        assert (stats[0], stats[2], stats[3], len(table)) == ((0, 0, 0, 0) if mq == 255 else COUNTS[case][k]) and stats[1] == 0
        # an identity that does not depend on the rule: every I and D op of a counted record goes to exactly one counter
        ops = sum(line.split(b"\t")[5].count(b"I") + line.split(b"\t")[5].count(b"D") for line in sam.split(b"\n")
                  if line and not line.startswith(b"@") and not int(line.split(b"\t")[1]) & 4 and int(line.split(b"\t")[4]) >= mq)
        assert stats[0] + stats[2] + stats[3] == ops == cs["ops"] and sum(sum(v) for v in table.values()) == stats[0]
        if case == "gap_se_mid" and mq == 0:
            assert ops == 694 + 681
        # the tally's own difference array is the coverage's rule under this tally's floor
        import depth_check
        assert np.array_equal(got_diff, depth_check.diff_of_sam(depth_check.lambda_contigs(), sam, mq)[0])
        # keys in order, all well-formed; the sam in two halves into one table gives the same
        assert all(int(a) < int(b) for a, b in zip(got[:-1, 0], got[1:, 0])) and all(indel_check.well_formed(int(key), len(genome.masks)) for key in got[:, 0])
        for min_alt, min_pct in ((1, 0), (2, 10), (3, 20)):
            assert salt_amd.indel_text(ix, got, got_diff, min_alt, min_pct) == indel_check.text(genome, want, diff, min_alt, min_pct)
    lines = sam.split(b"\n")
    halves = [b"\n".join(lines[:len(lines) // 2]) + b"\n", b"\n".join(lines[len(lines) // 2:])]
    whole, parts = salt_amd.indel_add_sam(ix, sam, 0), salt_amd.indel_add_sam(ix, halves, 0)
    assert all(np.array_equal(a, b) for a, b in zip(whole[:3], parts[:3])) and whole[3] == parts[3]


@pytest.mark.parametrize("case", GAP)
def test_the_gap_goldens_need_the_normalisation(case, lam):
    """On every gap golden insertions and deletions move under the left shift: tabled where the CIGAR has them, one allele would be
    several.  Alleles seen more than once: in each single-end gap golden (up to 8 times); the paired-end goldens show every allele once
    (358 and 354 alleles of 358 and 354 events at floor 0), so there the count is asserted over the gap goldens together."""
    salt_amd, ix, genome = lam
    cs = {}
    table, stats, _, _ = indel_check.add_sam(genome, golden_sam(case), 0, cs)
    most = max(sum(v) for v in table.values())
    print(case, cs, "largest count", most)
    assert cs["moved_ins"] >= 1 and cs["moved_del"] >= 1 and cs["max_steps"] < indel_check.MAX_SHIFT
    if case == "gap_se_mid":
        assert most == 8 and cs["moved"] == 453                        # (the issue's census: 8 and 449)
    if case.startswith("gap_se"):
        assert most > 1
    assert max(max(sum(v) for v in indel_check.add_sam(genome, golden_sam(c), 0)[0].values()) for c in GAP) > 1
    both = [k for k, v in table.items() if v[0] and v[1]]
    assert case.startswith("gap_pe") or both                           # alleles seen on both strands


# ---- hand-made lines ----
def make_line(genome, contig, pos1, ops, flag=0, mapq=60, name="r"):
    """a SAM line whose M runs copy the genome: ops = [("M", n) | ("I", "ACGT letters") | ("D", n) | ("S", n)]"""
    g, seq, cigar = genome.offsets[contig] + pos1 - 1, "", ""
    for op, x in ops:
        n = len(x) if op == "I" else x
        cigar += "%d%s" % (n, op)
        if op == "M":
            seq += "".join("ACGT"[indel_check.letter(genome, g + k)] for k in range(n))
            g += n
        elif op == "I":
            seq += x
        elif op == "D":
            g += n
        else:
            seq += "A" * n
    return ("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*\n" % (name, flag, contig, pos1, mapq, cigar, seq)).encode()


def both(salt_amd, ix, genome, sam, mq=0):
    """the twin's (entries, diff, stats), checked against the statement; with the statement's table"""
    table, stats, diff, n = indel_check.add_sam(genome, sam, mq)
    got, got_diff, got_stats, got_n = salt_amd.indel_add_sam(ix, sam, mq)
    assert got_n == n and got_stats.tolist() == stats and np.array_equal(got, indel_check.entries(table)) and np.array_equal(got_diff, diff)
    assert salt_amd.indel_text(ix, got, got_diff, 1, 0) == indel_check.text(genome, got, diff, 1, 0)
    return table, stats, diff


def letters(genome, a, b):
    return "".join("ACGT"[indel_check.letter(genome, x)] for x in range(a, b))


def test_ops_that_are_no_events(two):
    salt_amd, ix, genome = two
    for ops in ([("I", "AC"), ("M", 30)], [("M", 30), ("I", "AC")], [("D", 2), ("M", 30)], [("M", 30), ("D", 2)],      # first op, last op
                [("S", 5), ("I", "AC"), ("M", 30)], [("S", 5), ("D", 3), ("M", 30)], [("M", 30), ("I", "G"), ("S", 4)],      # directly behind S, in front of S
                [("M", 20), ("I", "AC"), ("D", 2), ("M", 20)], [("M", 20), ("D", 2), ("I", "AC"), ("M", 20)]):      # I next to D
        table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "a", 101, ops))
        gaps = sum(1 for op, _ in ops if op in "ID")
        assert stats == [0, 0, 0, gaps] and not table
    # the lengths: I of 12 and D of 63 are events, 13 and 64 are long (whatever else holds); 0 is long too
    for ops, want in (([("M", 20), ("I", "ACGTACGTACGT"), ("M", 20)], [1, 0, 0, 0]), ([("M", 20), ("I", "ACGTACGTACGTA"), ("M", 20)], [0, 0, 1, 0]),
                      ([("M", 20), ("D", 63), ("M", 20)], [1, 0, 0, 0]), ([("M", 20), ("D", 64), ("M", 20)], [0, 0, 1, 0]),
                      ([("I", "ACGTACGTACGTA"), ("M", 20)], [0, 0, 1, 0]), ([("M", 20), ("D", 0), ("M", 20)], [0, 0, 1, 0])):
        table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "a", 101, ops))
        assert stats == want and len(table) == want[0]
        if want[0]:
            g, is_del, n, bases = indel_check.key_parts(next(iter(table)))
            assert n == (63 if is_del else 12) and g <= 120
    # an inserted N
    table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "a", 101, [("M", 20), ("I", "ANC"), ("M", 20)]))
    assert stats == [0, 0, 0, 1]
    # a reverse record counts into the high half, a record below the floor not at all
    ops = [("M", 20), ("I", "ACG"), ("M", 20)]
    sam = make_line(genome, "a", 101, ops) + make_line(genome, "a", 101, ops, flag=16) + make_line(genome, "a", 101, ops, flag=16) + make_line(genome, "a", 101, ops, mapq=19)
    table, stats, _ = both(salt_amd, ix, genome, sam, 20)
    assert stats == [3, 0, 0, 0] and list(table.values()) == [[1, 2]]


def test_a_deletion_at_a_contigs_end_and_a_line_cut_at_ref_len(two):
    salt_amd, ix, genome = two
    (_, off_a, len_a), (_, off_c, len_c) = genome.contigs
    assert (off_a, len_a, off_c, len_c) == (0, 500, 500, 300) and len(genome.masks) == 800
    for contig, length in (("a", len_a), ("c", len_c)):
        # the deletion's last base is the contig's last base: an event; one base further: unanchored (the M run behind it lies in the next contig or beyond the genome)
        inside = make_line(genome, contig, length - 30, [("M", 20), ("D", 11), ("M", 5)])       # D covers 1-based [length - 10, length]
        beyond = make_line(genome, contig, length - 30, [("M", 20), ("D", 12), ("M", 5)])
        table, stats, diff = both(salt_amd, ix, genome, inside)
        assert stats == [1, 0, 0, 0]
        g, is_del, n, _ = indel_check.key_parts(next(iter(table)))
        assert is_del and n == 11 and g + n <= genome.offsets[contig] + length
        table, stats, diff = both(salt_amd, ix, genome, beyond)
        assert stats == [0, 0, 0, 1] and not table
    # an insertion whose anchor is contig a's last base: g is contig c's first position, not inside a
    table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "a", len_a - 19, [("M", 20), ("I", "AC"), ("M", 10)]))
    assert stats == [0, 0, 0, 1]
    # a line that runs past ref_len: its M run is cut in diff, not refused, and its indel is tabled
    line = make_line(genome, "c", len_c - 29, [("M", 10), ("I", "ACG"), ("M", 30)])
    table, stats, diff = both(salt_amd, ix, genome, line)
    assert stats == [1, 0, 0, 0] and int(diff[800]) == 0xFFFFFFFF and int(diff[770]) == 1 and int(diff[780]) == 0 and int(np.asarray(diff, dtype=np.uint64).sum() % (1 << 32)) == 0


def test_the_left_shift(two):
    salt_amd, ix, genome = two
    assert letters(genome, 0, 4) == "GGGC"
    # a homopolymer at the contig's start: the deletion of one G shifts until its anchor is the contig's first position, and stops
    table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "a", 1, [("M", 2), ("D", 1), ("M", 30)]))
    assert [indel_check.key_parts(k) for k in table] == [(1, True, 1, [])]
    table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "a", 1, [("M", 1), ("D", 1), ("M", 30)]))       # already there
    assert [indel_check.key_parts(k) for k in table] == [(1, True, 1, [])]
    table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "a", 1, [("M", 2), ("I", "G"), ("M", 30)]))
    assert [indel_check.key_parts(k) for k in table] == [(1, False, 1, [2])]
    # the same at contig c's start: the anchor stays on c's first position, 500
    run = 1
    while indel_check.letter(genome, 500 + run) == indel_check.letter(genome, 500):
        run += 1
    base = indel_check.letter(genome, 500)
    table, stats, _ = both(salt_amd, ix, genome, make_line(genome, "c", 1, [("M", run), ("I", "ACGT"[base]), ("M", 30)]))
    assert [indel_check.key_parts(k) for k in table] == [(501, False, 1, [base])]
    # the same deletion written at every position of a repeat gives one key: the first run of at least four equal letters behind position 20
    text = letters(genome, 0, 500)
    at = next(x for x in range(20, 400) if len(set(text[x:x + 4])) == 1 and text[x - 1] != text[x])
    length = next(k for k in range(4, 100) if text[at + k] != text[at])
    sam = b"".join(make_line(genome, "a", at - 14, [("M", 15 + k), ("D", 1), ("M", 30)], flag=16 * (k & 1)) for k in range(length))
    table, stats, _ = both(salt_amd, ix, genome, sam)
    assert stats == [length, 0, 0, 0] and [indel_check.key_parts(k) for k in table] == [(at, True, 1, [])] and list(table.values()) == [[(length + 1) // 2, length // 2]]
    # ... and so does a two-base deletion in a dinucleotide repeat, and the insertion of one more unit, whose bases rotate
    at = next(x for x in range(20, 400) if text[x:x + 2] == text[x + 2:x + 4] and text[x] != text[x + 1] and text[x - 2:x] != text[x:x + 2] and text[x - 1] != text[x + 1])
    unit, reps = text[at:at + 2], next(k for k in range(2, 50) if text[at + 2 * k:at + 2 * k + 2] != text[at:at + 2])
    span = 2 * reps + (1 if text[at + 2 * reps] == unit[0] else 0)
    sam = b"".join(make_line(genome, "a", at - 14, [("M", 15 + k), ("D", 2), ("M", 30)]) for k in range(span - 1))
    table, stats, _ = both(salt_amd, ix, genome, sam)
    assert [indel_check.key_parts(k) for k in table] == [(at, True, 2, [])] and list(table.values()) == [[span - 1, 0]]
    ins = [make_line(genome, "a", at - 14, [("M", 15 + k), ("I", (unit * 2)[k & 1:(k & 1) + 2]), ("M", 30)]) for k in range(0, span + 1)]
    table, stats, _ = both(salt_amd, ix, genome, b"".join(ins))
    want = (at, False, 2, ["ACGT".index(unit[0]), "ACGT".index(unit[1])])
    assert [indel_check.key_parts(k) for k in table] == [want] and list(table.values()) == [[span + 1, 0]]
    assert indel_check.normalise(genome, at + span, False, 2, want[3] if span % 2 == 0 else want[3][::-1])[2] == span      # the bases went round span times


def test_the_shift_is_cut_at_4096(tmp_path):
    """a synthetic single-contig genome that is one long run: the cap on the shift's work is part of the definition"""
    import salt_amd
    rng = random.Random(5)
    tail = "".join(rng.choice("ACGT") for _ in range(300))
    (tmp_path / "g.fa").write_text(">run\nC" + "A" * 6000 + tail + "\n")
    (tmp_path / "s.txt").write_text("run\t6100\t%s/%s\t%s\n" % (tail[98], "ACGT"[("ACGT".index(tail[98]) + 1) % 4], tail[98]))
    salt_amd.idx_build(str(tmp_path / "g.fa"), str(tmp_path / "s.txt"), str(tmp_path / "idx"), 19)
    ix, genome = salt_amd.Index.reload(str(tmp_path / "idx")), indel_check.Genome(str(tmp_path / "idx"))
    try:
        for pos1, want_g in ((5981, 5990 - 4096), (4087, 1), (4088, 1), (4089, 2)):      # the cap binds; the contig's start binds (4 095 and 4 096 steps away); the cap binds one step short of it
            for ops, is_del in (([("M", 10), ("D", 1), ("M", 30)], True), ([("M", 10), ("I", "A"), ("M", 30)], False)):
                cs = {}
                line = make_line(genome, "run", pos1, ops)
                table, stats, _, _ = indel_check.add_sam(genome, line, 0, cs)
                got = salt_amd.indel_add_sam(ix, line, 0)
                assert np.array_equal(got[0], indel_check.entries(table)) and got[2].tolist() == stats == [1, 0, 0, 0]
                g = indel_check.key_parts(next(iter(table)))[0]
                assert g == want_g and cs["max_steps"] == min(4096, pos1 + 8)
    finally:
        ix.destroy()


# ---- the text ----
def diff_of_depth(depth):
    n = len(depth)
    diff = np.zeros(n + 1, dtype=np.int64)
    diff[0], diff[1:n], diff[n] = depth[0], depth[1:] - depth[:-1], -depth[n - 1]
    return (diff % (1 << 32)).astype(np.uint32)


def test_hand_made_entries_hold_every_case_of_the_call_and_of_the_line(two):
    salt_amd, ix, genome = two
    n = len(genome.masks)
    depth = np.zeros(n, dtype=np.int64)
    K, V = indel_check.key_of, lambda fwd, rev: fwd | rev << 32
    cases = [  # (key, value, depth at the anchor, called at 3 / 20)
        (K(41, True, 3), V(2, 2), 20, True), (K(42, True, 3), V(2, 2), 21, False),          # 100 n == min_pct depth exactly, and one short of it
        (K(51, False, 2, [0, 3]), V(1, 1), 2, False),                                        # below min_alt
        (K(61, False, 1, [2]), V(3, 0), 0, True),                                            # depth 0 with a count
        (K(71, True, 1), V(5, 0), 10, True), (K(71, False, 1, [1]), V(0, 5), 10, True),      # forward only, reverse only; two alleles at one anchor, I sorts in front of D
        (K(101, True, 63), V(4, 4), 8, True),                                                # a 63-base deletion's REF
        (K(111, False, 12, [0, 1, 2, 3] * 3), V(3, 3), 6, True),                             # a 12-base insertion's ALT
        (K(1, True, 2), V(9, 0), 9, True), (K(500, False, 1, [3]), V(9, 0), 9, True),        # anchors on a's first and last position
        (K(501, True, 1), V(0, 9), 9, True), (K(799, True, 1), V(9, 9), 18, True),           # on c's first position; the genome's last deletable base
        (K(81, True, 1), V(0xFFFFFFFF, 0xFFFFFFFF), 0xFFFFFFFF, True),                       # the largest numbers of a line
    ]
    for key, _, d, _ in cases:
        depth[indel_check.key_parts(key)[0] - 1] = d
    diff = diff_of_depth(depth)
    pairs = np.array(sorted((k, v) for k, v, _, _ in cases), dtype=np.uint64)
    want = indel_check.text(genome, pairs, diff)
    assert salt_amd.indel_text(ix, pairs, diff) == want
    rows = indel_check.parse(want)
    assert len(rows) == sum(1 for c in cases if c[3])
    by = {(r[0], r[1], r[4]["TYPE"]): r for r in rows}
    assert ("a", 41, "DEL") in by and ("a", 42, "DEL") not in by and ("a", 51, "INS") not in by and by["a", 61, "INS"][4]["DP"] == 0
    assert by["a", 71, "DEL"][4] == dict(TYPE="DEL", LEN=1, DP=10, AO=5, AOF=5, AOR=0) and by["a", 71, "INS"][4] == dict(TYPE="INS", LEN=1, DP=10, AO=5, AOF=0, AOR=5)
    assert [r[4]["TYPE"] for r in rows if r[:2] == ("a", 71)] == ["INS", "DEL"]
    r = by["a", 101, "DEL"]
    assert r[2] == letters(genome, 100, 164) and r[3] == r[2][0] and len(r[2]) == 64
    r = by["a", 111, "INS"]
    assert r[2] == letters(genome, 110, 111) and r[3] == r[2] + "ACGT" * 3
    assert by["a", 1, "DEL"][2] == letters(genome, 0, 3) and by["a", 500, "INS"][3] == letters(genome, 499, 500) + "T"
    assert by["c", 1, "DEL"][2] == letters(genome, 500, 502) and by["c", 299, "DEL"][2] == letters(genome, 798, 800)
    assert by["a", 81, "DEL"][4]["AO"] == 2 * 0xFFFFFFFF and by["a", 81, "DEL"][4]["DP"] == 0xFFFFFFFF
    # with the floor at 1 / 0 every pair has a line; words that are no well-formed keys and values of 0 never have
    assert len(indel_check.parse(salt_amd.indel_text(ix, pairs, diff, 1, 0))) == len(cases)
    odd = np.array(sorted([(K(41, True, 3) & ~(1 << 63), 9), (K(0, True, 1), 9), (K(801, True, 1), 9), (K(90, False, 13), 9), (K(90, False, 0), 9), (K(91, True, 0), 9),
                           (K(92, False, 2, [1, 1]) | 1, 9), (K(93, True, 2) | 1 << 20, 9), (K(94, True, 2), 0), (K(800, False, 1, [0]), 9)]), dtype=np.uint64)
    text = salt_amd.indel_text(ix, odd, diff, 1, 0)
    assert text == indel_check.text(genome, odd, diff, 1, 0) and [(r[0], r[1]) for r in indel_check.parse(text)] == [("c", 300)]
    with pytest.raises(salt_amd.SaltError, match="key order"):
        salt_amd.indel_text(ix, pairs[::-1], diff)
    with pytest.raises(salt_amd.SaltError, match="min_alt"):
        salt_amd.indel_text(ix, pairs, diff, 0, 20)
    with pytest.raises(salt_amd.SaltError, match="positions"):
        salt_amd.indel_text(ix, pairs, diff[:-1])
    assert salt_amd.indel_text(ix, np.zeros((0, 2), dtype=np.uint64), diff) == b""


def test_the_header(two, lam):
    salt_amd, ix, genome = two
    h = salt_amd.indel_header(ix, 20, 3, 20, 7)
    assert h == indel_check.header(genome, 20, 3, 20, 7)
    lines = h.decode().split("\n")
    assert lines[0] == "##fileformat=VCFv4.2" and "##contig=<ID=a,length=500>" in lines and "##contig=<ID=c,length=300>" in lines
    assert "##salt_indels_dropped=7" in lines and "##salt_indels_parameters=<min_mapq=20,min_alt=3,min_pct=20>" in lines
    assert lines[-2] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" and lines[-1] == ""
    assert {l.split("ID=")[1].split(",")[0] for l in lines if l.startswith("##INFO")} == {"TYPE", "LEN", "DP", "AO", "AOF", "AOR"}
    salt_amd2, ix2, genome2 = lam
    assert salt_amd2.indel_header(ix2) == indel_check.header(genome2)


def test_a_bad_line_leaves_the_table_as_it_was(two):
    salt_amd, ix, genome = two
    good = make_line(genome, "a", 101, [("M", 20), ("D", 2), ("M", 20)])
    for bad in (good.replace(b"20M2D20M", b"20M2D21M"), good.replace(b"20M2D20M", b"20M2X20M"), good.replace(b"\ta\t", b"\tzz\t")):
        with pytest.raises(salt_amd.SaltError, match="indels: "):
            salt_amd.indel_add_sam(ix, good + bad)
