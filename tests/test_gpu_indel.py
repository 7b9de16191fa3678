"""Indel candidates on the device (salt --indels).  The table: k_indel_add behind every entry point that leaves result rows
against the host twin (salt_indel_add_sam) over the SAM text the same call returned and against the Python statement
(tests/indel_check.py) -- text and host-buffer calls, single and paired end, on the gap fixture's cases and on se_default; batch sizes
around the wave and the block; a hot allele; planted indels.  The insert routine through hand-made keys: the wrap at the table's end, a
probe run that is full, a table that overflows.  The state: two calls, a fork, reset, off, uncount, the errors.  The text kernels against
salt_indel_text byte for byte.  Then the `salt` binary with --indels."""
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import gap_cases
import indel_check
from bgzf_check import strip_pg
from conftest import LAMBDA, ROOT

pytestmark = pytest.mark.gpu

SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
REF_LEN, BOUND = 97004, 48502
SETS = dict({c: (a, [f + ".gz" for f in files]) for c, (a, files) in gap_cases.GAP_CASES.items()}, se_default=(["-d", "-c"], ["reads_se.fq"]))
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
K = indel_check.key_of


def _fq(name):
    data = open(os.path.join(LAMBDA, name), "rb").read()
    return gzip.decompress(data) if name.endswith(".gz") else data


def genome_letters():
    return b"".join(l.strip() for l in open(os.path.join(LAMBDA, "genome.fa"), "rb") if not l.startswith(b">")).upper()


def fastq_of(reads, qual=b"I"):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (name, seq, qual * len(seq)) for name, seq in reads)


def sam_records(sam):
    return [l.split(b"\t") for l in sam.split(b"\n") if l and not l.startswith(b"@")]


def _gunzip_members(data):
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        data = d.unused_data
    return b"".join(out)


def _opt(salt_amd, ix, args):
    return salt_amd.AlnOpt.from_argv(list(args), ix.l_seed)[0]


def new_aligner(salt_amd, ix, max_reads=8192):
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=max_reads, max_bases=max_reads * 160)
    aln.set_contigs(ix)
    return aln


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = new_aligner(salt_amd, ix)
    aln.indel_enable(True, 0, 16)                                      # 65 536 slots: the fixtures' alleles load it to 2 per cent
    aln.indel_enable(False, 0)
    yield salt_amd, ix, aln, indel_check.Genome()
    aln.close()
    ix.destroy()


def state(aln):
    return aln.indel_fetch(), aln.indel_fetch_diff(0, REF_LEN + 1), aln.indel_stats()


def check(what, got, want, events=True):
    for k, name in enumerate(("entries", "diff", "stats")):
        w = np.asarray(want[k])
        assert got[k].shape == w.shape, (what, name, got[k].shape, w.shape)
        if not np.array_equal(got[k], w):
            bad = np.flatnonzero((got[k] != w).reshape(len(w), -1).any(axis=1))
            raise AssertionError("%s: %d rows of %s differ; first at %s: device %s, twin %s" % (what, len(bad), name, bad[:3], got[k][bad[:3]].tolist(), w[bad[:3]].tolist()))
    assert not events or len(want[0])


def counted(aln, min_mapq, call):
    aln.indel_enable(True, min_mapq)
    aln.indel_reset()
    try:
        out = call()
        return out, state(aln)
    finally:
        aln.indel_enable(False, min_mapq)


def text_call(salt_amd, ix, aln, args, fqs, min_mapq=0):
    opt = _opt(salt_amd, ix, args)
    if len(fqs) == 1:
        return counted(aln, min_mapq, lambda: aln.align_se_text(opt, fqs[0])[0])
    return counted(aln, min_mapq, lambda: aln.align_pe_text(opt, ix, fqs[0], fqs[1])[0])


def statement(genome, sam, min_mapq=0):
    table, stats, diff, n = indel_check.add_sam(genome, sam, min_mapq)
    return indel_check.entries(table), diff, np.array(stats, dtype=np.uint64)


@pytest.fixture(scope="module")
def text_states(lam):
    """case -> (SAM of the text call, (entries, diff, stats) of that call at floor 0): computed once, shared"""
    salt_amd, ix, aln, _ = lam
    return {name: text_call(salt_amd, ix, aln, args, [_fq(f) for f in files]) for name, (args, files) in SETS.items()}


def test_before_the_first_enable_the_errors(lam):
    salt_amd, ix, _, _ = lam
    other = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    try:
        for call in (other.indel_reset, other.indel_stats, other.indel_fetch, lambda: other.indel_add(np.array([[K(5, True, 1), 1]], dtype=np.uint64)),
                     lambda: other.indel_fetch_diff(0, 1), lambda: other.indel_add_diff(0, np.zeros(1, dtype=np.uint32)), other.indel_text, other.indel_uncount):
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
        with pytest.raises(salt_amd.SaltError, match="contig table"):
            other.indel_enable(True, 0, 8)
        other.set_contigs(ix)
        for lg in (5, 29):
            with pytest.raises(salt_amd.SaltError, match="6 .. 28"):
                other.indel_enable(True, 0, lg)
        with pytest.raises(salt_amd.SaltError, match="256"):
            other.indel_enable(True, 256, 8)
        other.indel_enable(False)                                      # stopping what never ran is no error, and allocates nothing
        with pytest.raises(salt_amd.SaltError, match="never enabled"):
            other.indel_stats()
        other.indel_enable(True, 0, 8)
        other.indel_enable(True, 0, 0)
        with pytest.raises(salt_amd.SaltError, match="2\\^8"):
            other.indel_enable(True, 0, 9)                             # the size is fixed at the first enable
        for bad in (dict(min_alt=0), dict(min_pct=101)):
            with pytest.raises(salt_amd.SaltError, match="min_"):
                other.indel_text(**bad)
        for call in (lambda: other.indel_fetch_diff(REF_LEN, 2), lambda: other.indel_add_diff(REF_LEN + 1, np.ones(1, dtype=np.uint32))):
            with pytest.raises(salt_amd.SaltError, match="leave"):
                call()
        assert other.indel_fetch().shape == (0, 2) and other.indel_text() == b"" and not other.indel_stats().any()
    finally:
        other.close()


@pytest.mark.parametrize("name", sorted(SETS))
def test_text_call_equals_the_twin_and_the_python_statement(name, lam, text_states):
    salt_amd, ix, aln, genome = lam
    sam, got = text_states[name]
    twin = salt_amd.indel_add_sam(ix, sam, 0)
    print(name, got[2].tolist(), len(got[0]))
    check(name, got, twin[:3])
    check(name + " python", got, statement(genome, sam))
    assert int(got[2][0]) > 100 and int(got[2][1]) == 0 and twin[3] > 0
    # at the default floor, which drops records
    sam20, got20 = text_call(salt_amd, ix, aln, SETS[name][0], [_fq(f) for f in SETS[name][1]], 20)
    assert sam20 == sam
    check(name + " floor 20", got20, salt_amd.indel_add_sam(ix, sam, 20)[:3])
    check(name + " floor 20 python", got20, statement(genome, sam, 20))
    assert 0 < int(got20[2][0]) < int(got[2][0])


@pytest.mark.parametrize("name", ["se_default", "gap_se_lane", "gap_pe_short"])
def test_host_buffer_calls(name, lam, text_states):
    salt_amd, ix, aln, _ = lam
    args, files = SETS[name]
    paths = [os.path.join(LAMBDA, f) for f in files]
    if len(files) == 1:
        names, seqs, offs, quals = salt_amd.read_fastq(paths[0])
    else:
        names, seqs, offs, quals = salt_amd.interleave_pairs(salt_amd.read_fastq(paths[0]), salt_amd.read_fastq(paths[1]))
    opt = _opt(salt_amd, ix, args)
    call = (lambda: aln.alnpe_core1(opt, ix, seqs, offs)) if len(files) == 2 else (lambda: aln.alnse_core1(opt, seqs, offs))
    _, got = counted(aln, 0, call)
    check(name + " host buffer", got, text_states[name][1])


def test_two_calls_add_a_fork_shares_the_table_reset_off_and_uncount(lam, text_states):
    salt_amd, ix, aln, genome = lam
    opt_se, opt_pe = _opt(salt_amd, ix, SETS["gap_se_mid"][0]), _opt(salt_amd, ix, SETS["gap_pe_short"][0])
    fq, fq1, fq2 = _fq("reads_gap_se_mid.fq.gz"), _fq("reads_gap_pe_short_1.fq.gz"), _fq("reads_gap_pe_short_2.fq.gz")
    (sam_one, one), (sam_two, two) = text_states["gap_se_mid"], text_states["gap_pe_short"]
    zero = (np.zeros((0, 2), dtype=np.uint64), np.zeros(REF_LEN + 1, dtype=np.uint32), np.zeros(4, dtype=np.uint64))
    double = (one[0] * np.array([1, 2], dtype=np.uint64), 2 * one[1], 2 * one[2])
    summed = salt_amd.indel_add_sam(ix, [sam_one, sam_one, sam_two], 0)[:3]
    aln.indel_enable(True, 0)
    aln.indel_reset()
    fork = aln.fork()
    try:
        sam_on = aln.align_se_text(opt_se, fq)[0]
        aln.align_se_text(opt_se, fq)
        check("two calls", state(aln), double)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        check("fork", state(fork), summed)
        aln.indel_reset()
        check("reset", state(aln), zero, False)
        check("reset, fork", state(fork), zero, False)
        aln.indel_enable(False)
        sam_off = aln.align_se_text(opt_se, fq)[0]
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        check("off", state(aln), zero, False)
        assert sam_on == sam_off == sam_one                            # the SAM bytes do not depend on the tally
        # a block that is aligned and then dropped leaves table, counters and diff as they were; taking everything back leaves all-zero
        aln.indel_enable(True, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        aln.align_se_text(opt_se, fq)
        fork.indel_uncount()
        check("uncount", state(aln), one)
        fork.indel_uncount()                                           # only once
        check("uncount twice", state(aln), one)
        # counting after the text: the text only reads
        text = aln.indel_text(1, 0)
        assert text == salt_amd.indel_text(ix, one[0], one[1], 1, 0) == indel_check.text(genome, one[0], one[1], 1, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        check("after the text", state(aln), salt_amd.indel_add_sam(ix, [sam_one, sam_two], 0)[:3])
        fork.indel_uncount()
        aln.indel_uncount()
        check("all taken back", state(aln), zero, False)
        # indel_add and indel_add_diff on top of what is there: how GPUs are summed
        aln.indel_add(one[0])
        aln.indel_add(two[0])
        aln.indel_add(one[0][:100])
        aln.indel_add_diff(0, one[1])
        aln.indel_add_diff(REF_LEN, np.array([7], dtype=np.uint32))
        table = indel_check.table_of(one[0])
        for pairs in (two[0], one[0][:100]):
            for key, v in indel_check.table_of(pairs).items():
                cell = table.setdefault(key, [0, 0])
                cell[0], cell[1] = cell[0] + v[0], cell[1] + v[1]
        want_diff = one[1].copy()
        want_diff[REF_LEN] += np.uint32(7)
        events = int(one[2][0] + two[2][0]) + sum(sum(v) for v in indel_check.table_of(one[0][:100]).values())
        check("add", state(aln), (indel_check.entries(table), want_diff, np.array([events, 0, 0, 0], dtype=np.uint64)))
    finally:
        aln.indel_enable(False)
        aln.indel_reset()
        fork.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes_around_the_wave_and_the_block(n, lam):
    salt_amd, ix, aln, _ = lam
    fq = b"\n".join(_fq("reads_gap_se_lane.fq.gz").split(b"\n")[:4 * n]) + b"\n"
    sam, got = text_call(salt_amd, ix, aln, SETS["gap_se_lane"][0], [fq])
    assert len(sam_records(sam)) == n
    check("batch of %d" % n, got, salt_amd.indel_add_sam(ix, sam, 0)[:3], False)
    assert n == 1 or int(got[2][0]) > 0


def gapped_read(gen, g0, L, rev, at, delete=0, insert=b""):
    """L bases from g0 with `delete` bases taken out or `insert` put in at genome position `at`"""
    s = gen[g0:at] + insert + gen[at + delete:]
    s = s[:L]
    return s.translate(COMP)[::-1] if rev else s


def test_a_hot_allele_of_2048_copies_is_one_slot(lam):
    salt_amd, ix, aln, genome = lam
    gen = genome_letters()
    read = gapped_read(gen, 15000, 100, 0, 15050, delete=3)
    sam, got = text_call(salt_amd, ix, aln, ["-d", "-c"], [fastq_of([(b"h%d" % i, read) for i in range(2048)])])
    check("hot allele", got, salt_amd.indel_add_sam(ix, sam, 0)[:3])
    assert got[0].shape == (1, 2) and int(got[0][0, 1]) == 2048 and got[2].tolist() == [2048, 0, 0, 0]
    g, is_del, n, _ = indel_check.key_parts(int(got[0][0, 0]))
    assert is_del and n == 3 and g == indel_check.normalise(genome, 15050, True, 3, [])[0]
    assert int(got[1][15000]) == 2048


# (genome position, deleted bases, inserted letters): indels the aligner's edit-distance alignment writes as one op (an inserted ACG at
# 31 003, say, it writes as 2I1M1I, which is as good an alignment; the table then rightly holds two insertions)
PLANTED = ((30040, 2, b""), (31003, 0, b"GTC"), (32000, 0, b"TTG"), (33010, 1, b""), (35020, 0, b"T"))


def planted_reads(gen):
    """six reads a site, half of them reverse, the indel between their bases 35 and 65; between the sites, covered controls"""
    reads = []
    for k, (at, delete, insert) in enumerate(PLANTED):
        for i in range(6):
            reads.append((b"p%d_%d" % (k, i), gapped_read(gen, at - 35 - 6 * i, 100, i & 1, at, delete, insert)))
    return fastq_of(reads)


def test_planted_indels_are_the_file_at_the_defaults(lam):
    salt_amd, ix, aln, genome = lam
    sam, got = text_call(salt_amd, ix, aln, ["-d", "-c"], [planted_reads(genome_letters())], 20)
    py = statement(genome, sam, 20)
    check("planted", got, py)
    aln.indel_enable(True, 20)
    aln.indel_enable(False, 20)
    text = aln.indel_text()                                            # the table of the call is still there
    assert text == indel_check.text(genome, py[0], py[1]) == salt_amd.indel_text(ix, got[0], got[1])
    rows = indel_check.parse(text)
    want = []
    for at, delete, insert in PLANTED:
        g, bases, _ = indel_check.normalise(genome, at, delete > 0, delete or len(insert), [b"ACGT".index(x) for x in insert])
        want.append(("lambdaA", g, "DEL" if delete else "INS", delete or len(insert), "".join("ACGT"[b] for b in bases)))
    print(rows)
    assert [(r[0], r[1], r[4]["TYPE"], r[4]["LEN"], r[3][1:] if r[4]["TYPE"] == "INS" else "") for r in rows] == sorted(want, key=lambda w: w[1])
    assert all(r[4]["AO"] >= 3 and r[4]["AOF"] >= 1 and r[4]["AOR"] >= 1 and 100 * r[4]["AO"] >= 20 * r[4]["DP"] for r in rows)


# ---- the insert routine through hand-made keys ----
def keys_at_home(log2_slots, home, n, start=1):
    """the first n one-base deletions from g = start on whose home slot is `home`"""
    out, g = [], start
    while len(out) < n:
        if indel_check.home(K(g, True, 1), log2_slots) == home:
            out.append(K(g, True, 1))
        g += 1
    return out


def test_the_probe_wraps_at_the_tables_end_and_fetch_is_in_key_order(lam):
    salt_amd, ix, _, _ = lam
    aln = new_aligner(salt_amd, ix, 64)
    try:
        aln.indel_enable(True, 0, 8)
        aln.indel_enable(False, 0)
        a, b = keys_at_home(8, 255, 2)
        aln.indel_add(np.array([[b, 5], [a, 3 << 32]], dtype=np.uint64))                  # both at home in the last slot: one of them goes to slot 0
        aln.indel_add(np.array([[b, 1 | 2 << 32]], dtype=np.uint64))                      # a repeat: found again, wherever it went
        assert aln.indel_fetch().tolist() == [[a, 3 << 32], [b, 6 | 2 << 32]] and aln.indel_stats().tolist() == [11, 0, 0, 0]
        # keys of every shape, given in no order, come back sorted as integers: genome order, at one g insertions in front of deletions
        rng = np.random.RandomState(3)
        keys = {K(int(g), bool(d), int(n), [int(x) for x in rng.randint(0, 4, size=n)] if not d else ()) for g, d, n in zip(rng.randint(1, REF_LEN, 300), rng.randint(0, 2, 300), rng.randint(1, 13, 300))}
        special = {K(700, True, 63), K(700, False, 1, [3]), K(700, False, 12, [3] * 12), K(699, True, 1), K(701, False, 1, [0])}
        chosen = sorted(keys - special)[:95] + sorted(special)         # 100 of 256 slots: their longest cluster is 8 slots, so no order of arrival drops one
        pairs = np.array([[k, 1 + i] for i, k in enumerate(sorted(chosen, key=lambda k: indel_check.home(k, 8)))], dtype=np.uint64)
        aln.indel_reset()
        aln.indel_add(pairs)
        got = aln.indel_fetch()
        assert got.tolist() == sorted(pairs.tolist()) and int(aln.indel_stats()[1]) == 0
        assert aln.indel_text(1, 0) == salt_amd.indel_text(ix, got, np.zeros(REF_LEN + 1, dtype=np.uint32), 1, 0)
    finally:
        aln.close()


def test_a_full_probe_run_drops_exactly_the_keys_past_it(lam):
    salt_amd, ix, _, _ = lam
    aln = new_aligner(salt_amd, ix, 64)
    try:
        aln.indel_enable(True, 0, 8)
        aln.indel_enable(False, 0)
        keys = keys_at_home(8, 200, 129)                               # 129 distinct keys that share a home slot: the run from it holds 128
        first = np.array([[k, 2] for k in keys[:128]], dtype=np.uint64)
        aln.indel_add(first)
        assert aln.indel_fetch().tolist() == first.tolist() and aln.indel_stats().tolist() == [256, 0, 0, 0]
        aln.indel_add(np.array([[keys[128], 3 | 4 << 32]], dtype=np.uint64))             # the 129th finds the run full
        assert aln.indel_fetch().tolist() == first.tolist() and aln.indel_stats().tolist() == [256, 7, 0, 0]
        aln.indel_add(first[5:6])                                      # a key inside the run is still found
        assert int(aln.indel_fetch()[5, 1]) == 4 and aln.indel_stats().tolist() == [258, 7, 0, 0]
        # all 129 at once: whichever 128 win, one is dropped
        aln.indel_reset()
        aln.indel_add(np.array([[k, 1] for k in keys], dtype=np.uint64))
        got = aln.indel_fetch()
        assert len(got) == 128 and set(got[:, 0].tolist()) < set(keys) and aln.indel_stats().tolist() == [128, 1, 0, 0]
        # a key whose home is 100 slots in front of the full run still has 28 slots of its own run... which are taken: it probes 128 slots and is dropped too
        aln.indel_add(np.array([[k, 1] for k in keys_at_home(8, 100, 101)], dtype=np.uint64))      # fills [100, 200) and one more finds [200, 228) full
        assert aln.indel_stats().tolist() == [228, 2, 0, 0]
    finally:
        aln.close()


def test_a_table_of_64_slots_overflows_and_loses_nothing_it_holds(lam, text_states):
    salt_amd, ix, _, genome = lam
    aln = new_aligner(salt_amd, ix)
    try:
        aln.indel_enable(True, 0, 6)
        opt = _opt(salt_amd, ix, SETS["gap_se_mid"][0])
        sam = aln.align_se_text(opt, _fq("reads_gap_se_mid.fq.gz"))[0]
        got = state(aln)
        twin = salt_amd.indel_add_sam(ix, sam, 0)
        tabled, dropped = int(got[2][0]), int(got[2][1])
        print("64 slots under gap_se_mid:", got[2].tolist(), len(got[0]), "of", len(twin[0]), "alleles")
        assert sam == text_states["gap_se_mid"][0] and dropped > 0 and tabled + dropped == int(twin[2][0]) and got[2][2:].tolist() == twin[2][2:].tolist()
        assert len(got[0]) <= 64 and np.array_equal(got[1], twin[1])
        want = indel_check.table_of(twin[0])
        for key, v in indel_check.table_of(got[0]).items():            # every fetched value is at most the twin's, per strand
            assert key in want and v[0] <= want[key][0] and v[1] <= want[key][1], key
        assert sum(sum(v) for v in indel_check.table_of(got[0]).values()) == tabled
        assert aln.indel_text(1, 0) == salt_amd.indel_text(ix, got[0], got[1], 1, 0)
        aln.indel_uncount()
        after = state(aln)
        assert after[0].shape == (0, 2) and not after[1].any() and not after[2].any()
    finally:
        aln.close()


# ---- the text ----
@pytest.fixture(scope="module")
def hand_made(lam, text_states):
    """a call's own table and diff with alleles added by hand: anchors on position 0, on both sides of the contig boundary and on the
    genome's last positions, 64 alleles on consecutive anchors, two alleles at one anchor, words that are no well-formed keys"""
    salt_amd, ix, aln, genome = lam
    entries, diff = text_states["gap_se_mid"][1][:2]
    extra = [[K(1, True, 2), 900], [K(BOUND, False, 2, [1, 2]), 900 << 32], [K(BOUND + 1, True, 1), 900 | 900 << 32], [K(REF_LEN - 1, True, 1), 900], [K(REF_LEN, False, 1, [3]), 900],
             [K(64, True, 63), 901], [K(64, False, 12, [0, 1, 2, 3] * 3), 902], [K(REF_LEN + 1, True, 1), 900], [K(70, False, 13), 900], [K(71, True, 1) | 1 << 10, 900]]
    extra += [[K(g, True, 1), 800] for g in range(4097, 4161)]
    entries = entries[~np.isin(entries[:, 0], np.array([k for k, _ in extra], dtype=np.uint64))]      # (the call's own alleles at those keys make room)
    aln.indel_enable(True, 0)
    aln.indel_enable(False, 0)
    aln.indel_reset()
    aln.indel_add(entries)
    aln.indel_add(np.array(extra, dtype=np.uint64))
    aln.indel_add_diff(0, diff)
    pairs = np.array(sorted(entries.tolist() + extra), dtype=np.uint64)
    assert np.array_equal(aln.indel_fetch(), pairs)
    return pairs, diff


@pytest.mark.parametrize("tile", [64, 1000, 48502, 97004, 0])
@pytest.mark.parametrize("rule", [(3, 20), (1, 0)])
def test_device_text_equals_the_twins_byte_for_byte(tile, rule, lam, hand_made):
    salt_amd, ix, aln, genome = lam
    pairs, diff = hand_made
    want = salt_amd.indel_text(ix, pairs, diff, *rule)
    pieces = aln.indel_text(*rule, tile_positions=tile, pieces=True)
    assert b"".join(pieces) == want and want == indel_check.text(genome, pairs, diff, *rule)
    parsed = indel_check.parse(want)
    rows = {(r[0], r[1], r[4]["TYPE"]) for r in parsed}
    assert {("lambdaA", 1, "DEL"), ("lambdaA", BOUND, "INS"), ("lambdaB_div2pct", 1, "DEL"), ("lambdaB_div2pct", BOUND - 1, "DEL"), ("lambdaB_div2pct", BOUND, "INS"),
            ("lambdaA", 64, "DEL"), ("lambdaA", 64, "INS"), ("lambdaA", 4097, "DEL"), ("lambdaA", 4160, "DEL")} <= rows
    assert len(parsed) == len(pairs) - 3 if rule == (1, 0) else 71 < len(parsed) < len(pairs) - 3      # the three words that are no well-formed keys never have a line
    assert len(pieces) == 1 and pieces[0].endswith(b"\n")


def test_bgzf_pieces_inflate_to_the_text_twice_the_same_and_the_table_stays(lam, hand_made):
    salt_amd, ix, aln, genome = lam
    pairs, diff = hand_made
    want = salt_amd.indel_text(ix, pairs, diff, 1, 0)
    z = aln.indel_text(1, 0, tile_positions=1000, bgzf=True, pieces=True)
    assert len(z) == 1 and z[0][:4] == b"\x1f\x8b\x08\x04"
    assert _gunzip_members(b"".join(z)) == want == gzip.decompress(b"".join(z)) and not b"".join(z).endswith(BGZF_EOF)
    assert aln.indel_text(1, 0, tile_positions=1000, bgzf=True, pieces=True) == z and aln.indel_text(1, 0) == want
    assert np.array_equal(aln.indel_fetch(), pairs) and np.array_equal(aln.indel_fetch_diff(0, REF_LEN + 1), diff)


def test_a_text_larger_than_its_buffer_leaves_in_pieces_cut_at_line_ends(lam):
    salt_amd, ix, _, genome = lam
    aln = new_aligner(salt_amd, ix, 64)
    try:
        aln.indel_enable(True, 0, 18)
        aln.indel_enable(False, 0)
        pairs = np.array([[K(g, False, 12, [g & 3] * 12), 1 + (g % 7) << 32 | g] for g in range(1, 90001)], dtype=np.uint64)      # 90 000 lines of about 70 bytes
        aln.indel_add(pairs)
        assert aln.indel_stats().tolist()[1] == 0
        diff = np.zeros(REF_LEN + 1, dtype=np.uint32)
        diff[0], diff[50000] = 7, (1 << 32) - 7
        aln.indel_add_diff(0, diff)
        want = salt_amd.indel_text(ix, pairs, diff, 1, 100)            # a rule that passes some and stops others: AO against depth 7 or 0
        pieces = aln.indel_text(1, 100, pieces=True)
        assert len(want) > (4 << 20) and len(pieces) >= 2 and all(p.endswith(b"\n") and len(p) <= (4 << 20) + 512 for p in pieces)
        assert b"".join(pieces) == want
        z = aln.indel_text(1, 100, bgzf=True, pieces=True)
        assert len(z) == len(pieces) and [_gunzip_members(p) for p in z] == pieces
    finally:
        aln.close()


# ---- the driver ----
@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("indelidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


LOOSE = ["--indels-min-mapq", "0", "--indels-min-alt", "1", "--indels-min-pct", "0"]


def want_file(salt_amd, ix, sam, min_mapq=0, min_alt=1, min_pct=0, dropped=0):
    entries, diff, stats, n = salt_amd.indel_add_sam(ix, sam, min_mapq)
    assert n > 0
    return salt_amd.indel_header(ix, min_mapq, min_alt, min_pct, dropped) + salt_amd.indel_text(ix, entries, diff, min_alt, min_pct), stats


def test_cli_file_equals_the_twin_over_its_stdout_plain_gz_and_two_gpus(lam, lambda_cli_index, tmp_path):
    import torch
    salt_amd, ix, _, _ = lam
    reads = gap_cases.plain_paths("gap_se_mid", tmp_path)[0]
    f, fz = tmp_path / "indels.vcf", tmp_path / "indels.vcf.gz"
    plain = subprocess.run([SALT, "-d", "-c", lambda_cli_index, reads], capture_output=True, timeout=300)
    run = subprocess.run([SALT, "-d", "-c", "--indels", str(f)] + LOOSE + [lambda_cli_index, reads], capture_output=True, timeout=300)
    assert run.returncode == 0 and b"tabled and printed on the device" in run.stderr and b"WARNING" not in run.stderr, run.stderr[-600:]
    assert strip_pg(run.stdout) == strip_pg(plain.stdout) == gap_cases.golden("gap_se_mid")      # stdout is what it is without the option
    want, stats = want_file(salt_amd, ix, run.stdout)
    assert f.read_bytes() == want and want.count(b"\n") > 1000
    assert b"tabled %d, dropped 0, long %d, unanchored %d" % (stats[0], stats[2], stats[3]) in run.stderr
    gz = subprocess.run([SALT, "-d", "-c", "--indels", str(fz), lambda_cli_index, reads], capture_output=True, timeout=300)      # the defaults
    z = fz.read_bytes()
    assert gz.returncode == 0 and z.endswith(BGZF_EOF) and _gunzip_members(z) == want_file(salt_amd, ix, run.stdout, 20, 3, 20)[0], gz.stderr[-600:]
    assert len(indel_check.parse(_gunzip_members(z))) >= 1
    # a table that is too small: the dropped events are in the header and in a warning that names the option
    small = subprocess.run([SALT, "-d", "-c", "--indels", str(f), "--indels-slots", "64"] + LOOSE + [lambda_cli_index, reads], capture_output=True, timeout=300)
    assert small.returncode == 0 and b"WARNING" in small.stderr and b"--indels-slots" in small.stderr and strip_pg(small.stdout) == strip_pg(plain.stdout), small.stderr[-600:]
    head = [l for l in f.read_bytes().split(b"\n") if l.startswith(b"##salt_indels_dropped=")]
    assert len(head) == 1 and int(head[0].split(b"=")[1]) > 0
    if torch.cuda.device_count() >= 2:                                 # the other GPU's table and diff are merged into the first one's
        two = subprocess.run([SALT, "-d", "-c", "-t", "4", "--gpus", "2", "--indels", str(f)] + LOOSE + [lambda_cli_index, reads], capture_output=True, timeout=300,
                             env=dict(os.environ, SALT_CHUNK_BYTES="20000"))
        assert two.returncode == 0 and strip_pg(two.stdout) == strip_pg(run.stdout), two.stderr[-600:]
        assert f.read_bytes() == want


def test_cli_paired_end_text_path_and_host_pipeline(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _, _ = lam
    args = gap_cases.GAP_CASES["gap_pe_short"][0]
    reads = gap_cases.plain_paths("gap_pe_short", tmp_path)
    f = tmp_path / "indels.vcf"
    for env, word in ((dict(os.environ), b"text path"), (dict(os.environ, SALT_HOST_PIPELINE="1"), b"host phases")):
        run = subprocess.run([SALT] + list(args) + ["--indels", str(f)] + LOOSE + [lambda_cli_index] + reads, capture_output=True, timeout=300, env=env)
        assert run.returncode == 0 and word in run.stderr and b"on the device" in run.stderr, run.stderr[-600:]
        assert f.read_bytes() == want_file(salt_amd, ix, run.stdout)[0]


def test_cli_counts_every_written_block_once_across_the_hand_over(lam, lambda_cli_index, tmp_path):
    """A multi-line record in the middle of the file, chunks of 9 000 bytes: the blocks the workers had aligned behind the refused chunk
    are dropped and their adds taken back (salt_gpu_ws_indel_uncount); the host pipeline aligns those reads again."""
    salt_amd, ix, _, _ = lam
    recs = _fq("reads_gap_se_mid.fq.gz").split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1000 else r      # (behind the 256 KiB the driver looks at before it chooses the text path)
    fq, f = tmp_path / "mid_multiline.fq", tmp_path / "indels.vcf"
    fq.write_bytes(b"\n".join(out) + b"\n")
    run = subprocess.run([SALT, "-d", "-c", "-t", "8", "--indels", str(f)] + LOOSE + [lambda_cli_index, str(fq)], capture_output=True, timeout=300,
                         env=dict(os.environ, SALT_CHUNK_BYTES="9000"))
    assert run.returncode == 0, run.stderr[-600:]
    assert b"the host parser takes over" in run.stderr and b"on the device" in run.stderr
    assert strip_pg(run.stdout) == gap_cases.golden("gap_se_mid")
    want, stats = want_file(salt_amd, ix, run.stdout)
    assert f.read_bytes() == want and b"tabled %d, dropped 0" % stats[0] in run.stderr
