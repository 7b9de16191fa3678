"""SNP candidates off the index's sites without a GPU: the host twin and its printer (salt_disc_add_sam, salt_disc_text) against the Python
statement (tests/disc_check.py) on the lambda goldens, the quality filter on requalified goldens, hand-made arrays that hold every case
of the call rule and of the line, and the round trip through the index builder: the file is a SNP file salt-idx rebuilds an index from."""
import os

import numpy as np
import pytest

import disc_check
import errprof_check
import snp_check
from conftest import GOLDEN, LAMBDA

# golden -> events at (min_mapq, min_baseq) = (0, 0), (20, 20): counted when the test was written (the first column is the census of the issue)
EVENTS = {
    "expect_se_default.sam": (1243, 1228), "expect_pe_default.sam": (954, 937), "expect_ragged_pe.sam": (584, 579),
    "expect_gap_se_mid.sam.gz": (2451, 2177), "expect_gap_pe_short.sam.gz": (395, 371), "expect_span_default.sam": (22, 22),
}


def fields(alt):
    a = np.asarray(alt, dtype=np.uint64)
    return int(sum(((a >> np.uint64(21 * k)) & np.uint64(disc_check.FIELD)).sum() for k in range(3)))


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield salt_amd, ix, disc_check.Genome()
    ix.destroy()


@pytest.fixture(scope="module", params=["two_contigs", "all_snp_contigs"])
def small(request):
    import salt_amd
    prefix = os.path.join(GOLDEN, "index_cases", request.param, "idx")
    ix = salt_amd.Index.reload(prefix)
    yield salt_amd, ix, disc_check.Genome(prefix), request.param
    ix.destroy()


def test_the_defaults_are_the_definitions():
    import salt_amd
    assert salt_amd.DISC_DEFAULTS == disc_check.DEFAULTS == dict(min_mapq=20, min_baseq=20, min_alt=3, min_pct=20)
    assert salt_amd.DISC_FIELD_BITS == disc_check.BITS == 21 and (salt_amd.DISC_ALT, salt_amd.DISC_DIFF) == (0, 1)


@pytest.mark.parametrize("name", sorted(snp_check.GOLDENS))
def test_the_twins_arrays_equal_the_python_statement(name, lam):
    salt_amd, ix, genome = lam
    sam = snp_check.golden_sam(name)
    for k, (mq, bq) in enumerate(((0, 0), (20, 20), (255, 0))):
        st = {}
        alt, diff, n = disc_check.add_sam(genome, sam, mq, bq, st)
        got_alt, got_diff, got_n = salt_amd.disc_add_sam(ix, sam, mq, bq)
        print(name, mq, bq, n, st)
        assert got_n == n == (0 if mq == 255 else snp_check.GOLDENS[name][k])
        assert np.array_equal(got_alt, alt) and np.array_equal(got_diff, diff)
        assert st["counted"] == fields(alt) == (0 if mq == 255 else EVENTS[name][k])
        # the tally's own difference array is the coverage's rule under this tally's floor
        import depth_check
        assert np.array_equal(got_diff, depth_check.diff_of_sam(depth_check.lambda_contigs(), sam, mq)[0])
        again = salt_amd.disc_add_sam(ix, sam, mq, bq, alt=got_alt.copy(), diff=got_diff.copy())
        assert np.array_equal(again[0], 2 * got_alt) and np.array_equal(again[1], 2 * got_diff)
    assert disc_check.add_sam(genome, sam, 0, 0, st)[2] and st["at_sites"] == {"expect_se_default.sam": 31, "expect_gap_se_mid.sam.gz": 64}.get(name, st["at_sites"])


@pytest.mark.parametrize("name", sorted(snp_check.GOLDENS))
def test_the_printers_text_equals_the_python_statement(name, lam):
    salt_amd, ix, genome = lam
    alt, diff, _ = salt_amd.disc_add_sam(ix, snp_check.golden_sam(name), 0, 0)
    n_lines = {}
    for min_alt, min_pct in ((1, 0), (2, 10), (3, 20)):
        for all_sites in (False, True):
            want = disc_check.text(genome, alt, diff, min_alt, min_pct, all_sites)
            assert salt_amd.disc_text(ix, alt, diff, min_alt, min_pct, all_sites) == want
            n_lines[min_alt, all_sites] = len(disc_check.parse(want))
    rows = disc_check.parse(disc_check.text(genome, alt, diff, 1, 0))
    assert len(rows) == int(np.count_nonzero(alt)) and (len(rows) > 1000) == (name in ("expect_se_default.sam", "expect_gap_se_mid.sam.gz"))
    third = [r for r in rows if r[5].count(None) >= 2]             # lines at known sites: a third allele
    assert third and all(len(r[2].split("/")) >= 3 for r in third)
    assert all(r[2].split("/") == sorted(r[2].split("/")) and r[3] in "ACGT" for r in rows)
    # with all, every site of the index has a line, and the lines without all are among them
    assert n_lines[3, True] == len(genome.sites) + n_lines[3, False] - sum(1 for r in disc_check.parse(disc_check.text(genome, alt, diff)) if r[5].count(None) >= 2)
    assert n_lines[3, False] == (1 if name == "expect_gap_se_mid.sam.gz" else 0)      # the goldens are shallow: one candidate at the defaults in all six


def test_the_quality_filter_on_both_sides_of_the_floor(lam):
    salt_amd, ix, genome = lam
    sam = snp_check.golden_sam("expect_se_default.sam")
    st = {}
    alt, diff, n = disc_check.add_sam(genome, sam, 0, 30, st)                  # the golden's own qualities: all at least 20, some below 30
    got = salt_amd.disc_add_sam(ix, sam, 0, 30)
    assert np.array_equal(got[0], alt) and np.array_equal(got[1], diff) and st["below"] > 0 and st["passed"] > 0 and st["events"] == 1243
    assert np.array_equal(got[1], salt_amd.disc_add_sam(ix, sam, 0, 0)[1])     # diff does not look at qualities
    ramp = lambda k, L: bytes(33 + (k + j) % 94 for j in range(L))
    odd = lambda k, L: bytes((1 + (k + 7 * j) % 255) if (k + j) % 3 else 0x7F for j in range(L)).replace(b"\t", b"\x0b").replace(b"\n", b"\x0b")
    for name in ("expect_se_default.sam", "expect_gap_pe_short.sam.gz"):
        sam = snp_check.golden_sam(name)
        for qual_of, floor in ((ramp, 20), (ramp, 93), (lambda k, L: b"!" * L, 1), (lambda k, L: b"~" * L, 93), (lambda k, L: b"*" if L != 1 else b"I", 93), (odd, 40)):
            text = errprof_check.requalify(sam, qual_of)
            st = {}
            alt, diff, n = disc_check.add_sam(genome, text, 0, floor, st)
            got = salt_amd.disc_add_sam(ix, text, 0, floor)
            print(name, floor, st)
            assert np.array_equal(got[0], alt) and np.array_equal(got[1], diff) and got[2] == n
            if qual_of is ramp:
                assert st["below"] > 0 and st["passed"] > 0 and st["unusable"] == 0
            elif qual_of is odd:
                assert st["below"] > 0 and st["passed"] > 0 and st["unusable"] > 0      # bytes below 33 and above 126 pass the filter
            elif st["unusable"]:
                assert st["unusable"] == st["events"] == st["counted"]         # QUAL *: every event counts
            else:
                assert (st["below"] == st["events"]) != (st["passed"] == st["events"])      # all '!' below 1; all '~' at 93


def W(a=0, b=0, c=0):
    return a | b << 21 | c << 42


def test_hand_made_arrays_hold_every_case_of_the_call_and_of_the_line(small):
    salt_amd, ix, genome, which = small
    n = len(genome.masks)
    alt, depth = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)
    bound = genome.contigs[1][1]
    cases = {0: (W(5), 10), n - 1: (W(0, 7), 7), bound - 1: (W(3), 3), bound: (W(0, 0, 4), 4),      # position 0, ref_len - 1, both sides of a contig boundary
             20: (W(4, 5), 12), 21: (W(3, 4, 5), 12),                      # two and three called bases at one position
             30: (W(1, disc_check.FIELD, 1), 3000000),                     # a field at 2 097 151 beside neighbours at 1
             40: (W(4), 20), 41: (W(4), 21), 42: (W(2), 2),                # 100 n == min_pct depth exactly, one short of it, n below min_alt
             50: (W(3), 0)}                                                # depth 0 with a count
    for g, (w, d) in cases.items():
        assert bin(int(genome.masks[g])).count("1") == 1                   # plain positions: three bases outside the mask
        alt[g], depth[g] = w, d
    sites = [int(g) for g in genome.sites]
    alt[sites[0]] = W(6, 1)                                                # a known site: a third allele called, the fourth base seen once
    depth[sites[0]] = 20
    diff = np.zeros(n + 1, dtype=np.int64)
    diff[0], diff[1:n] = depth[0], depth[1:] - depth[:-1]
    diff[n] = -depth[n - 1]
    diff = (diff % (1 << 32)).astype(np.uint32)
    for all_sites in (False, True):
        want = disc_check.text(genome, alt, diff, 3, 20, all_sites)
        text, seen = salt_amd.disc_text(ix, alt, diff, 3, 20, all_sites, seen=True)
        assert text == want
        rows = {(r[0], r[1]): r for r in disc_check.parse(want)}

        def row(g):
            name, off, _ = genome.contigs[genome.contig_of(g)]
            return rows.get((name, g - off + 1))
        assert row(0) and row(n - 1) and row(bound - 1) and row(bound) and row(bound - 1)[0] != row(bound)[0] and row(bound)[1] == 1
        assert len(row(20)[2].split("/")) == 3 and len(row(21)[2].split("/")) == 4 and row(21)[2] == "A/C/G/T"
        assert sorted(x for x in row(30)[5] if x is not None) == [1, 1, 2097151] and len(row(30)[2].split("/")) == 2 and row(30)[4] == 3000000
        assert row(40) and row(40)[4] == 20 and row(41) is None and row(42) is None
        assert row(50) and row(50)[4] == 0
        s0 = row(sites[0])
        assert s0[5].count(None) == 2 and sorted(x for x in s0[5] if x is not None) == [1, 6] and len(s0[2].split("/")) == 3
        assert len(rows) == (9 + len(sites) if all_sites else 10)
        assert seen.tolist() == [1 if any(r[0] == c[0] for r in rows.values()) else 0 for c in genome.contigs]
    if which == "all_snp_contigs":
        g15 = int(np.flatnonzero(genome.masks == 15)[0])                   # mask 15: no base is outside it; a line only with all, all counts '.'
        alt2 = alt.copy()
        alt2[g15] = W(9, 9, 9)
        assert salt_amd.disc_text(ix, alt2, diff, 1, 0) == salt_amd.disc_text(ix, alt, diff, 1, 0) == disc_check.text(genome, alt2, diff, 1, 0)
        line = [r for r in disc_check.parse(salt_amd.disc_text(ix, alt2, diff, 1, 0, True)) if r[2] == "A/C/G/T" and r[5] == [None] * 4]
        assert len(line) == 1 and salt_amd.disc_text(ix, alt2, diff, 1, 0, True) == disc_check.text(genome, alt2, diff, 1, 0, True)
        only = np.zeros(n, dtype=np.uint64)
        only[0], only[n - 1] = alt[0], alt[n - 1]
        assert salt_amd.disc_text(ix, only, diff, 3, 20, seen=True)[1].tolist() == [1, 0, 1]     # the middle contig has no line
    # a SAM line that reaches past ref_len is cut, not refused
    name, off, length = genome.contigs[-1]
    seq = b"A" * 30
    line = b"r\t0\t%s\t%d\t60\t30M\t*\t0\t0\t%s\t%s\n" % (name.encode(), length - 9, seq, b"I" * 30)
    st = {}
    a, d, k = disc_check.add_sam(genome, line, 0, 0, st)
    got = salt_amd.disc_add_sam(ix, line, 0, 0)
    assert k == got[2] == 1 and st["cut"] == 1 and np.array_equal(got[0], a) and np.array_equal(got[1], d) and int(d[n - 10]) == 1 and int(d[n]) == 0xFFFFFFFF
    with pytest.raises(salt_amd.SaltError, match="min_alt"):
        salt_amd.disc_text(ix, alt, diff, 0, 20)
    with pytest.raises(salt_amd.SaltError, match="contiguous"):
        salt_amd.disc_add_sam(ix, line, alt=np.zeros(n + 1, dtype=np.uint64), diff=np.zeros(n + 2, dtype=np.uint32))


def test_a_genome_n_gets_no_line_whatever_its_word(lam):
    salt_amd, ix, genome = lam
    n = len(genome.masks)
    g0 = int(np.flatnonzero(genome.masks == 0)[0])
    alt, diff = np.zeros(n, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint32)
    alt[g0], alt[g0 - 1] = W(9, 9, 9), W(9)
    for all_sites in (False, True):
        text = salt_amd.disc_text(ix, alt, diff, 1, 0, all_sites)
        assert text == disc_check.text(genome, alt, diff, 1, 0, all_sites)
        pos = [r[1] for r in disc_check.parse(text) if r[0] == "lambdaB_div2pct"]
        assert g0 - 48502 in pos and g0 - 48502 + 1 not in pos


def test_round_trip_the_file_is_a_snp_file_the_index_builder_takes(tmp_path):
    import salt_amd
    d = os.path.join(GOLDEN, "index_cases", "two_contigs")
    ix, genome = salt_amd.Index.reload(os.path.join(d, "idx")), disc_check.Genome(os.path.join(d, "idx"))
    n = len(genome.masks)
    alt, diff = np.zeros(n, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint32)
    new = {100: None, 500 + 20: None}                                          # one new SNP in each contig
    for g in new:
        m = int(genome.masks[g])
        outside = [b for b in range(4) if not (m >> b) & 1]
        alt[g] = W(0, 8)                                                       # the second base outside the mask
        new[g] = m | 1 << outside[1]
    diff[0], diff[n] = 10, (1 << 32) - 10
    text = salt_amd.disc_text(ix, alt, diff, 3, 20, True)
    assert text == disc_check.text(genome, alt, diff, 3, 20, True) and len(disc_check.parse(text)) == 4
    snps = tmp_path / "found.txt"
    snps.write_bytes(text)
    salt_amd.idx_build(os.path.join(d, "genome.fa"), str(snps), str(tmp_path / "new"), 19)
    masks = snp_check.sites_of_ref(str(tmp_path / "new.ref"))[1]
    want = genome.masks.copy()
    for g, m in new.items():
        want[g] = m
    assert np.array_equal(masks, want) and int((masks != genome.masks).sum()) == 2
    salt_amd.idx_build(os.path.join(d, "genome.fa"), os.path.join(d, "snps.txt"), str(tmp_path / "old"), 19)
    assert open(str(tmp_path / "old.ref"), "rb").read() == open(os.path.join(d, "idx.ref"), "rb").read()
    ix.destroy()
