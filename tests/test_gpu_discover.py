"""SNP candidates off the index's sites on the device (salt --discover).  The arrays: k_disc_add behind every entry point
that leaves result rows against the host twin (salt_disc_add_sam) over the SAM text the same call returned and against the Python
statement (tests/disc_check.py) -- text, host-buffer with and without set_quals, resident, single and paired end; reads made to stand on
every edge of a word-at-a-time compare; batch sizes around the wave and the block; a hot spot; planted SNPs.  The state: two calls, a
fork, reset, off, uncount, the errors.  The text kernels against salt_disc_text byte for byte.  Then the `salt` binary with --discover."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import disc_check
import gap_cases
from bgzf_check import strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT

pytestmark = pytest.mark.gpu

SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
ALT, DIFF = 0, 1
REF_LEN, BOUND = 97004, 48502

SE_SETS = {
    "se_default": (["-d", "-c"], ["reads_se.fq"]), "ragged_default": EXTRA_CASES["ragged_default"], "span_default": EXTRA_CASES["span_default"],
    "gap_se_mid": (gap_cases.GAP_CASES["gap_se_mid"][0], ["reads_gap_se_mid.fq.gz"]),
}
PE_SETS = {
    "pe_default": (["-d", "-p", "-c", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"]), "ragged_pe": EXTRA_CASES["ragged_pe"],
    "gap_pe_short": (gap_cases.GAP_CASES["gap_pe_short"][0], ["reads_gap_pe_short_1.fq.gz", "reads_gap_pe_short_2.fq.gz"]),
}
ALL_SETS = dict(SE_SETS, **PE_SETS)
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _fq(name):
    data = open(os.path.join(LAMBDA, name), "rb").read()
    return gzip.decompress(data) if name.endswith(".gz") else data


def genome_letters():
    """the concatenated lambda genome as bytes (both contigs, N included)"""
    return b"".join(l.strip() for l in open(os.path.join(LAMBDA, "genome.fa"), "rb") if not l.startswith(b">")).upper()


def outside(mask):
    """the first letter the mask does not have"""
    return b"ACGT"[[b for b in range(4) if not (mask >> b) & 1][0]]


def make_read(gen, g0, L, rev, plant=()):
    s = bytearray(gen[g0:g0 + L])
    for g, letter in plant:
        s[g - g0] = letter
    return bytes(s).translate(COMP)[::-1] if rev else bytes(s)


def fastq_of(reads, qual=b"I"):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (name, seq, qual * len(seq)) for name, seq in reads)


def distinct_start(gen, g0, L):
    """the first start at or behind g0 with the same g & 7 where the two contigs (the second is a diverged copy of the first) differ in at
    least 4 of the L bases: a read from there has one best place"""
    while sum(a != b for a, b in zip(gen[g0:g0 + L], gen[g0 + BOUND:g0 + BOUND + L])) < 4:
        g0 += 8
    return g0


def edge_reads(gen, masks):
    """(FASTQ, {name: (g0, L, rev, planted position or None, category)}): reads cut from the lambda genome so that an M run begins at every
    g & 7, on both strands, with one base the mixRef does not have planted at the columns where a word-at-a-time compare goes wrong"""
    reads, info = [], {}

    def add(cat, g0, L, rev, col=None, letter=None):
        name = b"e%d_%s" % (len(reads), cat.encode())
        plant = []
        if col is not None:
            g = g0 + col
            assert masks[g] not in (0, 15)
            plant = [(g, letter if letter is not None else outside(int(masks[g])))]
        reads.append((name, make_read(gen, g0, L, rev, plant)))
        info[name] = (g0, L, rev, plant[0][0] if plant and plant[0][1] != ord("N") else None, cat)

    for k in range(8):                                                 # eight consecutive starts: every g & 7
        for rev in (0, 1):
            for col in (0, 7, 8, 31, 32, 98, 99):
                add("start%d_col%d" % (k, col), distinct_start(gen, 10000 + 136 * k + k, 100), 100, rev, col)
    for L in (100, 120, 121, 511, 512):                                # the lengths, in one batch
        for rev in (0, 1):
            for col in (0, L - 2, L - 1):
                add("len%d" % L, distinct_start(gen, 20003 + 7 * L, L), L, rev, col)
    for rev in (0, 1):
        add("genome_end", REF_LEN - 100, 100, rev, 99)                 # an M run that ends at ref_len - 1, its last column planted
        add("boundary", BOUND - 50, 100, rev, 10)                      # over the contig boundary at 48 502
        add("genome_n", int(np.flatnonzero(masks == 0)[0]) - 95, 100, rev, 5)      # over the genome's N: the read's last five bases are N
        add("read_n", distinct_start(gen, 30011, 100), 100, rev, 8, ord("N"))                    # a read N at a planted column: no event
    two = [int(g) for g in np.flatnonzero(np.isin(masks, (3, 5, 6, 9, 10, 12))) if 1000 < g < 40000][:2]
    three = [int(g) for g in np.flatnonzero(np.isin(masks, (7, 11, 13, 14))) if 1000 < g < 40000][:2]
    for cat, sites in (("site2", two), ("site3", three)):
        for g in sites:
            for rev in (0, 1):
                add(cat, g - 37, 100, rev, 37)
    return fastq_of(reads), info


def sam_records(sam):
    return [l.split(b"\t") for l in sam.split(b"\n") if l and not l.startswith(b"@")]


def sam_with_quals(sam, quals_of):
    """the SAM text with every record's QUAL replaced by quals_of[(name, mate)] as printed: reversed for a reverse read, a byte outside
    33 .. 126 as 0x7F (no usable quality for the twin either); quals_of None: `*`"""
    out = []
    for line in sam.split(b"\n"):
        if not line or line.startswith(b"@"):
            out.append(line)
            continue
        f = line.split(b"\t")
        if quals_of is None:
            f[10] = b"*"
        else:
            flag = int(f[1])
            q = np.array(quals_of[(f[0], 1 if flag & 0x80 else 0)], dtype=np.uint8)
            q = np.where((q < 33) | (q > 126), 0x7F, q).astype(np.uint8)
            f[10] = (q[::-1] if flag & 0x10 else q).tobytes()
            assert len(f[10]) == len(f[9])
        out.append(b"\t".join(f))
    return b"\n".join(out)


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=8192, max_bases=8192 * 160)
    aln.set_contigs(ix)
    yield salt_amd, ix, aln, disc_check.Genome()
    aln.close()
    ix.destroy()


def _opt(salt_amd, ix, args):
    return salt_amd.AlnOpt.from_argv(list(args), ix.l_seed)[0]


def fetch(aln):
    return aln.disc_fetch(ALT, 0, REF_LEN), aln.disc_fetch(DIFF, 0, REF_LEN + 1)


def check(what, got, want, events=True):
    for k, name in enumerate(("alt", "diff")):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, name)
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero(got[k] != want[k])
            raise AssertionError("%s: %d words of %s differ; first at %s: device %s, twin %s" % (what, len(bad), name, bad[:3], got[k][bad[:3]].tolist(), want[k][bad[:3]].tolist()))
    assert not events or want[0].any()


def counted(aln, min_mapq, min_baseq, call):
    aln.disc_enable(True, min_mapq, min_baseq)
    aln.disc_reset()
    try:
        out = call()
        return out, fetch(aln)
    finally:
        aln.disc_enable(False, min_mapq, min_baseq)


def text_call(salt_amd, ix, aln, args, fqs, min_mapq=0, min_baseq=0):
    opt = _opt(salt_amd, ix, args)
    if len(fqs) == 1:
        return counted(aln, min_mapq, min_baseq, lambda: aln.align_se_text(opt, fqs[0])[0])
    return counted(aln, min_mapq, min_baseq, lambda: aln.align_pe_text(opt, ix, fqs[0], fqs[1])[0])


@pytest.fixture(scope="module")
def text_arrays(lam):
    """name -> (SAM of the text call, (alt, diff) of that call at floors 0 / 0): computed once, shared"""
    salt_amd, ix, aln, _ = lam
    return {name: text_call(salt_amd, ix, aln, args, [_fq(f) for f in files]) for name, (args, files) in ALL_SETS.items()}


def test_before_the_first_enable_the_errors(lam):
    salt_amd, ix, _, _ = lam
    other = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    other.set_contigs(ix)
    try:
        for call in (other.disc_reset, lambda: other.disc_fetch(ALT, 0, 1), lambda: other.disc_add(DIFF, 0, np.zeros(1, dtype=np.uint32)), other.disc_text, other.disc_uncount):
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
        with pytest.raises(salt_amd.SaltError, match="256"):
            other.disc_enable(True, 256, 20)
        with pytest.raises(salt_amd.SaltError, match="94"):
            other.disc_enable(True, 20, 94)
        other.disc_enable(False)                                       # stopping what never ran is no error, and allocates nothing
        with pytest.raises(salt_amd.SaltError, match="never enabled"):
            other.disc_fetch(ALT, 0, 1)
    finally:
        other.close()


@pytest.mark.parametrize("name", sorted(ALL_SETS))
def test_text_call_arrays_equal_the_twin_and_the_python_statement(name, lam, text_arrays):
    salt_amd, ix, _, genome = lam
    sam, got = text_arrays[name]
    want = salt_amd.disc_add_sam(ix, sam, 0, 0)
    check(name, got, want[:2])
    py = disc_check.add_sam(genome, sam, 0, 0)
    check(name + " python", got, py[:2])
    assert want[2] == py[2] > 0


def test_the_gap_fixtures_hold_m_runs_of_one_to_eight_columns_and_the_paired_sets_soft_clips(lam, text_arrays):
    # an M column over a genome N (mask 0): the aligner rarely lays a read there, gap_pe_short has one
    n_pos = np.flatnonzero(lam[3].masks == 0)
    depth = np.cumsum(text_arrays["gap_pe_short"][1][1][:-1].astype(np.int64)) % (1 << 32)
    assert len(n_pos) == 60 and int(depth[n_pos].sum()) >= 1 and not text_arrays["gap_pe_short"][1][0][n_pos].any()
    for name, want_clips in (("gap_se_mid", False), ("gap_pe_short", True), ("ragged_pe", True)):
        lens, clips = set(), 0
        for f in sam_records(text_arrays[name][0]):
            if int(f[1]) & 4:
                continue
            ops = re.findall(rb"(\d+)([MIDS])", f[5])
            if len(ops) > 1:
                lens |= {int(n) for n, op in ops if op == b"M" and int(n) <= 8}
                clips += sum(1 for n, op in ops if op == b"S")
        assert (lens >= set(range(1, 9))) or name == "ragged_pe", (name, lens)
        assert (clips > 0) == want_clips


@pytest.mark.parametrize("name", sorted(ALL_SETS))
def test_text_call_at_the_default_floors_filters_mapq_and_quality(name, lam, text_arrays):
    salt_amd, ix, aln, genome = lam
    args, files = ALL_SETS[name]
    fqs = [ramp_quals(_fq(f), k) for k, f in enumerate(files)]
    sam, got = text_call(salt_amd, ix, aln, args, fqs, 20, 20)
    st = {}
    py = disc_check.add_sam(genome, sam, 20, 20, st)
    check(name, got, salt_amd.disc_add_sam(ix, sam, 20, 20)[:2])
    check(name + " python", got, py[:2])
    assert st["below"] > 0 and st["passed"] > 0 and not np.array_equal(got[0], text_arrays[name][1][0])


def ramp_quals(fq, k):
    """the strict 4-line FASTQ with its quality lines rewritten: a ramp over all of 33 .. 126"""
    lines = fq.split(b"\n")
    for i in range(3, len(lines) - 1, 4):
        lines[i] = bytes(33 + (i + k + j) % 94 for j in range(len(lines[i])))
    return b"\n".join(lines)


def _read_set(salt_amd, files):
    if len(files) == 1:
        return salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
    return salt_amd.interleave_pairs(salt_amd.read_fastq(os.path.join(LAMBDA, files[0])), salt_amd.read_fastq(os.path.join(LAMBDA, files[1])))


def _quals_of(names, offs, flat, pe):
    out = {(bytes(nm), (i & 1) if pe else 0): flat[offs[i]:offs[i + 1]] for i, nm in enumerate(names)}
    assert len(out) == len(names)
    return out


def _pattern(seed, n):
    """n quality bytes over the whole byte range, 0 and 255 and the floor's neighbours often"""
    rng = np.random.RandomState(seed)
    q = rng.randint(33, 127, size=n).astype(np.uint8)
    special = np.array([0, 255, 10, 32, 127, 33, 52, 53, 54, 126], dtype=np.uint8)
    pick = rng.randint(0, 3, size=n) == 0
    q[pick] = special[rng.randint(0, len(special), size=int(pick.sum()))]
    return q


@pytest.mark.parametrize("name", ["se_default", "gap_se_mid", "pe_default", "gap_pe_short"])
def test_host_buffer_calls_with_and_without_set_quals(name, lam, text_arrays):
    salt_amd, ix, aln, _ = lam
    pe = name in PE_SETS
    args, files = ALL_SETS[name]
    names, seqs, offs, quals = _read_set(salt_amd, files)
    opt = _opt(salt_amd, ix, args)
    call = (lambda: aln.alnpe_core1(opt, ix, seqs, offs)) if pe else (lambda: aln.alnse_core1(opt, seqs, offs))
    sam = text_arrays[name][0]
    # without qualities every event counts, whatever the floor: the twin over QUAL *
    _, got = counted(aln, 0, 93, call)
    check(name + " without", got, salt_amd.disc_add_sam(ix, sam_with_quals(sam, None), 0, 93)[:2])
    check(name + " without = floor 0", got, text_arrays[name][1])
    # with the fixture's own at floor 30
    own = np.frombuffer(b"".join(quals), dtype=np.uint8)
    aln.set_quals(own)
    _, got = counted(aln, 0, 30, call)
    check(name + " own", got, salt_amd.disc_add_sam(ix, sam, 0, 30)[:2])
    # with the pattern, bytes 0 and 255 among it; the bytes are consumed: the call behind it counts without again
    flat = _pattern(11, len(own))
    aln.set_quals(flat)
    _, got = counted(aln, 20, 20, call)
    check(name + " pattern", got, salt_amd.disc_add_sam(ix, sam_with_quals(sam, _quals_of(names, offs, flat, pe)), 20, 20)[:2])
    _, again = counted(aln, 20, 20, call)
    check(name + " consumed", again, salt_amd.disc_add_sam(ix, sam_with_quals(sam, None), 20, 20)[:2])
    assert not np.array_equal(again[0], got[0])


def test_resident_entry_points_with_device_quals_on_the_callers_stream(lam, text_arrays):
    import torch
    salt_amd, ix, aln, _ = lam
    isz = salt_amd.RESULT_DTYPE.itemsize
    st = torch.cuda.Stream()
    for name in ("ragged_default", "ragged_pe"):
        args, files = ALL_SETS[name]
        names, seqs, offs, quals = _read_set(salt_amd, files)
        n, max_len = len(offs) - 1, int(np.diff(offs).max())
        flat = _pattern(13, int(offs[-1]))
        d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(64, dtype=np.uint8)])).cuda()
        d_quals = torch.from_numpy(flat.copy()).cuda()
        d_offs = torch.from_numpy(np.asarray(offs).astype(np.int32)).cuda()
        d_res = torch.zeros(n * isz, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        opt = _opt(salt_amd, ix, args)

        def call():
            with torch.cuda.stream(st):
                if len(files) == 1:
                    aln.align_resident(opt, n, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
                else:
                    aln.align_pe_resident(opt, ix, n // 2, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)

        sam = text_arrays[name][0]
        aln.set_quals(d_quals.data_ptr(), on_device=True)
        _, got = counted(aln, 0, 20, call)                             # (disc_fetch synchronises the device)
        check(name + " device quals", got, salt_amd.disc_add_sam(ix, sam_with_quals(sam, _quals_of(names, offs, flat, len(files) == 2)), 0, 20)[:2])
        _, got = counted(aln, 0, 20, call)
        check(name + " none", got, text_arrays[name][1])


def test_two_calls_add_a_fork_shares_the_arrays_reset_off_and_uncount(lam, text_arrays):
    salt_amd, ix, aln, _ = lam
    opt_se, opt_pe = _opt(salt_amd, ix, SE_SETS["se_default"][0]), _opt(salt_amd, ix, PE_SETS["ragged_pe"][0])
    fq, fq1, fq2 = _fq("reads_se.fq"), _fq("reads_ragged_pe_1.fq"), _fq("reads_ragged_pe_2.fq")
    (sam_one, one), (_, two) = text_arrays["se_default"], text_arrays["ragged_pe"]
    zero = (np.zeros(REF_LEN, dtype=np.uint64), np.zeros(REF_LEN + 1, dtype=np.uint32))
    aln.disc_enable(True, 0, 0)
    aln.disc_reset()
    fork = aln.fork()
    try:
        sam_on, _ = aln.align_se_text(opt_se, fq)
        aln.align_se_text(opt_se, fq)
        check("two calls", fetch(aln), (2 * one[0], 2 * one[1]))
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        check("fork", fetch(fork), (2 * one[0] + two[0], 2 * one[1] + two[1]))
        assert np.array_equal(aln.disc_fetch(ALT, 100, 50), (2 * one[0] + two[0])[100:150]) and aln.disc_fetch(ALT, REF_LEN, 0).shape == (0,)
        assert aln.disc_fetch(DIFF, REF_LEN, 1).shape == (1,)
        for call in (lambda: aln.disc_fetch(ALT, REF_LEN - 1, 2), lambda: aln.disc_fetch(DIFF, REF_LEN, 2), lambda: aln.disc_fetch(ALT, REF_LEN + 1, 0),
                     lambda: aln.disc_add(ALT, REF_LEN, np.ones(1, dtype=np.uint64)), lambda: aln.disc_add(DIFF, REF_LEN + 1, np.ones(1, dtype=np.uint32))):
            with pytest.raises(salt_amd.SaltError, match="leave"):
                call()
        with pytest.raises(salt_amd.SaltError, match="neither"):
            aln.disc_fetch(2, 0, 1)
        with pytest.raises(salt_amd.SaltError, match="300"):
            aln.disc_enable(True, 300, 0)
        for bad in (dict(min_alt=0), dict(min_alt=1 << 21), dict(min_pct=101)):
            with pytest.raises(salt_amd.SaltError, match="min_"):
                aln.disc_text(**bad)
        aln.disc_reset()
        check("reset", fetch(aln), zero, False)
        check("reset, fork", fetch(fork), zero, False)
        aln.disc_enable(False)
        sam_off, _ = aln.align_se_text(opt_se, fq)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        check("off", fetch(aln), zero, False)
        assert sam_on == sam_off == sam_one                            # the SAM bytes do not depend on the tally
        # a block that is aligned and then dropped leaves the arrays as they were; taking everything back leaves all-zero
        aln.disc_enable(True, 0, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        aln.align_se_text(opt_se, fq)
        fork.disc_uncount()
        check("uncount", fetch(aln), one)
        fork.disc_uncount()                                            # only once
        check("uncount twice", fetch(aln), one)
        aln.disc_uncount()
        check("all taken back", fetch(aln), zero, False)
        # disc_add: word by word, on top of what is there
        aln.disc_add(ALT, 0, one[0])
        aln.disc_add(ALT, 10, two[0][10:50000])
        aln.disc_add(DIFF, 0, one[1])
        aln.disc_add(DIFF, REF_LEN, np.array([7], dtype=np.uint32))
        want = (one[0].copy(), one[1].copy())
        want[0][10:50000] += two[0][10:50000]
        want[1][REF_LEN] += np.uint32(7)
        check("add", fetch(aln), want)
    finally:
        aln.disc_enable(False)
        aln.disc_reset()
        fork.close()


def test_reads_on_every_edge_of_a_word_at_a_time_compare(lam):
    salt_amd, ix, aln, genome = lam
    fq, info = edge_reads(genome_letters(), genome.masks)
    sam, got = text_call(salt_amd, ix, aln, ["-d", "-c"], [fq])
    st = {}
    py = disc_check.add_sam(genome, sam, 0, 0, st)
    check("edges", got, salt_amd.disc_add_sam(ix, sam, 0, 0)[:2])
    check("edges python", got, py[:2])
    # which of the planted bases the aligner laid where they were cut: each category occurs, and each is an event in alt
    seen = {}
    for f in sam_records(sam):
        g0, L, rev, g, cat = info[f[0]]
        placed = not int(f[1]) & 4 and genome.offsets[f[2].decode()] + int(f[3]) - 1 == g0 and f[5] == b"%dM" % L and bool(int(f[1]) & 16) == bool(rev)
        if placed and g is not None:
            assert got[0][g] != 0, (f[0], g)
            seen.setdefault(cat, set()).add((rev, g0 & 7, g - g0))
        if placed and cat == "read_n":
            assert got[0][g0 + 8] == 0
            seen.setdefault(cat, set()).add((rev, 0, 8))
    for k in range(8):
        for col in (0, 7, 8, 31, 32, 98, 99):
            assert {r for r, _, _ in seen.get("start%d_col%d" % (k, col), ())} == {0, 1}, (k, col)
    assert {g7 for c, v in seen.items() if c.startswith("start") for _, g7, _ in v} == set(range(8))
    for L in (100, 120, 121, 511, 512):
        assert {(r, c) for r, _, c in seen["len%d" % L]} >= {(0, L - 1), (1, L - 1), (0, 0), (1, 0)}, L
    for cat in ("genome_end", "site2", "site3", "read_n"):
        assert {r for r, _, _ in seen[cat]} == {0, 1}, cat
    assert got[0][REF_LEN - 1] != 0 and int(got[1][REF_LEN]) != 0                  # the last position and the cut's word
    assert st["at_sites"] >= 8 and st["events"] >= 8 * 2 * 7


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_around_the_wave_and_the_block(n, lam):
    salt_amd, ix, aln, _ = lam
    fq = b"\n".join(_fq("reads_se.fq").split(b"\n")[:4 * n]) + b"\n"
    sam, got = text_call(salt_amd, ix, aln, ["-d", "-c"], [fq])
    assert len(sam_records(sam)) == n
    check("batch of %d" % n, got, salt_amd.disc_add_sam(ix, sam, 0, 0)[:2], False)


def test_a_hot_spot_of_2048_copies_is_exactly_2048_in_one_field(lam):
    salt_amd, ix, aln, genome = lam
    gen, g = genome_letters(), 15040
    assert bin(int(genome.masks[g])).count("1") == 1
    letter = b"ACGT"[[b for b in range(4) if not (int(genome.masks[g]) >> b) & 1][1]]      # the second base outside the mask: field 1
    read = make_read(gen, 15000, 100, 0, [(g, letter)])
    sam, got = text_call(salt_amd, ix, aln, ["-d", "-c"], [fastq_of([(b"h%d" % i, read) for i in range(2048)])])
    check("hot spot", got, salt_amd.disc_add_sam(ix, sam, 0, 0)[:2])
    assert int(got[0][g]) == 2048 << 21 and not got[0][g - 1] and not got[0][g + 1] and int(np.count_nonzero(got[0])) == 1
    assert int(got[1][15000]) == 2048 and int(got[1][15100]) == (1 << 32) - 2048


def planted_reads(gen, masks):
    """24 reads: 12, half of them reverse, carry a base the index does not have at one plain position; 12 more a third allele at a known
    site.  The positions next to the planted ones are covered controls."""
    plain = 30040
    site = [int(g) for g in np.flatnonzero(np.isin(masks, (3, 5, 6, 9, 10, 12))) if 33000 < g < 40000][0]
    assert bin(int(masks[plain])).count("1") == 1 and bin(int(masks[plain + 1])).count("1") == 1
    reads = []
    for tag, g in ((b"p", plain), (b"s", site)):
        for i in range(12):
            reads.append((b"%s%d" % (tag, i), make_read(gen, g - 5 - 7 * i, 100, i & 1, [(g, outside(int(masks[g])))])))
    return fastq_of(reads), plain, site


def test_planted_snps_are_the_file_at_the_defaults(lam):
    salt_amd, ix, aln, genome = lam
    fq, plain, site = planted_reads(genome_letters(), genome.masks)
    sam, got = text_call(salt_amd, ix, aln, ["-d", "-c"], [fq], 20, 20)
    py = disc_check.add_sam(genome, sam, 20, 20)
    check("planted", got, py[:2])
    assert py[2] == 24 and all(int(f[4]) >= 20 for f in sam_records(sam))
    aln.disc_enable(True, 20, 20)
    aln.disc_enable(False, 20, 20)
    text = aln.disc_text()                                             # the arrays of the call are still there
    assert text == disc_check.text(genome, py[0], py[1]) == salt_amd.disc_text(ix, got[0], got[1])
    rows = {(r[0], r[1]): r for r in disc_check.parse(text)}
    assert rows[("lambdaA", plain + 1)][4] == 12 and sorted(x for x in rows[("lambdaA", plain + 1)][5] if x is not None) == [0, 0, 12]
    assert len(rows[("lambdaA", site + 1)][2].split("/")) == 3 and rows[("lambdaA", site + 1)][5].count(None) == 2
    assert ("lambdaA", plain + 2) not in rows and ("lambdaA", site) not in rows and len(rows) == 2      # the covered controls have no line


def _gunzip_members(data):
    import zlib
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        data = d.unused_data
    return b"".join(out)


def W(a=0, b=0, c=0):
    return a | b << 21 | c << 42


@pytest.fixture(scope="module")
def hand_made(lam, text_arrays):
    """hand-made arrays on the device through disc_add: a call's own words, candidates at 0, at 63 | 64, at ref_len - 1 and on both sides of
    the contig boundary, every position of [4096, 4160) a candidate, and a long stretch without any"""
    salt_amd, ix, aln, genome = lam
    alt, diff = text_arrays["gap_se_mid"][1][0].copy(), text_arrays["gap_se_mid"][1][1].copy()
    alt[60000:] = 0                                                    # tiles without a candidate
    for g in (0, 63, 64, BOUND - 1, BOUND, REF_LEN - 1):
        alt[g] = W(900, 0, 900)
    alt[4096:4160] = W(800, 800, 800)
    aln.disc_enable(True, 0, 0)
    aln.disc_enable(False, 0, 0)
    aln.disc_reset()
    aln.disc_add(ALT, 0, alt)
    aln.disc_add(DIFF, 0, diff)
    return alt, diff


@pytest.mark.parametrize("tile", [64, 1000, 48502, 97004, 0])
@pytest.mark.parametrize("rule", [(3, 20, False), (1, 0, True)])
def test_device_text_equals_the_twins_byte_for_byte(tile, rule, lam, hand_made):
    salt_amd, ix, aln, genome = lam
    alt, diff = hand_made
    want, want_seen = salt_amd.disc_text(ix, alt, diff, *rule, seen=True)
    pieces, seen = aln.disc_text(*rule, tile_positions=tile, pieces=True, seen=2)
    assert b"".join(pieces) == want and want == disc_check.text(genome, alt, diff, *rule)
    assert seen.tolist() == want_seen.tolist() == [1, 1]
    rows = {(r[0], r[1]) for r in disc_check.parse(want)}
    assert {("lambdaA", 1), ("lambdaA", 64), ("lambdaA", 65), ("lambdaA", BOUND), ("lambdaB_div2pct", 1), ("lambdaB_div2pct", REF_LEN - BOUND)} <= rows
    assert all(p.endswith(b"\n") for p in pieces)
    if tile == 64:
        n_tiles_with = len({(0 if c == "lambdaA" else BOUND) + p - 1 >> 6 for c, p in rows})
        assert len(pieces) > n_tiles_with                                                   # the 64 lines of [4096, 4160) outgrow a tile's buffer: they leave in pieces cut at line ends
        assert n_tiles_with < (REF_LEN + 63) // 64 - (20 if rule[2] else 1000)              # ... and tiles without a line yield no piece (with all, the index's sites leave few)
    if tile == 0:
        assert len(pieces) == 1


def test_bgzf_pieces_inflate_to_the_text_twice_the_same_and_the_arrays_stay(lam, hand_made):
    salt_amd, ix, aln, genome = lam
    alt, diff = hand_made
    want = salt_amd.disc_text(ix, alt, diff, 1, 0, True)
    z = aln.disc_text(1, 0, True, tile_positions=1000, bgzf=True, pieces=True)
    assert len(z) > 10 and all(p[:4] == b"\x1f\x8b\x08\x04" for p in z)
    assert _gunzip_members(b"".join(z)) == want == gzip.decompress(b"".join(z))
    assert not b"".join(z).endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))      # no end-of-file block
    assert aln.disc_text(1, 0, True, tile_positions=1000, bgzf=True, pieces=True) == z and aln.disc_text(1, 0, True) == want
    check("only read", fetch(aln), (alt, diff))


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("discidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


LOOSE = ["--discover-min-mapq", "0", "--discover-min-baseq", "0", "--discover-min-alt", "1", "--discover-min-pct", "0"]


def _want_file(salt_amd, ix, sam, min_mapq=0, min_baseq=0, min_alt=1, min_pct=0, all_sites=False):
    alt, diff, n = salt_amd.disc_add_sam(ix, sam, min_mapq, min_baseq)
    assert n > 0
    return salt_amd.disc_text(ix, alt, diff, min_alt, min_pct, all_sites)


def test_cli_file_equals_the_twin_over_its_stdout_plain_gz_and_gz_input(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _, _ = lam
    reads = os.path.join(LAMBDA, "reads_se.fq")
    f, fz = tmp_path / "found.txt", tmp_path / "found.txt.gz"
    run = subprocess.run([SALT, "-d", "-c", "--discover", str(f)] + LOOSE + [lambda_cli_index, reads], capture_output=True, timeout=300)
    assert run.returncode == 0 and b"text path" in run.stderr and b"counted and printed on the device" in run.stderr, run.stderr[-600:]
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read() and b"have no line" not in run.stderr
    want = _want_file(salt_amd, ix, run.stdout)
    assert f.read_bytes() == want and want.count(b"\n") == 1230
    rz = tmp_path / "reads.fq.gz"
    rz.write_bytes(salt_amd.bgzf_deflate(open(reads, "rb").read()))
    gz = subprocess.run([SALT, "-d", "-c", "--discover", str(fz), "--discover-all"] + LOOSE + [lambda_cli_index, str(rz)], capture_output=True, timeout=300)
    assert gz.returncode == 0 and strip_pg(gz.stdout) == strip_pg(run.stdout), gz.stderr[-600:]
    z = fz.read_bytes()
    assert z.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")) and _gunzip_members(z) == _want_file(salt_amd, ix, run.stdout, all_sites=True)
    # the defaults on a shallow run: an empty file, and the warning names the first contig without a line
    d = subprocess.run([SALT, "-d", "-c", "--discover", str(f), lambda_cli_index, reads], capture_output=True, timeout=300)
    assert d.returncode == 0 and f.read_bytes() == b"" and b"2 of 2 contigs have no line" in d.stderr and b"the first is lambdaA:" in d.stderr


def test_cli_planted_snps_rebuild_an_index_that_knows_them(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _, genome = lam
    fq, plain, site = planted_reads(genome_letters(), genome.masks)
    reads, f = tmp_path / "planted.fq", tmp_path / "snps_all.txt"
    reads.write_bytes(fq)
    run = subprocess.run([SALT, "-d", "-c", "--discover", str(f), "--discover-all", lambda_cli_index, str(reads)], capture_output=True, timeout=300)
    assert run.returncode == 0 and b"have no line" not in run.stderr, run.stderr[-600:]
    assert f.read_bytes() == _want_file(salt_amd, ix, run.stdout, 20, 20, 3, 20, True)
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), str(f), str(tmp_path / "new")], check=True, stderr=subprocess.DEVNULL, timeout=600)
    import snp_check
    masks = snp_check.sites_of_ref(str(tmp_path / "new.ref"))[1]
    changed = np.flatnonzero(masks != genome.masks)
    assert changed.tolist() == sorted((plain, site)) and all(bin(int(masks[g])).count("1") == bin(int(genome.masks[g])).count("1") + 1 for g in changed)


def test_cli_under_polish_and_bam_the_file_is_the_plain_runs(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _, _ = lam
    reads = os.path.join(LAMBDA, "reads_se.fq")
    want = _want_file(salt_amd, ix, open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read())      # (the plain run's stdout)
    fp, fb = tmp_path / "found_polish.txt", tmp_path / "found_bam.txt"
    pol = subprocess.run([SALT, "-d", "-c", "--polish", "--discover", str(fp)] + LOOSE + [lambda_cli_index, reads], capture_output=True, timeout=300)
    assert pol.returncode == 0 and b"on the device" in pol.stderr, pol.stderr[-600:]
    assert fp.read_bytes() == want
    bam = subprocess.run([SALT, "-d", "-c", "--bam", "--discover", str(fb)] + LOOSE + [lambda_cli_index, reads], capture_output=True, timeout=300)
    assert bam.returncode == 0 and bam.stdout[:4] == b"\x1f\x8b\x08\x04" and fb.read_bytes() == want, bam.stderr[-600:]


def test_cli_paired_end_text_path_and_host_pipeline_hand_the_qualities_over(lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _, _ = lam
    args, files = PE_SETS["ragged_pe"]
    f = tmp_path / "found.txt"
    floors = ["--discover-min-mapq", "0", "--discover-min-baseq", "30", "--discover-min-alt", "1", "--discover-min-pct", "0"]
    reads = []
    for k, x in enumerate(files):                                      # (the fixture's qualities are all 'I')
        reads.append(str(tmp_path / ("ramp_%d.fq" % k)))
        open(reads[-1], "wb").write(ramp_quals(_fq(x), k))
    for env, word in ((dict(os.environ), b"text path"), (dict(os.environ, SALT_HOST_PIPELINE="1"), b"host phases")):
        run = subprocess.run([SALT] + list(args) + ["--discover", str(f)] + floors + [lambda_cli_index] + reads,
                             capture_output=True, timeout=300, env=env)
        assert run.returncode == 0 and word in run.stderr and b"on the device" in run.stderr, run.stderr[-600:]
        assert f.read_bytes() == _want_file(salt_amd, ix, run.stdout, 0, 30) != _want_file(salt_amd, ix, run.stdout, 0, 0)


def test_cli_counts_every_written_block_once_across_the_hand_over(lam, lambda_cli_index, tmp_path):
    """A multi-line record in the middle of the file, chunks of 9 000 bytes: the blocks the workers had aligned behind the refused chunk
    are dropped and their adds taken back (salt_gpu_ws_disc_uncount); the host pipeline aligns those reads again."""
    salt_amd, ix, _, _ = lam
    recs = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq, f = tmp_path / "mid_multiline.fq", tmp_path / "found.txt"
    fq.write_bytes(b"\n".join(out) + b"\n")
    run = subprocess.run([SALT, "-d", "-c", "-t", "8", "--discover", str(f)] + LOOSE + [lambda_cli_index, str(fq)], capture_output=True, timeout=300,
                         env=dict(os.environ, SALT_CHUNK_BYTES="9000"))
    assert run.returncode == 0, run.stderr[-600:]
    assert b"the host parser takes over" in run.stderr and b"on the device" in run.stderr
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert f.read_bytes() == _want_file(salt_amd, ix, run.stdout)
