"""The error profile on the device: k_errprof behind every entry point that leaves result rows against the host twin (salt_errprof_add_sam)
over the SAM text the same call returned AND against the Python statement (tests/errprof_check.py) -- single and paired end, text,
host-buffer and resident entry points, with and without qualities, under polish --, the state of the tables (two calls, a fork, reset,
off, uncount), small synthetic batches at the shapes where the kernel takes another path, and `salt --error-profile` end to end."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import errprof_check as ec
import gap_cases
from conftest import EXTRA_CASES, LAMBDA, ROOT

pytestmark = pytest.mark.gpu

EDGE, REF_LEN = 48502, 97004
CHUNK, TILE = 1024, 16                      # reads a workgroup of k_errprof owns; cycles of its LDS table

SE_SETS = {
    "se_default": (["-d", "-c"], ["reads_se.fq"]), "ragged_default": EXTRA_CASES["ragged_default"], "span_default": EXTRA_CASES["span_default"],
    "gap_se_mid": (gap_cases.GAP_CASES["gap_se_mid"][0], ["reads_gap_se_mid.fq.gz"]),
}
PE_SETS = {
    "pe_default": (["-d", "-p", "-c", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"]), "ragged_pe": EXTRA_CASES["ragged_pe"],
    "gap_pe_short": (gap_cases.GAP_CASES["gap_pe_short"][0], ["reads_gap_pe_short_1.fq.gz", "reads_gap_pe_short_2.fq.gz"]),
}


def _fq(name):
    data = open(os.path.join(LAMBDA, name), "rb").read()
    return gzip.decompress(data) if name.endswith(".gz") else data


def _opt(salt_amd, ix, args):
    return salt_amd.AlnOpt.from_argv(list(args), ix.l_seed)[0]


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=8192, max_bases=8192 * 160)
    aln.set_contigs(ix)
    yield salt_amd, ix, aln
    aln.close()
    ix.destroy()


@pytest.fixture(scope="module")
def model():
    masks, offsets = ec.lambda_masks(), ec.lambda_offsets()
    return lambda sam, q=0: ec.tables_of_sam(masks, offsets, sam, q)


def _check(salt_amd, ix, model, got, sam, min_mapq=0, skipped=0, what=""):
    """the device's (E, R) = the twin over the SAM = the Python statement; a skipped read prints as an empty line, so only the device sees it"""
    E, R = got
    assert E.dtype == np.uint64 and E.shape == ec.SHAPE and R.shape == (2, 8)
    tE, tR, _ = salt_amd.errprof_add_sam(ix, sam, min_mapq)
    mE, mR, _ = model(sam, min_mapq)
    assert np.array_equal(tE, mE) and np.array_equal(tR, mR), what
    assert int(R[:, 1].sum()) == skipped and not R[:, 7].any(), (what, R.tolist())
    R = R.copy()
    R[:, 0] -= R[:, 1]
    R[:, 1] = 0
    assert np.array_equal(R, tR), (what, R.tolist(), tR.tolist())
    if not np.array_equal(E, tE):
        bad = np.argwhere(E != tE)
        raise AssertionError("%s: %d cells differ; first [mate cycle q ref read] %s: device %s, twin %s" %
                             (what, len(bad), bad[:4].tolist(), [int(E[tuple(b)]) for b in bad[:4]], [int(tE[tuple(b)]) for b in bad[:4]]))
    return E, R


def _text_call(aln, call, min_mapq=0):
    """the call's SAM and what it alone added to the tables"""
    aln.errprof_enable(True, min_mapq)
    aln.errprof_table(reset=True)
    sam = call()
    got = aln.errprof_table()
    aln.errprof_enable(False)
    return sam, got


def test_before_the_first_enable_the_errors_and_nothing_allocated(lam):
    salt_amd, ix, _ = lam
    other = salt_amd.GpuAligner(ix, device=0, max_reads=64)
    try:
        for call in (other.errprof_table, other.errprof_uncount):
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
        with pytest.raises(salt_amd.SaltError, match="255"):
            other.errprof_enable(True, 256)
        other.errprof_enable(False)                                  # stopping what never ran is no error, and allocates nothing:
        with pytest.raises(salt_amd.SaltError, match="never enabled"):      # the tables are still not there
            other.errprof_table()
        other.errprof_enable(True, 255)
        E, R = other.errprof_table()
        assert not E.any() and not R.any()
        lib = salt_amd.gpu_lib()
        small = np.zeros(10, dtype=np.uint64)
        assert lib.salt_gpu_index_errprof_fetch(other._ix, small.ctypes.data, small.size, None, 0) == -1
        assert b"1556480" in lib.salt_gpu_last_error() and b"10" in lib.salt_gpu_last_error()
        assert lib.salt_gpu_index_errprof_fetch(other._ix, None, 0, None, 1) == 0      # reset only
    finally:
        other.close()


@pytest.fixture(scope="module")
def se_tabs(lam):
    """name -> {"sam", 0: (E, R), 20: (E, R)} of the single-end text call"""
    salt_amd, ix, aln = lam
    out = {}
    for name, (args, files) in SE_SETS.items():
        opt, fq = _opt(salt_amd, ix, args), _fq(files[0])
        per_q = {}
        for q in (0, 20):
            sam, per_q[q] = _text_call(aln, lambda: aln.align_se_text(opt, fq)[0], q)
            assert sam == per_q.setdefault("sam", sam)
        out[name] = per_q
    return out


@pytest.fixture(scope="module")
def pe_tabs(lam):
    salt_amd, ix, aln = lam
    out = {}
    for name, (args, files) in PE_SETS.items():
        opt, fq1, fq2 = _opt(salt_amd, ix, args), _fq(files[0]), _fq(files[1])
        per_q = {}
        for q in (0, 20):
            sam, per_q[q] = _text_call(aln, lambda: aln.align_pe_text(opt, ix, fq1, fq2)[0], q)
            assert sam == per_q.setdefault("sam", sam)
        out[name] = per_q
    return out


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("name", sorted(SE_SETS))
def test_single_end_text_call(name, min_mapq, lam, model, se_tabs):
    salt_amd, ix, _ = lam
    E, R = _check(salt_amd, ix, model, se_tabs[name][min_mapq], se_tabs[name]["sam"], min_mapq, what=name)
    assert E.any() and not E[1].any() and int(R[0, 4]) > 0


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("name", sorted(PE_SETS))
def test_paired_end_text_call(name, min_mapq, lam, model, pe_tabs):
    salt_amd, ix, _ = lam
    E, R = _check(salt_amd, ix, model, pe_tabs[name][min_mapq], pe_tabs[name]["sam"], min_mapq, what=name)
    assert E[0].any() and E[1].any() and int(R[0, 0]) == int(R[1, 0])


def test_the_calls_cover_qualities_indels_clips_and_the_contig_boundary(se_tabs, pe_tabs):
    """None of the comparisons above passes on empty ground."""
    import snp_check
    assert len(np.flatnonzero(se_tabs["se_default"][0][0].sum(axis=(0, 1, 3, 4)))) == 21            # 21 quality values
    assert snp_check.census(se_tabs["gap_se_mid"]["sam"])[0] >= 1000 and int(se_tabs["gap_se_mid"][0][1][0, 6]) >= 500
    assert snp_check.census(pe_tabs["gap_pe_short"]["sam"])[0] >= 300
    assert snp_check.census(pe_tabs["pe_default"]["sam"])[1] >= 40 and int(pe_tabs["pe_default"][0][1][:, 6].sum()) >= 40      # rescued mates' clips
    assert se_tabs["gap_se_mid"][0][0][0, 160:168].any() and not se_tabs["gap_se_mid"][0][0][0, 168:].any()
    assert int(se_tabs["span_default"][0][1][0, 4]) == 40


def _read_set(salt_amd, files):
    if len(files) == 1:
        return salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
    return salt_amd.interleave_pairs(salt_amd.read_fastq(os.path.join(LAMBDA, files[0])), salt_amd.read_fastq(os.path.join(LAMBDA, files[1])))


@pytest.mark.parametrize("name", ["se_default", "gap_se_mid", "pe_default", "gap_pe_short"])
def test_host_buffer_calls_with_and_without_set_quals(name, lam, model, se_tabs, pe_tabs):
    salt_amd, ix, aln = lam
    pe = name in PE_SETS
    args, files = (PE_SETS if pe else SE_SETS)[name]
    names, seqs, offs, quals = _read_set(salt_amd, files)
    opt = _opt(salt_amd, ix, args)
    call = (lambda: aln.alnpe_core1(opt, ix, seqs, offs)) if pe else (lambda: aln.alnse_core1(opt, seqs, offs))
    want = (pe_tabs if pe else se_tabs)[name]
    # without: every event in q = none, the other coordinates those of the text call
    _, (E, R) = _text_call(aln, call, 20)
    assert np.array_equal(R, want[20][1]) and not E[:, :, :94].any() and np.array_equal(E[:, :, 94], want[20][0].sum(axis=2))
    # with: the text call's table, cell for cell; the bytes are consumed: a second call counts in none again
    flat = np.frombuffer(b"".join(quals), dtype=np.uint8)
    aln.errprof_enable(True, 20)
    aln.errprof_table(reset=True)
    aln.set_quals(flat)
    call()
    E, R = aln.errprof_table(reset=True)
    assert np.array_equal(E, want[20][0]) and np.array_equal(R, want[20][1])
    call()
    E2, _ = aln.errprof_table()
    assert not E2[:, :, :94].any() and np.array_equal(E2[:, :, 94], E.sum(axis=2))
    # uncount of a host-buffer call whose quals were consumed: back to the cell
    aln.errprof_table(reset=True)
    aln.set_quals(flat)
    call()
    aln.errprof_uncount()
    E3, R3 = aln.errprof_table()
    aln.errprof_enable(False)
    assert not E3.any() and not R3.any()


def test_resident_entry_points_with_device_quals_on_the_callers_stream(lam, se_tabs, pe_tabs):
    import torch
    salt_amd, ix, aln = lam
    isz = salt_amd.RESULT_DTYPE.itemsize
    st = torch.cuda.Stream()
    for name, sets, want in (("ragged_default", SE_SETS, se_tabs), ("ragged_pe", PE_SETS, pe_tabs)):
        args, files = sets[name]
        _, seqs, offs, quals = _read_set(salt_amd, files)
        n, max_len = len(offs) - 1, int(np.diff(offs).max())
        d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(64, dtype=np.uint8)])).cuda()
        d_quals = torch.from_numpy(np.frombuffer(b"".join(quals), dtype=np.uint8).copy()).cuda()
        d_offs = torch.from_numpy(np.asarray(offs).astype(np.int32)).cuda()
        d_res = torch.zeros(n * isz, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        opt = _opt(salt_amd, ix, args)
        for with_q in (True, False):
            aln.errprof_enable(True, 0)
            aln.errprof_table(reset=True)
            if with_q:
                aln.set_quals(d_quals.data_ptr(), on_device=True)
            with torch.cuda.stream(st):
                if len(files) == 1:
                    aln.align_resident(opt, n, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
                else:
                    aln.align_pe_resident(opt, ix, n // 2, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
            E, R = aln.errprof_table()                               # (synchronises the device)
            aln.errprof_enable(False)
            assert np.array_equal(R, want[name][0][1])
            if with_q:
                assert np.array_equal(E, want[name][0][0])
            else:
                assert not E[:, :, :94].any() and np.array_equal(E[:, :, 94], want[name][0][0].sum(axis=2))
        # host bytes cannot serve a resident call
        lib = salt_amd.gpu_lib()
        host_q = np.zeros(16, dtype=np.uint8)
        lib.salt_gpu_ws_set_quals(aln._ws, host_q.ctypes.data, 0)
        with pytest.raises(salt_amd.SaltError, match="resident"):
            aln.align_resident(opt, 1, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)


def test_under_set_polish_the_table_is_the_plain_calls(lam, se_tabs, pe_tabs):
    salt_amd, ix, aln = lam
    aln.set_pac(ix)
    aln.set_polish(1)
    try:
        opt = _opt(salt_amd, ix, SE_SETS["se_default"][0])
        _, (E, R) = _text_call(aln, lambda: aln.align_se_text(opt, _fq("reads_se.fq"))[0])
        assert np.array_equal(E, se_tabs["se_default"][0][0]) and np.array_equal(R, se_tabs["se_default"][0][1])
        args, files = PE_SETS["ragged_pe"]
        _, (E, R) = _text_call(aln, lambda: aln.align_pe_text(_opt(salt_amd, ix, args), ix, _fq(files[0]), _fq(files[1]))[0])
        assert np.array_equal(E, pe_tabs["ragged_pe"][0][0]) and np.array_equal(R, pe_tabs["ragged_pe"][0][1])
    finally:
        aln.set_polish(0)


def test_two_calls_add_a_fork_shares_the_table_reset_off_and_uncount(lam, se_tabs, pe_tabs):
    salt_amd, ix, aln = lam
    opt_se, opt_pe = _opt(salt_amd, ix, SE_SETS["se_default"][0]), _opt(salt_amd, ix, PE_SETS["ragged_pe"][0])
    fq, fq1, fq2 = _fq("reads_se.fq"), _fq("reads_ragged_pe_1.fq"), _fq("reads_ragged_pe_2.fq")
    (E1, R1), (E2, R2) = se_tabs["se_default"][0], pe_tabs["ragged_pe"][0]
    aln.errprof_enable(True, 0)
    aln.errprof_table(reset=True)
    sam_on, _ = aln.align_se_text(opt_se, fq)
    aln.align_se_text(opt_se, fq)
    E, R = aln.errprof_table()
    assert np.array_equal(E, 2 * E1) and np.array_equal(R, 2 * R1)
    fork = aln.fork()
    try:
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        for a in (aln, fork):
            E, R = a.errprof_table()
            assert np.array_equal(E, 2 * E1 + E2) and np.array_equal(R, 2 * R1 + R2)
        E, R = fork.errprof_table(reset=True)
        assert E.any() and not aln.errprof_table()[0].any() and not aln.errprof_table()[1].any()
        # off: nothing is counted
        aln.errprof_enable(False)
        sam_off, _ = aln.align_se_text(opt_se, fq)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert not aln.errprof_table()[0].any() and not aln.errprof_table()[1].any()
        assert sam_on == sam_off == se_tabs["se_default"]["sam"]    # the SAM bytes do not depend on the profile
        # a block that is aligned and then dropped leaves the tables cell for cell as they were
        aln.errprof_enable(True, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        aln.align_se_text(opt_se, fq)
        fork.errprof_uncount()
        E, R = aln.errprof_table()
        assert np.array_equal(E, E1) and np.array_equal(R, R1)
        fork.errprof_uncount()                                       # only once
        assert np.array_equal(aln.errprof_table()[0], E1)
        aln.errprof_uncount()
        assert not aln.errprof_table()[0].any() and not aln.errprof_table()[1].any()
    finally:
        aln.errprof_enable(False)
        fork.close()


# ---- shapes where the kernel can go wrong: small synthetic batches, each against the twin and the model over the call's own SAM ----
def _records(name):
    lines = _fq(name).split(b"\n")
    return [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]


def _fastq(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def _genome():
    seqs, name = {}, None
    for line in open(os.path.join(LAMBDA, "genome.fa")).read().split("\n"):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        elif line:
            seqs[name].append(line.strip().upper())
    return "".join("".join(seqs[n]) for n in ("lambdaA", "lambdaB_div2pct"))


def _synthetic(lam, model, fq, what, min_events=1, opt_args=("-d", "-c")):
    salt_amd, ix, aln = lam
    opt = _opt(salt_amd, ix, opt_args)
    sam, got = _text_call(aln, lambda: aln.align_se_text(opt, fq)[0])
    E, R = _check(salt_amd, ix, model, got, sam, what=what)
    assert int(E.sum()) >= min_events, what
    return sam, E, R


@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_single_end_batch_sizes_around_a_wave_and_a_workgroups_chunk(n, lam, model):
    recs = _records("reads_se.fq")
    _, E, R = _synthetic(lam, model, _fastq([recs[i % len(recs)] for i in range(n)]), "%d records" % n, min_events=50)
    assert int(R[0, 0]) == n


@pytest.mark.parametrize("n", [1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_paired_end_batch_sizes_around_a_workgroups_chunk_of_one_mate(n, lam, model):
    salt_amd, ix, aln = lam
    r1, r2 = _records("reads_pe_1.fq"), _records("reads_pe_2.fq")
    fq1, fq2 = _fastq([r1[i % len(r1)] for i in range(n)]), _fastq([r2[i % len(r2)] for i in range(n)])
    opt = _opt(salt_amd, ix, PE_SETS["pe_default"][0])
    sam, got = _text_call(aln, lambda: aln.align_pe_text(opt, ix, fq1, fq2)[0])
    E, R = _check(salt_amd, ix, model, got, sam, what="%d pairs" % n)
    assert int(R[0, 0]) == int(R[1, 0]) == n and E[0].any() and E[1].any()


def test_no_records(lam):
    salt_amd, ix, aln = lam
    opt = _opt(salt_amd, ix, ["-d", "-c"])
    sam, (E, R) = _text_call(aln, lambda: aln.align_se_text(opt, b"")[0])
    assert sam == b"" and not E.any() and not R.any()
    aln.errprof_enable(True, 0)
    aln.errprof_uncount()                                            # nothing to take back
    aln.errprof_enable(False)


def test_read_lengths_around_the_tile_and_the_longest_in_one_batch(lam, model):
    g = _genome()
    recs = []
    for k, L in enumerate([1, TILE - 1, TILE, TILE + 1, 120, 121, 511, 512, 100, 33]):
        seq = g[3000 + 700 * k:3000 + 700 * k + L].replace("N", "A")
        recs.append([b"@len%d" % L, seq.encode(), b"+", bytes(33 + (k + j) % 94 for j in range(L))])
    sam, E, R = _synthetic(lam, model, _fastq(recs), "lengths", min_events=1000)
    assert int(R[0, 0]) == 10 and int(R[0, 4]) >= 6                   # the short ones may be unmapped: they still land in R
    assert E[0, 511].any() and E[0, 510].any()                       # the 512-base read reaches the last cycle


def test_2048_copies_of_one_read_fall_on_one_cell_per_cycle(lam, model):
    r = _records("reads_se.fq")[0]
    sam, E, R = _synthetic(lam, model, _fastq([[b"@c%d" % k] + r[1:] for k in range(2048)]), "2048 copies", min_events=2048 * 80)
    assert int(R[0, 4]) == 2048 and int(E.max()) == 2048 and len(np.flatnonzero(E)) <= 100


def test_2048_copies_with_qualities_cycling_through_all_94_values(lam, model):
    r = _records("reads_se.fq")[0]
    L = len(r[1])
    recs = [[b"@c%d" % k, r[1], b"+", bytes(33 + (k + j) % 94 for j in range(L))] for k in range(2048)]
    sam, E, R = _synthetic(lam, model, _fastq(recs), "2048 copies, 94 qualities", min_events=2048 * 80)
    per_q = E.sum(axis=(0, 1, 3, 4))
    assert per_q[:94].all() and per_q[94] == 0                       # every q bin of the LDS tile is used


@pytest.mark.parametrize("strand", [0, 16])
def test_all_forward_and_all_reverse_batches(strand, lam, model, se_tabs):
    recs, k, keep = _records("reads_se.fq"), 0, []
    for line in se_tabs["se_default"]["sam"].split(b"\n"):
        if line and not line.startswith(b"@"):
            f = line.split(b"\t")
            if not int(f[1]) & 4 and int(f[1]) & 16 == strand:
                keep.append(recs[k])
            k += 1
    sam, E, R = _synthetic(lam, model, _fastq(keep), "strand %d" % strand, min_events=50000)
    assert int(R[0, 5]) == (int(R[0, 4]) if strand else 0) and int(R[0, 4]) >= 800


def test_reads_with_n(lam, model):
    recs = []
    for k, r in enumerate(_records("reads_se.fq")[:300]):
        s = bytearray(r[1])
        for j in (k % len(s), (7 * k + 3) % len(s)):
            s[j] = ord("N")
        recs.append([r[0], bytes(s), r[2], r[3]])
    fq = _fastq(recs)
    sam, E, R = _synthetic(lam, model, fq, "reads with N", min_events=10000)
    st = {}
    ec.tables_of_sam(ec.lambda_masks(), ec.lambda_offsets(), sam, stats=st)
    assert st["read_n"] >= 300


def test_a_read_that_ends_at_the_genomes_last_position_over_a_site_and_over_an_n(lam, model):
    g = _genome()
    masks = ec.lambda_masks()
    inner = lambda a: int([x for x in a.tolist() if 200 <= x % EDGE < EDGE - 200][0])
    site, n_pos = inner(np.flatnonzero((masks & (masks - 1)) != 0)), inner(np.flatnonzero(masks == 0))
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
    recs = []
    for k, (a, L) in enumerate([(REF_LEN - 100, 100), (REF_LEN - 37, 37), (EDGE - 100, 100), (site - 50, 100), (site - 99, 100), (site, 100),
                                (n_pos - 50, 100), (n_pos - 3, 120), (0, 100), (EDGE, 64)]):
        seq = g[a:a + L].replace("N", "A")
        for rc in (False, True):
            s = "".join(comp[c] for c in reversed(seq)) if rc else seq
            recs.append([b"@edge%d_%d" % (k, rc), s.encode(), b"+", bytes(33 + (k + j) % 94 for j in range(L))])
    sam, E, R = _synthetic(lam, model, _fastq(recs), "edges", min_events=1000)
    st = {}
    ec.tables_of_sam(masks, ec.lambda_offsets(), sam, stats=st)
    assert st["masked"] >= 8
    ends = [int(f[3]) - 1 + EDGE + int(f[5][:-1]) for f in (l.split(b"\t") for l in sam.split(b"\n") if l) if f[2] == b"lambdaB_div2pct" and f[5].endswith(b"M") and f[5][:-1].isdigit()]
    assert REF_LEN in ends                                           # an M run ends at ref_len - 1


# ---- the `salt` binary on the GPU ----
SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("errprofidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


def _salt(args, **env):
    return subprocess.run([SALT] + args, capture_output=True, timeout=300, env=dict(os.environ, **env))


def _file_of(salt_amd, ix, model, sam, min_mapq=0, full=False):
    E, R, n = salt_amd.errprof_add_sam(ix, sam, min_mapq)
    mE, mR, _ = model(sam, min_mapq)
    assert n > 0 and np.array_equal(E, mE) and np.array_equal(R, mR)
    text = salt_amd.errprof_text(E, R, min_mapq, full)
    assert text == ec.text_of(mE, mR, min_mapq, full)
    return text


CLI_SETS = {"se": (["-d", "-c"], ["reads_se.fq"]), "pe": (["-d", "-p", "-c", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"])}
_cli_runs = {}


def _cli(case, prefix, extra=()):
    """one `salt` run of a case, made once and shared by the tests that read it"""
    key = (case, prefix) + tuple(extra)
    if key not in _cli_runs:
        args, files = CLI_SETS[case]
        _cli_runs[key] = _salt(args + list(extra) + [prefix] + [os.path.join(LAMBDA, f) for f in files])
        assert _cli_runs[key].returncode == 0, _cli_runs[key].stderr[-600:]
    return _cli_runs[key]


@pytest.mark.parametrize("case", ["se", "pe"])
def test_cli_file_equals_the_model_over_the_runs_sam(case, lam, model, lambda_cli_index, tmp_path_factory):
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    f = tmp_path_factory.getbasetemp() / ("errprof_%s.tsv" % case)
    off, run = _cli(case, lambda_cli_index), _cli(case, lambda_cli_index, ["--error-profile", str(f)])
    assert b"counted on the device" in run.stderr and run.stderr.count(b"[salt] error profile:") == 1 and b"error profile" not in off.stderr
    assert strip_pg(run.stdout) == strip_pg(off.stdout)
    assert f.read_bytes() == _file_of(salt_amd, ix, model, run.stdout) and b"\n#E\t" not in f.read_bytes()


@pytest.mark.parametrize("case", ["se", "pe"])
def test_cli_full_file_at_min_mapq_20(case, lam, model, lambda_cli_index, tmp_path):
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    ff = tmp_path / "e_full.tsv"
    full = _cli(case, lambda_cli_index, ["--error-profile", str(ff), "--error-profile-full", "--error-profile-min-mapq", "20"])
    assert strip_pg(full.stdout) == strip_pg(_cli(case, lambda_cli_index).stdout)
    assert ff.read_bytes() == _file_of(salt_amd, ix, model, full.stdout, 20, True)
    p = ec.parse_file(ff.read_bytes())
    assert p["min_mapq"] == 20 and p["E"].any()


@pytest.mark.parametrize("case", ["se", "pe"])
def test_cli_with_bam_output(case, lam, model, lambda_cli_index, tmp_path):
    from bam_check import decode_stream
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    fb = tmp_path / "e_bam.tsv"
    bam_off, bam = _cli(case, lambda_cli_index, ["--bam"]), _cli(case, lambda_cli_index, ["--bam", "--error-profile", str(fb)])
    (text, lines, _), (text0, lines0, _) = decode_stream(bam.stdout), decode_stream(bam_off.stdout)
    assert lines == lines0 and strip_pg(text) == strip_pg(text0)
    assert fb.read_bytes() == _file_of(salt_amd, ix, model, lines)


@pytest.mark.parametrize("case", ["se", "pe"])
def test_cli_under_polish_the_file_is_the_plain_runs(case, lam, model, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    fp = tmp_path / "e_polish.tsv"
    pol, alone = _cli(case, lambda_cli_index, ["--polish", "--error-profile", str(fp)]), _cli(case, lambda_cli_index, ["--polish"])
    assert pol.stdout == alone.stdout and len(alone.stdout) > 100000
    assert fp.read_bytes() == _file_of(salt_amd, ix, model, _cli(case, lambda_cli_index).stdout)      # the rows are counted, whatever is printed of them


def test_cli_blocked_gzip_input_takes_the_qualities_from_the_inflated_text(lam, model, lambda_cli_index, tmp_path):
    """salt_gpu_align_se_text_dev: the block is a range of the workspace's inflated text"""
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    fq = _fq("reads_se.fq")
    gz = tmp_path / "reads.fq.gz"
    gz.write_bytes(salt_amd.bgzf_deflate(fq) + salt_amd.BGZF_EOF)
    f = tmp_path / "e.tsv"
    run = _salt(["-d", "-c", "--error-profile", str(f), "--error-profile-full", lambda_cli_index, str(gz)], SALT_INFLATE_DEVICE="1")
    assert run.returncode == 0 and b"counted on the device" in run.stderr and b"[salt] BGZF input: device inflate, " in run.stderr, run.stderr[-600:]
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert f.read_bytes() == _file_of(salt_amd, ix, model, run.stdout, 0, True)
    assert len(ec.parse_file(f.read_bytes())["Q"]) == 21


def test_cli_counts_every_written_block_once_across_the_hand_over_and_on_the_host_pipeline(lam, model, lambda_cli_index, tmp_path):
    """A multi-line record in the middle of the file: the blocks behind the refused chunk are taken back (salt_gpu_ws_errprof_uncount) and
    the host pipeline, which hands its batches' qualities over with salt_gpu_ws_set_quals, aligns those reads again."""
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    recs = _records("reads_se.fq")
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq, f, fh = tmp_path / "mid_multiline.fq", tmp_path / "e.tsv", tmp_path / "e_host.tsv"
    fq.write_bytes(b"\n".join(out) + b"\n")
    run = _salt(["-d", "-c", "-t", "8", "--error-profile", str(f), "--error-profile-full", lambda_cli_index, str(fq)], SALT_CHUNK_BYTES="9000")
    assert run.returncode == 0, run.stderr[-600:]
    assert b"the host parser takes over" in run.stderr and b"counted on the device" in run.stderr
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    want = _file_of(salt_amd, ix, model, run.stdout, 0, True)
    assert f.read_bytes() == want
    host = _salt(["-d", "-c", "-t", "8", "--error-profile", str(fh), "--error-profile-full", lambda_cli_index, os.path.join(LAMBDA, "reads_se.fq")], SALT_HOST_PIPELINE="1")
    assert host.returncode == 0 and b"host phases" in host.stderr, host.stderr[-600:]
    assert fh.read_bytes() == want                                   # the file does not depend on which path read a record
