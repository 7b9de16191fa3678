"""The run's summary on the device: k_stats_add behind every entry point that leaves result rows against the host twin (salt_stats_add_sam)
over the SAM text the same call returned AND against the Python statement (tests/stats_check.py) -- single and paired end, text,
host-buffer and resident entry points, under polish --, the state of the tables (two calls, a fork, reset, off, uncount), small
synthetic batches at the shapes where the kernel takes another path, an index with more contigs than a workgroup holds in LDS, and
`salt --stats` end to end.

The listed calls together reach every table and every SN cell with a non-zero count: test_the_calls_cover_every_table_and_every_sn_cell
asserts it over the fixtures the other tests compare (tests/test_stats_host.py shows on the CPU that the goldens of the same inputs can)."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import gap_cases
import pe_geometry as pg
import stats_check as sc
from conftest import EXTRA_CASES, LAMBDA, ROOT

pytestmark = pytest.mark.gpu

EDGE, REF_LEN = 48502, 97004
PIECE = 16                                  # bytes of the loads k_stats_add takes a read's bases in

SE_SETS = {
    "se_default": (["-d", "-c"], ["reads_se.fq"]), "ragged_default": EXTRA_CASES["ragged_default"],
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


CONTIGS = sc.lambda_contigs()


def _narrow_aligner(salt_amd, ix, **kw):
    """a second device index beside the module's, with a narrow W-mer table (the default width takes 64 GiB)"""
    old = os.environ.get("SALT_GPU_LKT_LEN")
    os.environ["SALT_GPU_LKT_LEN"] = "12"
    try:
        return salt_amd.GpuAligner(ix, device=0, **kw)
    finally:
        if old is None:
            del os.environ["SALT_GPU_LKT_LEN"]
        else:
            os.environ["SALT_GPU_LKT_LEN"] = old


def _check(salt_amd, ix, got, sam, min_mapq=0, skipped=0, what="", contigs=CONTIGS):
    """the device's (cells, ct) = the twin over the SAM = the Python statement; a skipped read prints as an empty line, so only the device
    sees it (SN seen and skipped)"""
    cells, ct = got
    assert cells.dtype == np.uint64 and cells.shape == (sc.CELLS,) and ct.shape == (len(contigs), 8)
    t_cells, t_ct, _ = salt_amd.stats_add_sam(ix, sam, min_mapq)
    m_cells, m_ct, _ = sc.tables_of_sam(contigs, sam, min_mapq)
    assert np.array_equal(t_cells, m_cells) and np.array_equal(t_ct, m_ct), what
    cells = cells.copy()
    T, W = sc.split(cells), sc.split(t_cells)
    assert int(T["SN"][:, 1].sum()) == skipped, (what, T["SN"].tolist())
    T["SN"][:, 0] -= T["SN"][:, 1]
    T["SN"][:, 1] = 0
    for name in sc.TABLES:
        if not np.array_equal(T[name], W[name]):
            bad = np.argwhere(T[name] != W[name])
            raise AssertionError("%s: %s differs in %d cells; first %s: device %s, twin %s" %
                                 (what, name, len(bad), bad[:6].tolist(), [int(T[name][tuple(b)]) for b in bad[:6]], [int(W[name][tuple(b)]) for b in bad[:6]]))
    assert np.array_equal(ct, t_ct), (what, ct[(ct != t_ct).any(axis=1)][:4].tolist(), t_ct[(ct != t_ct).any(axis=1)][:4].tolist())
    assert not T["OR"][3] and not ct[:, 6:].any()
    return T, ct


def _text_call(aln, call, min_mapq=0):
    """the call's SAM and what it alone added to the tables"""
    aln.stats_enable(True, min_mapq)
    aln.stats_tables(reset=True)
    sam = call()
    got = aln.stats_tables()
    aln.stats_enable(False)
    return sam, got


def test_before_the_first_enable_the_errors_and_nothing_allocated(lam):
    salt_amd, ix, _ = lam
    other = _narrow_aligner(salt_amd, ix, max_reads=64)
    try:
        for call in (other.stats_tables, other.stats_uncount):
            with pytest.raises(salt_amd.SaltError, match="never enabled"):
                call()
        with pytest.raises(salt_amd.SaltError, match="set_contigs"):     # the per-contig counts need the table, and the message names it
            other.stats_enable(True, 0)
        with pytest.raises(salt_amd.SaltError, match="never enabled"):
            other.stats_tables()
        other.set_contigs(ix)
        with pytest.raises(salt_amd.SaltError, match="255"):
            other.stats_enable(True, 256)
        other.stats_enable(False)                                    # stopping what never ran is no error, and allocates nothing:
        with pytest.raises(salt_amd.SaltError, match="never enabled"):      # the tables are still not there
            other.stats_tables()
        other.stats_enable(True, 255)
        cells, ct = other.stats_tables()
        assert not cells.any() and not ct.any() and ct.shape == (2, 8)
        lib = salt_amd.gpu_lib()
        small = np.zeros(10, dtype=np.uint64)
        assert lib.salt_gpu_index_stats_fetch(other._ix, small.ctypes.data, small.size, None, 0, 0) == -1
        assert b"6021" in lib.salt_gpu_last_error() and b"10" in lib.salt_gpu_last_error()
        assert lib.salt_gpu_index_stats_fetch(other._ix, None, 0, small.ctypes.data, small.size, 0) == -1
        assert b"16" in lib.salt_gpu_last_error()
        assert lib.salt_gpu_index_stats_fetch(other._ix, None, 0, None, 0, 1) == 0      # reset only
    finally:
        other.close()


@pytest.fixture(scope="module")
def se_tabs(lam):
    """name -> {"sam", 0: (cells, ct), 20: (cells, ct)} of the single-end text call"""
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
def test_single_end_text_call(name, min_mapq, lam, se_tabs):
    salt_amd, ix, _ = lam
    T, ct = _check(salt_amd, ix, se_tabs[name][min_mapq], se_tabs[name]["sam"], min_mapq, what=name)
    assert int(T["SN"][0, 4]) > 0 and not T["SN"][1].any() and not T["IS"].any() and not T["OR"].any()


@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("name", sorted(PE_SETS))
def test_paired_end_text_call(name, min_mapq, lam, pe_tabs):
    salt_amd, ix, _ = lam
    T, ct = _check(salt_amd, ix, pe_tabs[name][min_mapq], pe_tabs[name]["sam"], min_mapq, what=name)
    assert int(T["SN"][0, 0]) == int(T["SN"][1, 0]) > 0 and T["IS"].any() and int(T["IS"].sum()) == int(T["SN"][0, 8])


# ---- the pairs of the designed fixture: TLEN at -a, -b and one outside each, every orientation, both contigs, and equal POS ----
def _genome():
    seqs, name = {}, None
    for line in open(os.path.join(LAMBDA, "genome.fa")).read().split("\n"):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        elif line:
            seqs[name].append(line.strip().upper())
    return "".join("".join(seqs[n]) for n in ("lambdaA", "lambdaB_div2pct"))


COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def _rc(s):
    return "".join(COMP[c] for c in reversed(s))


@pytest.fixture(scope="module")
def geom_tabs(lam):
    """row -> (sam, (cells, ct)) of the designed pairs under the row's window, with one pair added whose mates start at the same position"""
    salt_amd, ix, aln = lam
    g = _genome()
    same = g[20000:20100]
    fq1 = _fq(pg.READS[0] + ".gz") + ("@samepos\n%s\n+\n%s\n" % (same, "I" * 100)).encode()
    fq2 = _fq(pg.READS[1] + ".gz") + ("@samepos\n%s\n+\n%s\n" % (_rc(same), "I" * 100)).encode()
    out = {}
    for row, (args, lo, hi) in pg.ROWS.items():
        opt = _opt(salt_amd, ix, args)
        out[row] = _text_call(aln, lambda: aln.align_pe_text(opt, ix, fq1, fq2)[0])
    return out


@pytest.mark.parametrize("row", sorted(pg.ROWS))
def test_pairs_at_the_edges_of_the_window_every_orientation_and_equal_pos(row, lam, geom_tabs):
    salt_amd, ix, _ = lam
    sam, got = geom_tabs[row]
    T, ct = _check(salt_amd, ix, got, sam, what="geometry " + row)
    _, lo, hi = pg.ROWS[row]
    IS = T["IS"]
    assert IS[lo] and IS[lo + 1] and IS[hi - 1] and IS[hi] and not IS[:lo].any() and not IS[hi + 1:].any()      # printed TLEN is -a and -b, and nothing outside
    recs = {name: (a, b) for name, a, b in pg.records(sam)}
    table = pg.class_table()
    outside = [n for n, (a, b) in recs.items() if table.get(n, ("", 0))[1] in (lo - 1, hi + 1) and table[n][0].startswith("edge_" + row) and a[8] == "0" and not int(a[1]) & 2]
    assert len(outside) >= 4                                         # designed one outside each edge: no TLEN, no 0x2, no IS entry
    a, b = recs["samepos"]
    assert a[2] == b[2] == "lambdaA" and a[3] == b[3] == a[7] == "20001" and not (int(a[1]) | int(b[1])) & 12
    assert T["OR"][:3].all() and T["SN"][:, 9].any() and T["SN"][:, 10].any() and ct[:, :6].all()


# ---- the other entry points ----
def _read_set(salt_amd, files):
    if len(files) == 1:
        return salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
    return salt_amd.interleave_pairs(salt_amd.read_fastq(os.path.join(LAMBDA, files[0])), salt_amd.read_fastq(os.path.join(LAMBDA, files[1])))


@pytest.mark.parametrize("name", ["se_default", "gap_se_mid", "pe_default", "gap_pe_short"])
def test_host_buffer_calls_and_their_uncount(name, lam, se_tabs, pe_tabs):
    salt_amd, ix, aln = lam
    pe = name in PE_SETS
    args, files = (PE_SETS if pe else SE_SETS)[name]
    names, seqs, offs, quals = _read_set(salt_amd, files)
    opt = _opt(salt_amd, ix, args)
    call = (lambda: aln.alnpe_core1(opt, ix, seqs, offs)) if pe else (lambda: aln.alnse_core1(opt, seqs, offs))
    want = (pe_tabs if pe else se_tabs)[name]
    _, (cells, ct) = _text_call(aln, call, 20)
    assert np.array_equal(cells, want[20][0]) and np.array_equal(ct, want[20][1])
    aln.stats_enable(True, 20)
    aln.stats_tables(reset=True)
    call()
    aln.stats_uncount()
    cells, ct = aln.stats_tables()
    aln.stats_enable(False)
    assert not cells.any() and not ct.any()


def test_resident_entry_points_on_the_callers_stream(lam, se_tabs, pe_tabs):
    import torch
    salt_amd, ix, aln = lam
    isz = salt_amd.RESULT_DTYPE.itemsize
    st = torch.cuda.Stream()
    for name, sets, want in (("ragged_default", SE_SETS, se_tabs), ("ragged_pe", PE_SETS, pe_tabs)):
        args, files = sets[name]
        _, seqs, offs, _ = _read_set(salt_amd, files)
        n, max_len = len(offs) - 1, int(np.diff(offs).max())
        d_seqs = torch.from_numpy(np.concatenate([seqs, np.zeros(64, dtype=np.uint8)])).cuda()
        d_offs = torch.from_numpy(np.asarray(offs).astype(np.int32)).cuda()
        d_res = torch.zeros(n * isz, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        opt = _opt(salt_amd, ix, args)
        aln.stats_enable(True, 0)
        aln.stats_tables(reset=True)
        with torch.cuda.stream(st):
            if len(files) == 1:
                aln.align_resident(opt, n, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
            else:
                aln.align_pe_resident(opt, ix, n // 2, max_len, d_seqs.data_ptr(), d_offs.data_ptr(), d_res.data_ptr(), st.cuda_stream)
        cells, ct = aln.stats_tables()                               # (synchronises the device)
        aln.stats_enable(False)
        assert np.array_equal(cells, want[name][0][0]) and np.array_equal(ct, want[name][0][1])


def test_under_set_polish_the_tables_are_the_plain_calls(lam, se_tabs, pe_tabs):
    salt_amd, ix, aln = lam
    aln.set_pac(ix)
    aln.set_polish(1)
    try:
        opt = _opt(salt_amd, ix, SE_SETS["se_default"][0])
        _, (cells, ct) = _text_call(aln, lambda: aln.align_se_text(opt, _fq("reads_se.fq"))[0])
        assert np.array_equal(cells, se_tabs["se_default"][0][0]) and np.array_equal(ct, se_tabs["se_default"][0][1])
        args, files = PE_SETS["ragged_pe"]
        _, (cells, ct) = _text_call(aln, lambda: aln.align_pe_text(_opt(salt_amd, ix, args), ix, _fq(files[0]), _fq(files[1]))[0])
        assert np.array_equal(cells, pe_tabs["ragged_pe"][0][0]) and np.array_equal(ct, pe_tabs["ragged_pe"][0][1])
    finally:
        aln.set_polish(0)


def test_two_calls_add_a_fork_shares_the_tables_reset_off_and_uncount(lam, se_tabs, pe_tabs):
    salt_amd, ix, aln = lam
    opt_se, opt_pe = _opt(salt_amd, ix, SE_SETS["se_default"][0]), _opt(salt_amd, ix, PE_SETS["ragged_pe"][0])
    fq, fq1, fq2 = _fq("reads_se.fq"), _fq("reads_ragged_pe_1.fq"), _fq("reads_ragged_pe_2.fq")
    (c1, t1), (c2, t2) = se_tabs["se_default"][0], pe_tabs["ragged_pe"][0]
    same = lambda got, cells, ct: np.array_equal(got[0], cells) and np.array_equal(got[1], ct)
    aln.stats_enable(True, 0)
    aln.stats_tables(reset=True)
    sam_on, _ = aln.align_se_text(opt_se, fq)
    aln.align_se_text(opt_se, fq)
    assert same(aln.stats_tables(), 2 * c1, 2 * t1)
    fork = aln.fork()
    try:
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        for a in (aln, fork):
            assert same(a.stats_tables(), 2 * c1 + c2, 2 * t1 + t2)
        cells, ct = fork.stats_tables(reset=True)
        assert cells.any() and same(aln.stats_tables(), 0 * c1, 0 * t1)
        # off: nothing is counted
        aln.stats_enable(False)
        sam_off, _ = aln.align_se_text(opt_se, fq)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        assert same(aln.stats_tables(), 0 * c1, 0 * t1)
        assert sam_on == sam_off == se_tabs["se_default"]["sam"]    # the SAM bytes do not depend on the tally
        # a block that is aligned and then dropped leaves the tables cell for cell as they were
        aln.stats_enable(True, 0)
        fork.align_pe_text(opt_pe, ix, fq1, fq2)
        aln.align_se_text(opt_se, fq)
        fork.stats_uncount()
        assert same(aln.stats_tables(), c1, t1)
        fork.stats_uncount()                                         # only once
        assert same(aln.stats_tables(), c1, t1)
        aln.stats_uncount()
        assert same(aln.stats_tables(), 0 * c1, 0 * t1)
    finally:
        aln.stats_enable(False)
        fork.close()


# ---- shapes where the kernel can go wrong: small synthetic batches, each against the twin and the model over the call's own SAM ----
def _records(name):
    lines = _fq(name).split(b"\n")
    return [lines[i:i + 4] for i in range(0, len(lines) - 3, 4)]


def _fastq(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def _synthetic(lam, fq, what, skipped=0, opt_args=("-d", "-c")):
    salt_amd, ix, aln = lam
    opt = _opt(salt_amd, ix, opt_args)
    sam, got = _text_call(aln, lambda: aln.align_se_text(opt, fq)[0])
    T, ct = _check(salt_amd, ix, got, sam, skipped=skipped, what=what)
    return sam, T, ct


def test_the_chunk_is_the_kernels():
    import salt_amd
    src = open(os.path.join(ROOT, "salt_amd", "csrc", "salt_kernels.h")).read()
    assert "SALT_STATS_CHUNK = %d;" % salt_amd.STATS_CHUNK in src
    hdr = open(os.path.join(ROOT, "include", "salt_gpu.h")).read()
    assert "#define SALT_STATS_CT_LDS   %du" % salt_amd.STATS_CT_LDS in hdr and "#define SALT_STATS_CELLS    %du" % sc.CELLS in hdr


def _sizes():
    import salt_amd
    c = salt_amd.STATS_CHUNK
    return [1, 63, 64, 65, c - 1, c, c + 1, 2 * c + 3]


@pytest.mark.parametrize("n", _sizes())
def test_single_end_batch_sizes_around_a_wave_and_a_workgroups_chunk(n, lam):
    recs = _records("reads_se.fq")
    _, T, _ = _synthetic(lam, _fastq([recs[i % len(recs)] for i in range(n)]), "%d records" % n)
    assert int(T["SN"][0, 0]) == n and int(T["RL"][0].sum()) == n


@pytest.mark.parametrize("n", [1, _sizes()[5] // 2 - 1, _sizes()[5] // 2, _sizes()[5] // 2 + 1])
def test_paired_end_batch_sizes_around_a_workgroups_chunk(n, lam):
    salt_amd, ix, aln = lam
    r1, r2 = _records("reads_pe_1.fq"), _records("reads_pe_2.fq")
    fq1, fq2 = _fastq([r1[i % len(r1)] for i in range(n)]), _fastq([r2[i % len(r2)] for i in range(n)])
    opt = _opt(salt_amd, ix, PE_SETS["pe_default"][0])
    sam, got = _text_call(aln, lambda: aln.align_pe_text(opt, ix, fq1, fq2)[0])
    T, _ = _check(salt_amd, ix, got, sam, what="%d pairs" % n)
    assert int(T["SN"][0, 0]) == int(T["SN"][1, 0]) == n and int(T["SN"][0, 4]) > 0 and int(T["SN"][1, 4]) > 0


def test_no_records(lam):
    salt_amd, ix, aln = lam
    opt = _opt(salt_amd, ix, ["-d", "-c"])
    sam, (cells, ct) = _text_call(aln, lambda: aln.align_se_text(opt, b"")[0])
    assert sam == b"" and not cells.any() and not ct.any()
    aln.stats_enable(True, 0)
    aln.stats_uncount()                                              # nothing to take back
    aln.stats_enable(False)


def test_2048_copies_of_one_read_fall_on_one_cell_of_every_table(lam):
    r = [x for x in _records("reads_se.fq")][0]
    sam, T, ct = _synthetic(lam, _fastq([[b"@c%d" % k] + r[1:] for k in range(2048)]), "2048 copies")
    assert int(T["SN"][0, 4]) == 2048
    for name in ("MQ", "RL", "GC", "XA"):
        assert len(np.flatnonzero(T[name])) == 1 and int(T[name].max()) == 2048, name
    assert int(ct[:, 2].max()) == 2048 and int(ct[:, 5].sum()) == int(T["SN"][0, 12]) >= 2048 * 80


def test_2048_copies_of_one_pair(lam):
    salt_amd, ix, aln = lam
    a, b = _records("reads_pe_1.fq")[0], _records("reads_pe_2.fq")[0]
    fq1, fq2 = _fastq([[b"@c%d" % k] + a[1:] for k in range(2048)]), _fastq([[b"@c%d" % k] + b[1:] for k in range(2048)])
    opt = _opt(salt_amd, ix, PE_SETS["pe_default"][0])
    sam, got = _text_call(aln, lambda: aln.align_pe_text(opt, ix, fq1, fq2)[0])
    T, _ = _check(salt_amd, ix, got, sam, what="2048 copies of a pair")
    assert int(T["SN"][0, 8]) == int(T["SN"][1, 8]) == 2048 and int(T["IS"].max()) == 2048 and int(T["OR"].max()) == 2048


@pytest.mark.parametrize("strand", [0, 16])
def test_all_forward_and_all_reverse_batches(strand, lam, se_tabs):
    recs, k, keep = _records("reads_se.fq"), 0, []
    for line in se_tabs["se_default"]["sam"].split(b"\n"):
        if line and not line.startswith(b"@"):
            f = line.split(b"\t")
            if not int(f[1]) & 4 and int(f[1]) & 16 == strand:
                keep.append(recs[k])
            k += 1
    sam, T, ct = _synthetic(lam, _fastq(keep), "strand %d" % strand)
    assert int(T["SN"][0, 5]) == (int(T["SN"][0, 4]) if strand else 0) and int(T["SN"][0, 4]) >= 800 and int(ct[:, 4].sum()) == int(T["SN"][0, 5])


LENGTHS = [1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE - 1, 2 * PIECE, 2 * PIECE + 1, 120, 121, 511, 512, 100, 33]


@pytest.fixture(scope="module")
def lengths_tab(lam):
    """(sam, (cells, ct)) of one batch of reads of every length around a piece, reads with N, a read of all N and a skipped read"""
    salt_amd, ix, aln = lam
    g = _genome()
    recs = []
    for k, L in enumerate(LENGTHS):
        seq = g[3000 + 700 * k:3000 + 700 * k + L].replace("N", "A")
        recs.append([b"@len%d_%d" % (L, k), seq.encode(), b"+", b"I" * L])
    for k in range(40):                                              # reads with N, at every offset of a piece
        s = bytearray(g[30000 + 150 * k:30000 + 150 * k + 100].encode())
        for j in (k % 100, (7 * k + 3) % 100, 99 - k % 16):
            s[j] = ord("N")
        recs.append([b"@n%d" % k, bytes(s), b"+", b"I" * 100])
    recs.append([b"@all_n", b"N" * 40, b"+", b"I" * 40])
    recs.append([b"@skipped", (g[60000:60050] + "N" * 250).encode(), b"+", b"I" * 300])      # more than 200 N: the aligner leaves it untouched
    opt = _opt(salt_amd, ix, ["-d", "-c"])
    return _text_call(aln, lambda: aln.align_se_text(opt, _fastq(recs))[0])


def test_read_lengths_around_a_16_byte_piece_reads_with_n_all_n_and_a_skipped_read(lam, lengths_tab):
    salt_amd, ix, _ = lam
    sam, got = lengths_tab
    T, ct = _check(salt_amd, ix, got, sam, skipped=1, what="lengths and N")
    assert int(sc.split(got[0])["SN"][0, 1]) == 1 and int(sc.split(got[0])["SN"][0, 0]) == len(LENGTHS) + 42
    assert all(T["RL"][0, L] for L in LENGTHS + [40]) and not T["RL"][0, 300]      # the skipped read is in SN 0 and 1 only
    assert int(T["GC"][0, 101]) == 1 and int(T["SN"][0, 11]) == sum(LENGTHS) + 40 * 100 + 40 and int(T["SN"][0, 4]) >= 30
    assert sam.count(b"\n\n") >= 1


def test_a_read_that_ends_at_the_genomes_last_position(lam):
    g = _genome()
    recs = []
    for k, (a, L) in enumerate([(REF_LEN - 100, 100), (REF_LEN - 37, 37), (EDGE - 100, 100), (0, 100), (EDGE, 64)]):
        seq = g[a:a + L].replace("N", "A")
        for rc in (False, True):
            recs.append([b"@edge%d_%d" % (k, rc), (_rc(seq) if rc else seq).encode(), b"+", b"I" * L])
    sam, T, ct = _synthetic(lam, _fastq(recs), "edges")
    ends = [int(f[3]) - 1 + EDGE + int(f[5][:-1]) for f in (l.split(b"\t") for l in sam.split(b"\n") if l) if f[2] == b"lambdaB_div2pct" and f[5].endswith(b"M") and f[5][:-1].isdigit()]
    assert REF_LEN in ends and int(T["SN"][0, 12]) == int(ct[:, 5].sum()) >= 600      # an M run ends at ref_len - 1


# ---- more contigs than a workgroup holds in LDS ----
@pytest.fixture(scope="module")
def many_contigs(tmp_path_factory):
    """An index of SALT_STATS_CT_LDS + 3 contigs of 300 bases, made by the project's host index builder (one SNP: the builder wants one)."""
    import salt_amd
    d = tmp_path_factory.mktemp("statsctg")
    rng = random.Random(5)
    seqs = ["".join(rng.choice("ACGT") for _ in range(300)) for _ in range(salt_amd.STATS_CT_LDS + 3)]
    (d / "g.fa").write_text("".join(">ctg%03d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    ref = seqs[0][49]
    (d / "s.txt").write_text("ctg000\t50\t%s/%s\t%s\n" % (tuple(sorted([ref, "C" if ref != "C" else "G"])) + (ref,)))
    prefix = str(d / "idx")
    salt_amd.idx_build(str(d / "g.fa"), str(d / "s.txt"), prefix, 19, flags=salt_amd.IDX_NO_LP)
    ix = salt_amd.Index.reload(prefix)
    aln = _narrow_aligner(salt_amd, ix, max_reads=4096, max_bases=4096 * 160)
    aln.set_contigs(ix)
    yield salt_amd, ix, aln, seqs, sc.contigs_of_ann(prefix + ".C.ann")
    aln.close()
    ix.destroy()


def test_contigs_held_in_lds_and_contigs_counted_in_global_memory(many_contigs):
    salt_amd, ix, aln, seqs, contigs = many_contigs
    lds = salt_amd.STATS_CT_LDS
    assert len(contigs) == lds + 3 and contigs[-1][1] + contigs[-1][2] == 300 * (lds + 3)
    recs = []
    for c, n in ((0, 5), (lds - 1, 7), (lds, 11), (lds + 2, 3), (17, 2)):
        for k in range(n):
            s = seqs[c][10 * k:10 * k + 100] if k % 2 == 0 else _rc(seqs[c][10 * k:10 * k + 100])
            recs.append([b"@c%d_%d" % (c, k), s.encode(), b"+", b"I" * 100])
    recs.append([b"@last", seqs[-1][200:].encode(), b"+", b"I" * 100])  # ends at the genome's last position
    fq = _fastq(recs * 80)                                           # 2 320 records: more than a workgroup's chunk
    opt = _opt(salt_amd, ix, ["-d", "-c"])
    sam, got = _text_call(aln, lambda: aln.align_se_text(opt, fq)[0])
    T, ct = _check(salt_amd, ix, got, sam, what="many contigs", contigs=contigs)
    assert ct[0, 2] >= 80 * 5 and ct[lds - 1, 2] >= 80 * 7 and ct[lds, 2] >= 80 * 11 and ct[lds + 2, 2] >= 80 * 4 and ct[17, 2] >= 80 * 2
    assert int(ct[:, 5].sum()) == int(T["SN"][0, 12]) and int(ct[:, 4].sum()) == int(T["SN"][0, 5]) > 0
    # the adds that went to global memory directly are taken back like the others, and at a floor they are mapped and not counted
    aln.stats_enable(True, 255)
    aln.stats_tables(reset=True)
    aln.align_se_text(opt, fq)
    cells, ct255 = aln.stats_tables()
    assert np.array_equal(ct255[:, 0], ct[:, 0]) and not ct255[:, 2:].any() and ct255[lds, 0] > 0
    aln.stats_uncount()
    cells, ct0 = aln.stats_tables()
    aln.stats_enable(False)
    assert not cells.any() and not ct0.any()


def test_the_calls_cover_every_table_and_every_sn_cell(se_tabs, pe_tabs, geom_tabs, lengths_tab):
    """None of the comparisons above passes on empty ground: together the calls reach every table and all 16 cells of SN."""
    cells = np.zeros(sc.CELLS, dtype=np.uint64)
    ct = np.zeros((2, 8), dtype=np.uint64)
    for got in [t[q] for tabs in (se_tabs, pe_tabs) for t in tabs.values() for q in (0, 20)] + [g[1] for g in geom_tabs.values()] + [lengths_tab[1]]:
        cells += got[0]
        ct += got[1]
    T = sc.split(cells)
    assert all(T[name].any() for name in sc.TABLES) and ct[:, :6].all()
    assert T["SN"].sum(axis=0).all(), T["SN"].tolist()
    assert T["OR"][:3].all() and T["ID"].any(axis=1).all() and T["XA"][:, 1:].any() and T["IS"][1:4096].any() and T["GC"][:, 101].any()


# ---- the `salt` binary on the GPU ----
SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("statsidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    return prefix


def _salt(args, **env):
    return subprocess.run([SALT] + args, capture_output=True, timeout=300, env=dict(os.environ, **env))


def _file_of(salt_amd, ix, sam, min_mapq=0):
    cells, ct, n = salt_amd.stats_add_sam(ix, sam, min_mapq)
    m_cells, m_ct, _ = sc.tables_of_sam(CONTIGS, sam, min_mapq)
    assert n > 0 and np.array_equal(cells, m_cells) and np.array_equal(ct, m_ct)
    text = salt_amd.stats_text(ix, cells, ct, min_mapq)
    assert text == sc.text_of(CONTIGS, m_cells, m_ct, min_mapq)
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
def test_cli_file_equals_the_model_over_the_runs_sam(case, lam, lambda_cli_index, tmp_path_factory):
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    f = tmp_path_factory.getbasetemp() / ("stats_%s.tsv" % case)
    q = 20 if case == "pe" else 0
    off, run = _cli(case, lambda_cli_index), _cli(case, lambda_cli_index, ["--stats", str(f)] + (["--stats-min-mapq", "20"] if q else []))
    assert b"counted on the device" in run.stderr and run.stderr.count(b"[salt] stats:") == 1 and b"[salt] stats:" not in off.stderr
    assert strip_pg(run.stdout) == strip_pg(off.stdout)
    assert f.read_bytes() == _file_of(salt_amd, ix, run.stdout, q)
    assert sc.parse_file(f.read_bytes())["min_mapq"] == q


@pytest.mark.parametrize("case", ["se", "pe"])
def test_cli_with_bam_output(case, lam, lambda_cli_index, tmp_path):
    from bam_check import decode_stream
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    fb = tmp_path / "s_bam.tsv"
    bam_off, bam = _cli(case, lambda_cli_index, ["--bam"]), _cli(case, lambda_cli_index, ["--bam", "--stats", str(fb)])
    (text, lines, _), (text0, lines0, _) = decode_stream(bam.stdout), decode_stream(bam_off.stdout)
    assert lines == lines0 and strip_pg(text) == strip_pg(text0)
    assert fb.read_bytes() == _file_of(salt_amd, ix, lines)


@pytest.mark.parametrize("case", ["se", "pe"])
def test_cli_under_polish_the_file_is_the_plain_runs(case, lam, lambda_cli_index, tmp_path):
    salt_amd, ix, _ = lam
    fp = tmp_path / "s_polish.tsv"
    pol, alone = _cli(case, lambda_cli_index, ["--polish", "--stats", str(fp)]), _cli(case, lambda_cli_index, ["--polish"])
    assert pol.stdout == alone.stdout and len(alone.stdout) > 100000
    assert fp.read_bytes() == _file_of(salt_amd, ix, _cli(case, lambda_cli_index).stdout)      # the rows are counted, whatever is printed of them


def test_cli_blocked_gzip_input(lam, lambda_cli_index, tmp_path):
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    gz = tmp_path / "reads.fq.gz"
    gz.write_bytes(salt_amd.bgzf_deflate(_fq("reads_se.fq")) + salt_amd.BGZF_EOF)
    f = tmp_path / "s.tsv"
    run = _salt(["-d", "-c", "--stats", str(f), lambda_cli_index, str(gz)], SALT_INFLATE_DEVICE="1")
    assert run.returncode == 0 and b"counted on the device" in run.stderr and b"[salt] BGZF input: device inflate, " in run.stderr, run.stderr[-600:]
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    assert f.read_bytes() == _file_of(salt_amd, ix, run.stdout)


def test_cli_counts_every_written_block_once_across_the_hand_over_and_on_the_host_pipeline(lam, lambda_cli_index, tmp_path):
    """A multi-line record in the middle of the file: the blocks behind the refused chunk are taken back (salt_gpu_ws_stats_uncount) and
    the host pipeline aligns those reads again."""
    from bgzf_check import strip_pg
    salt_amd, ix, _ = lam
    recs = _records("reads_se.fq")
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq, f, fh = tmp_path / "mid_multiline.fq", tmp_path / "s.tsv", tmp_path / "s_host.tsv"
    fq.write_bytes(b"\n".join(out) + b"\n")
    run = _salt(["-d", "-c", "-t", "8", "--stats", str(f), lambda_cli_index, str(fq)], SALT_CHUNK_BYTES="9000")
    assert run.returncode == 0, run.stderr[-600:]
    assert b"the host parser takes over" in run.stderr and b"counted on the device" in run.stderr
    assert strip_pg(run.stdout) == open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read()
    want = _file_of(salt_amd, ix, run.stdout)
    assert f.read_bytes() == want
    host = _salt(["-d", "-c", "-t", "8", "--stats", str(fh), lambda_cli_index, os.path.join(LAMBDA, "reads_se.fq")], SALT_HOST_PIPELINE="1")
    assert host.returncode == 0 and b"host phases" in host.stderr, host.stderr[-600:]
    assert fh.read_bytes() == want                                   # the file does not depend on which path read a record
