"""Pins the CPU oracle (oracle/salt_oracle.c) against the reference's own outputs.

* tests/golden/lambda/expect_se_*.sam were printed by the real reference (`oracle/_ref/salt`,
  compiled in place from /root/reference by oracle/Makefile) -- see tests/golden/make_fixtures.py.
* tests/golden/lv_vectors.txt was printed by oracle/ref_harness.c linked against the reference's
  LandauVishkin.c / editdistance.c; tests/golden/lv_vectors_shapes.txt.gz by its --shapes mode.
* tests/golden/lambda/expect_gap_*.sam.gz: the reference on reads that all take the gapped pass (make_gap_fixture.py).
Bar: byte-identical SAM, exact integers / CIGAR strings.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gap_cases
from conftest import EXTRA_CASES, LAMBDA, GOLDEN, read_cases

SE_CASES = [c for c in read_cases() if c.startswith("se_")]


@pytest.mark.parametrize("case", SE_CASES)
def test_oracle_sam_matches_reference(case, oracle_cli, tmp_path):
    args = read_cases()[case]
    out = subprocess.run([oracle_cli] + args + [os.path.join(LAMBDA, "idx"), os.path.join(LAMBDA, "reads_se.fq")],
                         check=True, capture_output=True).stdout
    want = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    assert out == want


@pytest.mark.parametrize("case", sorted(EXTRA_CASES))
def test_oracle_sam_matches_reference_on_boundary_and_ragged_reads(case, oracle_cli):
    """The reference's own SAM for reads straddling the contig boundary / hanging over the genome's ends
    (make_span_fixture.py) and for mixed read lengths 19..300 bp, SE and PE (make_ragged_fixture.py)."""
    args, files = EXTRA_CASES[case]
    out = subprocess.run([oracle_cli] + args + [os.path.join(LAMBDA, "idx")] + [os.path.join(LAMBDA, f) for f in files],
                         check=True, capture_output=True).stdout
    assert out == open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()


def test_oracle_threads_do_not_change_output(oracle_cli):
    base = [os.path.join(LAMBDA, "idx"), os.path.join(LAMBDA, "reads_se.fq")]
    a = subprocess.run([oracle_cli, "-d", "-c"] + base, check=True, capture_output=True).stdout
    b = subprocess.run([oracle_cli, "-d", "-c", "-t", "4"] + base, check=True, capture_output=True).stdout
    assert a == b


def test_oracle_units_match_reference_vectors(oracle_lib):
    lib = oracle_lib
    ref = None
    n = 0
    with open(os.path.join(GOLDEN, "lv_vectors.txt")) as f:
        for line in f:
            t = line.split()
            if t[0] == "R":
                l_ref = int(t[1])
                ref = np.array([int(x, 16) for x in t[2:]] + [0] * 8, dtype=np.uint32)
                rp = ref.ctypes.data_as(ctypes.c_void_p)
                continue
            pos, L, kmis, kdiff = map(int, t[1:5])
            seq = np.ascontiguousarray(np.frombuffer(t[5].encode(), dtype=np.uint8) - 48)
            sp = seq.ctypes.data_as(ctypes.c_void_p)
            mis, diff, cret, cig = int(t[6]), int(t[7]), int(t[8]), t[9]
            assert lib.so_ed_mismatch(rp, pos, sp, L, kmis) == mis
            assert lib.so_ed_diff(rp, l_ref, pos, L + 4, sp, L, kdiff) == diff
            if 0 <= diff < 31:
                buf = ctypes.create_string_buffer(160)
                assert lib.so_ed_diff_cigar(rp, pos, L + 4, sp, L, diff, buf, 128) == cret
                assert (buf.value.decode() or "-") == cig
            n += 1
    assert n == 4000


@pytest.mark.parametrize("case", sorted(gap_cases.GAP_CASES))
def test_oracle_sam_matches_reference_on_the_gap_fixture(case, oracle_cli, tmp_path):
    """The reference's own SAM for reads built to have no gap-free hit (make_gap_fixture.py): 40..512 bases, indels of 1..L/10+1 bases at
    both sides of the 8-base words of the Landau-Vishkin windows, windows that end at the genome's end, indel mates of 100..250 bases.
    The golden files keep the gapped records they are for: gap_cases.MINIMA per file, 40 per read length."""
    args, _ = gap_cases.GAP_CASES[case]
    want = gap_cases.golden(case)
    n, n_gap, n_xa, by_len = gap_cases.census(want)
    assert all(have >= need for have, need in zip((n, n_gap, n_xa), gap_cases.MINIMA[case])), (n, n_gap, n_xa)
    assert min(by_len.values()) >= gap_cases.MIN_GAPPED_PER_LENGTH, by_len
    out = subprocess.run([oracle_cli] + args + [os.path.join(LAMBDA, "idx")] + gap_cases.plain_paths(case, tmp_path), check=True,
                         capture_output=True).stdout
    assert out == want, gap_cases.diff_message(out, want)


def test_oracle_units_match_reference_shape_vectors(oracle_lib):
    """ed_mismatch / ed_diff / ed_diff_withcigar on the shape vectors (ref_harness.c --shapes): lengths 19..512, bounds {L/10, 3, 12, 13,
    30}, indel runs up to 30 bases, windows at the reference's end.  The file keeps what the GPU unit test needs of it."""
    lib = oracle_lib
    l_ref, ref, vecs = gap_cases.load_lv_vectors(os.path.join(GOLDEN, "lv_vectors_shapes.txt.gz"))
    assert len(vecs) == 3000
    refp = np.concatenate([ref, np.zeros(8, dtype=np.uint32)])
    rp = refp.ctypes.data_as(ctypes.c_void_p)
    for i, v in enumerate(vecs):
        seq = np.ascontiguousarray(v.seq)
        sp = seq.ctypes.data_as(ctypes.c_void_p)
        L = len(seq)
        if v.mis != -9:
            assert lib.so_ed_mismatch(rp, v.pos, sp, L, v.kmis) == v.mis, i
        assert lib.so_ed_diff(rp, l_ref, v.pos, L + 4, sp, L, v.kdiff) == v.diff, i
        if 0 <= v.diff < 31:
            buf = ctypes.create_string_buffer(512)
            assert lib.so_ed_diff_cigar(rp, v.pos, L + 4, sp, L, v.diff, buf, 400) == v.cret, i
            assert (buf.value.decode() or "-") == v.cigar, i
    gap_cases.check_lv_vector_census(l_ref, vecs)


PE_CASES = [c for c in read_cases() if c.startswith("pe_")]


@pytest.mark.parametrize("case", PE_CASES)
def test_oracle_pe_sam_matches_reference(case, oracle_cli):
    """Paired end: pairing2 / pairing_singleton / SSW mate rescue (emulated lane by lane) / alnpe_sam against the
    SAM the real reference printed.  (The reference's PE locate calls rand() when an R interval exceeds max_locate;
    this fixture has none, so its output is deterministic.)"""
    args = read_cases()[case]
    out = subprocess.run([oracle_cli] + args + [os.path.join(LAMBDA, "idx"), os.path.join(LAMBDA, "reads_pe_1.fq"),
                                                os.path.join(LAMBDA, "reads_pe_2.fq")], check=True, capture_output=True).stdout
    want = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    assert out == want


def _ssw_vectors():
    out = []
    with open(os.path.join(GOLDEN, "ssw_vectors.txt")) as f:
        for line in f:
            t = line.split()
            out.append((int(t[1]), np.array([int(c, 16) for c in t[2]], dtype=np.uint8),
                        np.frombuffer(t[3].encode(), dtype=np.uint8) - 48, [int(x) for x in t[4:10]], t[10]))
    return out


def test_oracle_ssw_matches_reference_vectors(oracle_lib):
    """SSW 0.1.4 word kernel (forward, reverse, second best, banded traceback) emulated lane by lane, against answers
    printed by the reference's own ssw.c (oracle/ref_harness_ssw.c) for both score matrices."""
    lib = oracle_lib
    n = 0
    for aware, ref, codes, want6, cig in _ssw_vectors():
        out6 = (ctypes.c_int * 6)()
        buf = ctypes.create_string_buffer(512)
        codes = np.ascontiguousarray(codes)
        lib.so_ssw_unit(aware, ref.ctypes.data_as(ctypes.c_void_p), len(ref), codes.ctypes.data_as(ctypes.c_void_p), len(codes), out6, buf, 512)
        assert list(out6) == want6, (n, list(out6), want6)
        assert (buf.value.decode() or "-") == cig, (n, buf.value, cig)
        n += 1
    assert n == 600


def test_oracle_ssw_matches_reference_shape_sweep(oracle_lib):
    """The same restatement against ssw.c's answers for the shape sweep (oracle/ref_harness_ssw.c --shapes: reads of 16-512 bases,
    windows up to ~3000 columns, indel runs up to 60 bases, copies of the target around the second-best mask, CIGARs beyond 64
    operations).  With the half-width at which the band doubling stopped, each vector is classed by the k_swtb pass its traceback
    reads in the GPU launch of its length class (tests/ssw_sweep.py); every class keeps a minimum count, so no fixture edit can drop
    a code path of the GPU tests unnoticed."""
    import collections
    import re
    import ssw_sweep
    lib = oracle_lib
    vecs = ssw_sweep.load()
    assert len(vecs) == 1000
    band = []
    for n, v in enumerate(vecs):
        out6 = (ctypes.c_int * 6)()
        buf = ctypes.create_string_buffer(4096)
        bw = ctypes.c_int(0)
        codes = np.ascontiguousarray(v.codes)
        lib.so_ssw_unit_band(v.aware, v.ref.ctypes.data_as(ctypes.c_void_p), len(v.ref), codes.ctypes.data_as(ctypes.c_void_p), len(codes),
                             out6, buf, 4096, ctypes.byref(bw))
        assert list(out6) == v.want6, (n, list(out6), v.want6)
        assert (buf.value.decode() or "-") == v.cigar, (n, buf.value, v.cigar)
        band.append(bw.value)
    total = collections.Counter()
    for edge, order in ssw_sweep.launches(vecs):
        max_len = ssw_sweep.launch_max_len(vecs, order)
        c = collections.Counter()
        for i in order:
            v = vecs[i]
            c[ssw_sweep.tb_pass(v, band[i], max_len)] += 1
            rfl, rdl = v.want6[3] - v.want6[2] + 1, v.want6[5] - v.want6[4] + 1
            if band[i] > abs(rfl - rdl) + 1:
                c["doubled"] += 1
            if v.n_ops > ssw_sweep.MAX_CIGAR_OPS:
                c["over_ops"] += 1
        for k in ("reg", "lds", "rows_lds", "global", "doubled"):
            assert c[k] >= 5, (edge, k, dict(c))
        assert c["over"] == 0 and c[None] == 0, (edge, dict(c))          # no band beyond SW_BAND_W; every vector has a traceback
        total.update(c)
    want = {"reg": 400, "lds": 50, "rows_lds": 50, "dir_lds": 10, "global": 100, "doubled": 80, "over_ops": 8}
    assert all(total[k] >= m for k, m in want.items()), dict(total)
    # the other shapes the sweep is for
    lens = collections.Counter(len(v.codes) for v in vecs)
    assert all(lens[L] >= 10 for L in (104, 105, 152, 153, 256, 257, 512)), lens
    assert sum(lens[L] for L in range(16, 30)) >= 20                                  # maskLen < 15: no second best
    assert sum(1 for v in vecs if len(v.codes) in (30, 31) and v.want6[1] > 0) >= 5    # maskLen == 15: second best
    assert max(len(v.ref) for v in vecs) >= 2500 and sum(len(v.ref) < len(v.codes) for v in vecs) >= 20
    assert sum(v.want6[0] == v.want6[1] and v.want6[0] >= 50 for v in vecs) >= 10     # ties at real alignment scores
    gap = [max([int(x) for x in re.findall(r"(\d+)[ID]", v.cigar)] or [0]) for v in vecs]
    assert sum(g >= 30 for g in gap) >= 10
    assert sum((v.codes == 4).sum() >= 5 for v in vecs) >= 20
    assert sum(v.aware and (v.ref == 0).sum() >= 5 for v in vecs) >= 20
