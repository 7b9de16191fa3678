"""GPU parity tests proper: everything goes through the C ABI (libsalt_gpu.so) and is compared with
(a) the committed golden SAM the real reference printed and (b) the CPU oracle on seeded inputs."""
import os
import subprocess

import numpy as np
import pytest

from conftest import EXTRA_CASES, LAMBDA, read_cases

pytestmark = pytest.mark.gpu

SE_CASES = [c for c in read_cases() if c.startswith("se_")]
# The many-row CLI tests (option / tandem / seed-length / SNP-density matrices) compare semantics, not table widths: their `salt`
# processes use a 4 GiB W-mer table (W = 14) instead of tabulating 64 GiB each; the golden-fixture tests run at the default.
MATRIX_ENV = dict(os.environ, SALT_GPU_LKT_LEN=os.environ.get("SALT_GPU_LKT_LEN", "14"))


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=4096)
    reads = salt_amd.read_fastq(os.path.join(LAMBDA, "reads_se.fq"))
    yield salt_amd, idx, aln, reads
    aln.close()
    idx.destroy()


@pytest.mark.parametrize("case", SE_CASES)
def test_gpu_sam_matches_reference_golden(case, lam):
    salt_amd, idx, aln, (names, seqs, offs, quals) = lam
    opt, _ = salt_amd.AlnOpt.from_argv(read_cases()[case], idx.l_seed)
    res = aln.alnse_core1(opt, seqs, offs)
    got = salt_amd.sam_text(idx, opt, names, seqs, offs, quals, res)
    want = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    if got != want:
        g, w = got.split(b"\n"), want.split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        msg = "\n".join("line %d\n  got  %r\n  want %r" % (i, g[i][:400], w[i][:400]) for i in bad[:5])
        pytest.fail("%d differing lines (of %d)\n%s" % (len(bad), len(w), msg))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """Seeded synthetic genome with a repeat family (salt_amd/workload.py), indexed by the product's builder."""
    import salt_amd
    from salt_amd import workload
    cache = str(tmp_path_factory.mktemp("wl"))
    w = workload.prepare("tiny", cache)
    seqs, offs, _, _ = workload.make_reads(w["genome"], w["snp_pos"], w["snp_mask"], w["n_reads"], w["read_len"], seed=7)
    return w, seqs, offs


@pytest.mark.parametrize("optargs", [[], ["-r", "3", "-m", "64"], ["-s", "2", "-m", "200"], ["-v"]])
def test_gpu_fields_match_oracle_on_synthetic_repeats(tiny, optargs):
    """Every result field (pos, strand, n_diff, is_gap, mapq, b0/b1, alt hits, CIGAR) against the CPU oracle on
    4000 reads from a repeat-bearing genome; covers k_light, the k_heavy queue and the max_locate cap."""
    import sys
    import salt_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_py
    w, seqs, offs = tiny
    idx = salt_amd.Index.reload(w["prefix"], rebuild_lkt=False)
    opt, _ = salt_amd.AlnOpt.from_argv(optargs, idx.l_seed)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1)
    res = aln.alnse_core1(opt, seqs, offs)
    n_heavy = len(aln.heavy_reads())
    aln.close()
    ora = oracle_py.Oracle(w["prefix"])
    oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
    want = ora.align(oo, seqs, offs, n_threads=8)
    ora.close()
    idx.destroy()
    bad = oracle_py.compare(res, want)
    assert len(bad) == 0, "reads differing: %s (heavy queue %d)" % (bad[:10], n_heavy)
    assert (res["pos"] != 0xFFFFFFFF).mean() > 0.9


def test_gpu_verify_and_lv_units_match_reference_vectors():
    """ed_mismatch / ed_diff / ed_diff_withcigar known answers printed by the reference's own units
    (tests/golden/lv_vectors.txt) against both LV kernels and the CIGAR traceback on the GPU.  The one-candidate-per-lane
    kernel must answer every vector within its limits (gap_cases.run_lv_units) and none beyond them."""
    import gap_cases
    from conftest import GOLDEN
    n, n_lane = gap_cases.run_lv_units(os.path.join(GOLDEN, "lv_vectors.txt"))
    assert n == 4000 and n_lane > 1000


def test_cli_salt_matches_reference_golden(tmp_path):
    """The C++ drop-in CLI (salt_amd/bin/salt) on an index written by salt_amd/bin/salt-idx: SAM stream
    identical to the reference's for the same command line (the dated @PG line excluded)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    if not (os.path.exists(salt) and os.path.exists(salt_idx)):
        subprocess.run(["make", "-C", os.path.join(root, "salt_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    for case, extra in (("se_default", []), ("se_r1_m500", ["--gpus", "1", "-t", "4"])):
        args = read_cases()[case]
        out = subprocess.run([salt] + args + extra + [prefix, os.path.join(LAMBDA, "reads_se.fq")], check=True,
                             capture_output=True).stdout
        got = b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
        want = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
        assert got == want, case


@pytest.mark.parametrize("case", sorted(EXTRA_CASES))
def test_gpu_and_cli_match_reference_on_boundary_and_ragged_reads(case, lam, tmp_path):
    """The reference's own SAM (a) for reads straddling the contig boundary, hanging over the genome's start / end (candidate
    positions wrap below 0 or run past mixRef.l) and lying exactly at contig ends (make_span_fixture.py); (b) for mixed read
    lengths 19..300 bp, SE and PE with unequal mates (make_ragged_fixture.py) -- through the C ABI and through the C++ CLI."""
    salt_amd, idx, aln, _ = lam
    args, files = EXTRA_CASES[case]
    paths = [os.path.join(LAMBDA, f) for f in files]
    want = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    opt, _ = salt_amd.AlnOpt.from_argv(args, idx.l_seed)
    if len(paths) == 1:
        names, seqs, offs, quals = salt_amd.read_fastq(paths[0])
        got = salt_amd.sam_text(idx, opt, names, seqs, offs, quals, aln.alnse_core1(opt, seqs, offs))
    else:
        names, seqs, offs, quals = salt_amd.interleave_pairs(salt_amd.read_fastq(paths[0]), salt_amd.read_fastq(paths[1]))
        got = salt_amd.sam_text_pe(idx, opt, names, seqs, offs, quals, aln.alnpe_core1(opt, idx, seqs, offs))
    assert got == want
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    out = subprocess.run([salt] + args + [prefix] + paths, check=True, capture_output=True).stdout
    assert b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG")) == want


def _oracle_compare(prefix, seqs, offs, optargs=()):
    import sys
    import salt_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_py
    idx = salt_amd.Index.reload(prefix)
    opt, _ = salt_amd.AlnOpt.from_argv(list(optargs), idx.l_seed)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=max(len(offs) - 1, 1), max_bases=max(int(offs[-1]), 1) + 64)
    res = aln.alnse_core1(opt, seqs, offs)
    aln.close()
    ora = oracle_py.Oracle(prefix)
    oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
    want = ora.align(oo, seqs, offs, n_threads=8)
    ora.close()
    idx.destroy()
    return res, want, oracle_py.compare(res, want)


def test_gpu_ragged_lengths_n_runs_and_extremes():
    """Edge cases of the batch interface: read lengths from the seed length to 512 in one batch (k_light takes
    <= 160, the rest go through the k_heavy queue and the diagonal-per-lane LV), reads full of N (> 200 N are
    skipped like alnse.c:1328), a read of exactly the seed length, contig-end reads."""
    import salt_amd
    rng = np.random.default_rng(5)
    from salt_amd import api
    g = api.read_fastq  # noqa: F841
    genome = []
    with open(os.path.join(LAMBDA, "genome.fa")) as f:
        cur = []
        for line in f:
            if line.startswith(">"):
                if cur:
                    genome.append("".join(cur))
                cur = []
            else:
                cur.append(line.strip())
        genome.append("".join(cur))
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    reads = []
    lens = [19, 20, 36, 50, 75, 100, 101, 120, 121, 129, 130, 150, 160, 161, 200, 250, 300, 400, 512] * 12
    for L in lens:
        ci = int(rng.integers(0, 2)); s = genome[ci]
        p = int(rng.integers(0, len(s) - L))
        if rng.random() < 0.1:
            p = len(s) - L                              # at the very end of a contig / the genome
        r = np.array([code[c] for c in s[p:p + L]], dtype=np.uint8)
        k = rng.random()
        if k < 0.3:                                     # substitutions
            for _ in range(int(rng.integers(1, 6))):
                q = int(rng.integers(0, L)); r[q] = (r[q] + 1 + rng.integers(0, 3)) & 3 if r[q] < 4 else r[q]
        elif k < 0.5 and L > 30:                        # an indel
            q = int(rng.integers(10, L - 10))
            r = np.concatenate([r[:q], r[q + 1:], r[-1:]]) if rng.random() < 0.5 else np.concatenate([r[:q], [rng.integers(0, 4)], r[q:-1]])
        elif k < 0.6:
            r[rng.integers(0, L, size=min(L, int(rng.integers(1, 12))))] = 4
        if rng.random() < 0.5:
            r = np.where(r[::-1] < 4, 3 - r[::-1], r[::-1])
        reads.append(r.astype(np.uint8))
    reads.append(np.full(300, 4, dtype=np.uint8))       # > 200 N: skipped
    reads.append(np.concatenate([np.full(201, 4), np.zeros(99)]).astype(np.uint8))
    reads.append(np.concatenate([np.full(200, 4), np.array([code[c] for c in genome[0][500:600]])]).astype(np.uint8))   # exactly 200 N: processed
    offs = np.zeros(len(reads) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    seqs = np.concatenate(reads)
    res, want, bad = _oracle_compare(os.path.join(LAMBDA, "idx"), seqs, offs)
    assert len(bad) == 0, bad[:10]
    assert res["skipped"][-3] == 1 and res["skipped"][-2] == 1 and res["skipped"][-1] == 0
    # a one-read batch and a stride-1 seeding batch on short reads
    res1, want1, bad1 = _oracle_compare(os.path.join(LAMBDA, "idx"), reads[5], np.array([0, len(reads[5])], dtype=np.uint32))
    assert len(bad1) == 0
    short = [r for r in reads if len(r) <= 120][:60]
    so = np.zeros(len(short) + 1, dtype=np.uint32); so[1:] = np.cumsum([len(r) for r in short])
    _, _, bad2 = _oracle_compare(os.path.join(LAMBDA, "idx"), np.concatenate(short), so, ["-r", "1", "-m", "500"])
    assert len(bad2) == 0


def test_gpu_one_workspace_takes_batches_of_growing_read_length():
    """A 100-base batch followed by a 200-base batch (then 100 again) through ONE workspace: the second batch regrows the packed-read
    records; the result-head staging buffers must survive that (they were freed there once and used afterwards)."""
    import sys
    import salt_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_py
    prefix = os.path.join(LAMBDA, "idx")
    names, seqs, offs, quals = salt_amd.read_fastq(os.path.join(LAMBDA, "reads_ragged.fq"))
    lens = np.diff(offs.astype(np.int64))
    def batch(sel):
        rs = [seqs[offs[i]:offs[i + 1]] for i in sel]
        o = np.zeros(len(rs) + 1, dtype=np.uint32); o[1:] = np.cumsum([len(r) for r in rs])
        return np.concatenate(rs), o
    short = [i for i in range(len(lens)) if lens[i] <= 100][:150]
    long_ = [i for i in range(len(lens)) if 150 <= lens[i] <= 300][:150]
    assert len(short) > 50 and len(long_) > 20
    idx = salt_amd.Index.reload(prefix)
    opt, _ = salt_amd.AlnOpt.from_argv([], idx.l_seed)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=256, max_bases=256 * 512)
    ora = oracle_py.Oracle(prefix)
    oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
    for sel in (short, long_, short, long_):
        s, o = batch(sel)
        got = aln.alnse_core1(opt, s, o).copy()
        want = ora.align(oo, s, o, n_threads=4)
        assert len(oracle_py.compare(got, want)) == 0
    ora.close(); aln.close(); idx.destroy()


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5, 6])
def test_gpu_verifiers_never_dereference_a_wrapped_locate(mode):
    """Candidates at or beyond mixRef.l -- `pos - offset` that wrapped below 0 passes the reference's range check (alnse.c:672-673)
    and is only dropped by the candidate rule (alnse.c:762) -- must come back as "no hit" from every verifier without being used as an
    address.  Fault-free: the mixRef here is 4 KB and the wild values are 0xFFFFFFF0-style, so a regression shows as a wrong byte (or
    a fault), a correct build as 255; in-range candidates must still give the masked Hamming distance.  Modes 5 / 6 are modes 3 / 4 on
    half-waves, two cases a wave: neighbouring cases differ in length, so the halves of a wave do not run in step."""
    import ctypes
    from salt_amd import api
    lib = api.gpu_lib()
    rng = np.random.default_rng(11 + mode)
    ref_len = 8000
    masks = (1 << rng.integers(0, 4, size=ref_len)).astype(np.uint32)
    snp = rng.random(ref_len) < 0.05
    masks[snp] |= (1 << rng.integers(0, 4, size=int(snp.sum()))).astype(np.uint32)
    words = np.zeros((ref_len + 7) // 8, dtype=np.uint32)
    for q in range(8):
        m = masks[q::8]
        words[:len(m)] |= m << np.uint32(4 * q)
    Ls = [100, 120, 37, 8, 64] if mode in (0, 1, 3, 5) else [150, 248, 121]
    if mode == 0:
        Ls += [300]
    reads, cands, coffs, want = [], [], [0], []
    for L in Ls * 8:
        p = int(rng.integers(0, ref_len - L))
        r = np.array([int(np.log2(int(m) & -int(m))) for m in masks[p:p + L]], dtype=np.uint8)
        e = rng.random(L) < 0.02
        r[e] = (r[e] + 1) & 3
        wild = [0xFFFFFFF0, 0xFFFFFFFF, 0xFFFFFF9C, 0x80000000, ref_len, ref_len + 5, 0xFFFF0000]
        good = [p, max(0, p - 1), int(rng.integers(0, ref_len - L))]
        c = [int(x) for x in rng.permutation(np.array(wild + good + wild[:3], dtype=np.uint64))]
        for x in c:
            if x >= ref_len:
                want.append(255)
            else:
                mm = int(sum(1 for i in range(L) if x + i < ref_len and not (int(masks[x + i]) >> int(r[i])) & 1)) + max(0, x + L - ref_len)
                want.append(mm if mm <= 3 else 255)
        reads.append(r); cands += c; coffs.append(len(cands))
    offs = np.zeros(len(reads) + 1, dtype=np.uint32); offs[1:] = np.cumsum([len(r) for r in reads])
    seqs = np.concatenate(reads)
    cand = np.array(cands, dtype=np.uint32); co = np.array(coffs, dtype=np.uint32)
    out = np.zeros(len(cand), dtype=np.uint8)
    rc = lib.salt_gpu_diag_verify(words.ctypes.data, ref_len, len(reads), seqs.ctypes.data, offs.ctypes.data, cand.ctypes.data, co.ctypes.data,
                                  mode, out.ctypes.data)
    assert rc == 0, lib.salt_gpu_last_error()
    # candidates whose window runs past the end are never produced by locate (pos + L <= l is checked there): compare only windows inside
    inside = np.array([(c >= ref_len) or (c + int(offs[i + 1] - offs[i]) <= ref_len) for i in range(len(reads)) for c in cands[coffs[i]:coffs[i + 1]]])
    assert np.array_equal(out[inside], np.array(want, dtype=np.uint8)[inside]), (mode, np.nonzero(out[inside] != np.array(want, dtype=np.uint8)[inside])[0][:10])


def test_gpu_rejects_what_it_cannot_do():
    """Loud errors instead of silent fallbacks: reads above SALT_MAX_READ_LEN = 512 bases (the kernels' LDS records; the reference's
    Landau-Vishkin caps k at 30, LandauVishkin.c:13, so it aligns nothing meaningful beyond ~300 bases), -m above 262 144 (the located rows
    of a strand: 1 024 in LDS, up to MAX_LOC_POS = 0x40000 in global memory).  The message names the limit."""
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=8, max_bases=8192)
    seq = np.zeros(600, dtype=np.uint8)
    with pytest.raises(salt_amd.SaltError, match="SALT_MAX_READ_LEN"):
        aln.alnse_core1(salt_amd.AlnOpt(l_seed=idx.l_seed), seq, np.array([0, 600], dtype=np.uint32))
    with pytest.raises(salt_amd.SaltError, match="262144"):
        aln.alnse_core1(salt_amd.AlnOpt(l_seed=idx.l_seed, max_locate=300000), seq[:100], np.array([0, 100], dtype=np.uint32))
    aln.alnse_core1(salt_amd.AlnOpt(l_seed=idx.l_seed, max_locate=5000), seq[:100], np.array([0, 100], dtype=np.uint32))     # fine since round 3
    aln.close()
    idx.destroy()


def test_gpu_stride_one_seeding_on_long_reads_matches_oracle():
    """-r 1 on reads of 150 ... 300 bases: up to 282 seed slots per strand (the first round stopped at 128), with -m 500 and the
    default cap: every field against the oracle."""
    import salt_amd
    names, seqs, offs, quals = salt_amd.read_fastq(os.path.join(LAMBDA, "reads_ragged.fq"))
    lens = np.diff(offs.astype(np.int64))
    sel = [i for i in range(len(lens)) if lens[i] >= 150][:120]
    assert len(sel) >= 60 and max(lens[sel]) >= 290
    rs = [seqs[offs[i]:offs[i + 1]] for i in sel]
    o = np.zeros(len(rs) + 1, dtype=np.uint32); o[1:] = np.cumsum([len(r) for r in rs])
    for optargs in (["-r", "1"], ["-r", "1", "-m", "500", "-s", "10"], ["-r", "2", "-v"]):
        res, want, bad = _oracle_compare(os.path.join(LAMBDA, "idx"), np.concatenate(rs), o, optargs)
        assert len(bad) == 0, (optargs, bad[:5])


def _sequential_rule(pos, val, bound, vmax, in_range):
    """The reference's candidate loop on the SORTED, duplicate-free list (code_kmismatch alnse.c:348-369 / code_kdiff
    alnse.c:371-393 as alnse_check_nogap / alnse_check_withgap drive it): returns what the kernels must reproduce."""
    seen, cand = set(), []
    for p, v in sorted(zip(pos, val)):
        if p in seen:
            continue
        seen.add(p)
        if in_range(p):
            cand.append((p, v))
    found, best_pos, best_v, hits, a0 = 0, 0, 0, [], 0
    for p, v in cand:
        if v > vmax or v > bound:
            continue
        if v < bound or not found:
            bound, best_pos, best_v = v, p, v
        if len(hits) < 6:
            hits.append((p, v))
        if not found:
            a0 = v
        found = 1
    return found, best_pos, best_v, hits, a0, bound


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_gpu_rule_on_unsorted_lists_equals_the_sequential_rule(mode):
    """rule_unsorted / rule_sparse (no sort, duplicates allowed) against the sequential loop over the sorted unique list, on
    3000 random lists: lengths 0..300, few distinct loci or many, duplicates, loci at and beyond the reference end, every
    incoming bound.  Mode 3 is rule_sparse on half-waves, two lists a wave: neighbouring lists differ in length, so a half that
    leaked into the other would show."""
    import ctypes
    import salt_amd
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_diag_rule.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    rng = np.random.Generator(np.random.PCG64(100 + mode))
    L, ref_len, vmax = 100, 1000000, (3 if mode != 2 else 12)
    in_range = (lambda p: p < ref_len) if mode != 2 else (lambda p: not ((p + L + 4) & 0xFFFFFFFF >= ref_len))
    pos, val, offs, bounds = [], [], [0], []
    for c in range(3000):
        n = int(rng.choice([0, 1, 2, 5, 17, 63, 64, 65, 128, 300]))
        n_distinct = int(rng.choice([1, 2, 3, 8, 1000]))
        lo = ref_len - 200 if rng.random() < 0.2 else 0                   # some lists straddle the reference end
        universe = rng.integers(lo, ref_len + 150 if lo else ref_len - 200, size=max(n_distinct, 1), dtype=np.int64)
        p = universe[rng.integers(0, len(universe), size=n)]
        dist_of = {int(u): int(rng.choice([0, 1, 2, 3, 4, 7, 12, 200], p=[.1, .15, .15, .15, .1, .05, .05, .25])) for u in universe}
        v = np.array([dist_of[int(x)] for x in p], dtype=np.uint8)
        v[v > vmax] = 255
        pos.append(p.astype(np.uint32)); val.append(v); offs.append(offs[-1] + n)
        bounds.append(int(rng.integers(0, vmax + 1)) if rng.random() < 0.5 else vmax)
    pos_a = np.concatenate(pos) if offs[-1] else np.zeros(1, np.uint32)
    val_a = np.concatenate(val) if offs[-1] else np.zeros(1, np.uint8)
    offs_a, b_a = np.array(offs, dtype=np.uint32), np.array(bounds, dtype=np.uint32)
    out = np.zeros((3000, 18), dtype=np.uint32)
    rc = lib.salt_gpu_diag_rule(3000, pos_a.ctypes.data, val_a.ctypes.data, offs_a.ctypes.data, b_a.ctypes.data, L, ref_len, mode, out.ctypes.data)
    assert rc == 0, lib.salt_gpu_last_error()
    for c in range(3000):
        found, bp, bv, hits, a0, bound = _sequential_rule([int(x) for x in pos[c]], [int(x) for x in val[c]], bounds[c], vmax, in_range)
        got = [int(x) for x in out[c]]
        want = [found, bp if found else 0, bv if found else 0, len(hits), a0 if hits else 0, bound]
        for h in range(6):
            want += list(hits[h]) if h < len(hits) else [0, 0]
        assert got == want, (mode, c, got, want, pos[c][:10], val[c][:10], bounds[c])


@pytest.mark.parametrize("env", [{"SALT_GPU_HEAVY_PER_CU": "1"}, {"SALT_GPU_ALL_HEAVY": "1"}, {"SALT_GPU_ALL_HEAVY": "1", "SALT_GPU_HEAVY_PER_CU": "3"},
                                 {"SALT_GPU_GAP_PER_CU": "1"}])
def test_gpu_ranged_queue_heads_hand_out_every_item_once(tiny, monkeypatch, env):
    """The persistent kernels take their items through 64 ranged heads (pop_ranged): with one block per CU every block walks through all
    the ranges, with SALT_GPU_ALL_HEAVY the queue is the whole batch (and k_light never zeroes the heads), with one k_gap block per CU the
    gapped items go the same way.  Rows equal to the default workspace's, which the other tests hold against the oracle."""
    import salt_amd

    def differing(a, b):                                     # the fields that mean something (not the stale bytes behind n_hits / n_cigar)
        bad = np.zeros(len(a), dtype=bool)
        for f in ("pos", "strand", "n_diff", "is_gap", "mapq", "b0", "b1", "n_cigar", "skipped"):
            bad |= a[f] != b[f]
        bad |= (a["n_hits"] != b["n_hits"]).any(axis=1)
        for s in range(2):
            for j in range(a["hits"].shape[2]):
                live = (a["n_hits"][:, s] > j) & ~bad
                for f in ("pos", "n_diff", "is_gap"):
                    bad |= live & (a["hits"][f][:, s, j] != b["hits"][f][:, s, j])
        for i in np.nonzero(~bad & (a["pos"] != 0xFFFFFFFF))[0]:
            n = int(a["n_cigar"][i])
            if (a["cigar"][i][:n] != b["cigar"][i][:n]).any():
                bad[i] = True
        return np.nonzero(bad)[0]

    w, seqs, offs = tiny
    idx = salt_amd.Index.reload(w["prefix"], rebuild_lkt=False)
    opt, _ = salt_amd.AlnOpt.from_argv(["-m", "200"], idx.l_seed)
    base = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1)
    want = base.alnse_core1(opt, seqs, offs).copy()
    base.close()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    other = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1)
    try:
        for _ in range(2):                                   # twice: the heads are zeroed per call
            got = other.alnse_core1(opt, seqs, offs)
            bad = differing(got, want)
            assert len(bad) == 0, (env, bad[:10])
    finally:
        other.close()
        idx.destroy()


def test_gpu_attach_to_a_copied_image_gives_the_same_rows(lam):
    """The multi-GPU path on one GPU: the packed device image is copied into another buffer (what the RCCL broadcast in
    bench.py / salt_gpu_index_replicate delivers to the other ranks) and a second aligner attaches to the copy."""
    import ctypes
    salt_amd, idx, aln, (names, seqs, offs, quals) = lam
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_buffer_alloc.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
    lib.salt_gpu_buffer_free.argtypes = [ctypes.c_int, ctypes.c_void_p]
    ptr, nbytes = aln.image()
    buf = ctypes.c_void_p()
    assert lib.salt_gpu_buffer_alloc(0, nbytes, ctypes.byref(buf)) == 0, lib.salt_gpu_last_error()
    other = None
    try:
        aln.image_copy(buf.value, nbytes)
        other = salt_amd.GpuAligner(None, device=0, max_reads=2048, image=(buf.value, nbytes))
        opt, _ = salt_amd.AlnOpt.from_argv(read_cases()["se_default"], idx.l_seed)
        a = aln.alnse_core1(opt, seqs, offs)
        b = other.alnse_core1(opt, seqs, offs)
    finally:
        if other:
            other.close()
        lib.salt_gpu_buffer_free(0, buf)
    assert salt_amd.sam_text(idx, opt, names, seqs, offs, quals, a) == salt_amd.sam_text(idx, opt, names, seqs, offs, quals, b)


def test_gpu_attach_to_the_compact_image_rebuilds_the_kmer_table(lam):
    """What bench.py's ranks > 0 and salt_gpu_index_replicate do: only the compact part of the image (everything but the
    W-mer table) is copied; the receiver tabulates the table itself, owns the result (the transfer buffer is freed before
    aligning), and its full image equals the sender's byte for byte."""
    import ctypes
    salt_amd, idx, aln, (names, seqs, offs, quals) = lam
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_buffer_alloc.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
    lib.salt_gpu_buffer_free.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.salt_gpu_buffer_equal.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]
    _, nbytes = aln.image()
    cptr, cbytes = aln.image_compact()
    assert 0 < cbytes < nbytes
    buf = ctypes.c_void_p()
    assert lib.salt_gpu_buffer_alloc(0, cbytes, ctypes.byref(buf)) == 0, lib.salt_gpu_last_error()
    try:
        aln.image_copy(buf.value, cbytes)
        other = salt_amd.GpuAligner(None, device=0, max_reads=2048, compact=(buf.value, cbytes))
    finally:
        lib.salt_gpu_buffer_free(0, buf)
    try:
        optr, obytes = other.image()
        same = ctypes.c_int(0)
        assert obytes == nbytes
        assert lib.salt_gpu_buffer_equal(0, aln.image()[0], optr, nbytes, ctypes.byref(same)) == 0, lib.salt_gpu_last_error()
        assert same.value == 1
        opt, _ = salt_amd.AlnOpt.from_argv(read_cases()["se_default"], idx.l_seed)
        a = aln.alnse_core1(opt, seqs, offs)
        b = other.alnse_core1(opt, seqs, offs)
    finally:
        other.close()
    assert salt_amd.sam_text(idx, opt, names, seqs, offs, quals, a) == salt_amd.sam_text(idx, opt, names, seqs, offs, quals, b)
    with pytest.raises(salt_amd.SaltError):
        salt_amd.GpuAligner(None, device=0, max_reads=64, compact=(cptr, cbytes - 256))


OPTION_MATRIX = [
    "-g rg1 -d -c", "-g rg1", "-l 100 -d -c", "-M 2 -O 5 -E 2 -d -c", "-n 5 -d -c", "-e -d -c", "-s 1 -d -c", "-s 0 -d -c",
    "-m 1 -d -c", "-m 3 -d -c", "-r 19 -d -c", "-r 40 -d -c", "-r 100 -d -c", "-r 2 -m 1000 -d -c", "-d", "-c", "-t 3 -d -c -v",
    "-p -d -c", "-p -d -c -a 0 -b 100000", "-p -d -c -a 600 -b 500", "-p -c -g lib7 -t 2", "-p -d -c -v -r 3", "-p -d -c -m 5 -s 2",
]


def test_cli_option_matrix_equals_the_oracle(oracle_cli, tmp_path):
    """Every option of the reference's optstring that reaches this path (aln.c:102-124), including the ones it parses and
    ignores (-n -e -M -O -E -l) and degenerate values (-s 0, -m 1, overlap > read, an empty insert window): the C++ CLI's SAM
    against the CPU oracle's.  The oracle itself was compared with the real reference on this same matrix in the build
    container (identical on all rows; DESIGN.md 'oracle pinning')."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    bad = []
    for row in OPTION_MATRIX:
        args = row.split()
        files = [os.path.join(LAMBDA, f) for f in (("reads_pe_1.fq", "reads_pe_2.fq") if "-p" in args else ("reads_se.fq",))]
        got = subprocess.run([salt] + args + [prefix] + files, capture_output=True, env=MATRIX_ENV)
        want = subprocess.run([oracle_cli] + args + [prefix] + files, capture_output=True)
        if got.returncode != want.returncode or strip(got.stdout) != strip(want.stdout):
            bad.append((row, got.returncode, want.returncode, got.stderr[-300:]))
    assert not bad, bad


TANDEM_ROWS = ["-d -c", "-d -c -r 2", "-d -c -s 100000", "-d -c -m 50", "-d -c -r 2 -s 100000", "-d -c -r 1 -s 3 -m 200", "-d -c -v -s 100000",
               "-p -d -c -r 2 -s 100000", "-p -d -c -m 200",       # PE with -m below ~60 here subsamples R intervals with rand(): undefined
               # -m above the 1 024 rows a strand keeps in LDS: the lists move to global memory (the reference's vector grows, alnse.c:678);
               # the oracle equals the real reference on these four rows too (checked in the build container)
               "-d -c -m 1025", "-d -c -m 5000 -s 100000", "-d -c -m 30000 -r 2 -s 100000", "-p -d -c -m 3000 -s 100000"]


def test_cli_on_a_tandem_repeat_equals_the_oracle(oracle_cli, tmp_path):
    """40 000 diverged copies of a 30-base unit: every seed has hundreds to thousands of rows, so the global / per-interval
    locate caps bite (alnse.c:678,719 SE; alnse.c:523,533 PE), the interval-size introsort decides which rows are seen
    (alnse.c:307-308), seed extension runs long (-s) or not at all (-s 100000), and XA lists fill up.  SAM of the C++ CLI
    against the CPU oracle's; the oracle equals the real reference on these rows (checked in the build container)."""
    from salt_amd import workload
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    genome = workload.make_tandem()
    pos, mask = workload.make_snps(genome, 600, seed=5)
    fa, snp, prefix = str(tmp_path / "g.fa"), str(tmp_path / "s.txt"), str(tmp_path / "idx")
    workload.write_fasta(fa, "tandem", genome)
    workload.write_snps(snp, "tandem", genome, pos, mask)
    subprocess.run([salt_idx, "-k", "21", fa, snp, prefix], check=True, stderr=subprocess.DEVNULL)
    seqs, offs, _, _ = workload.make_reads(genome, pos, mask, 400, 100, seed=13)
    se = str(tmp_path / "se.fq")
    workload.write_fastq(se, seqs, offs)
    ps, po, _, _ = workload.make_pairs(genome, pos, mask, 100, 150, seed=9, insert_mean=400, insert_sd=40)
    o1 = np.arange(101, dtype=np.uint32) * 150
    p1, p2 = str(tmp_path / "p1.fq"), str(tmp_path / "p2.fq")
    workload.write_fastq(p1, np.concatenate([ps[po[2 * i]:po[2 * i + 1]] for i in range(100)]), o1)
    workload.write_fastq(p2, np.concatenate([ps[po[2 * i + 1]:po[2 * i + 2]] for i in range(100)]), o1)
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    bad = []
    for row in TANDEM_ROWS:
        args = row.split()
        files = [p1, p2] if "-p" in args else [se]
        got = subprocess.run([salt] + args + [prefix] + files, capture_output=True, env=MATRIX_ENV)
        want = subprocess.run([oracle_cli] + args + [prefix] + files, capture_output=True)
        if got.returncode != want.returncode or strip(got.stdout) != strip(want.stdout):
            g, w = strip(got.stdout).split(b"\n"), strip(want.stdout).split(b"\n")
            d = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
            bad.append((row, got.returncode, want.returncode, len(d), [(g[i][:160], w[i][:160]) for i in d[:2]], got.stderr[-200:]))
    assert not bad, bad


def test_cli_reads_the_fastq_shapes_kseq_reads(tmp_path):
    """query_read_seq goes through kseq.h (query.c:146-239): gzip'ed input, CRLF line ends, and records whose sequence and
    quality span several lines are all legal.  Expected SAMs are the real reference's (tests/golden/make_span_fixture.py)."""
    import gzip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    span = open(os.path.join(LAMBDA, "reads_span.fq"), "rb").read()
    gz, crlf = str(tmp_path / "span.fq.gz"), str(tmp_path / "span_crlf.fq")
    with gzip.open(gz, "wb") as f:
        f.write(span)
    open(crlf, "wb").write(span.replace(b"\n", b"\r\n"))
    want_span = open(os.path.join(LAMBDA, "expect_span_default.sam"), "rb").read()
    for fq, want in ((gz, want_span), (crlf, want_span),
                     (os.path.join(LAMBDA, "reads_wrapped.fq"), open(os.path.join(LAMBDA, "expect_wrapped.sam"), "rb").read())):
        out = subprocess.run([salt, "-d", "-c", prefix, fq], check=True, capture_output=True).stdout
        assert strip(out) == want, fq
    # FASTA has no qualities: the reference crashes on it, this CLI says so
    fa = str(tmp_path / "r.fa")
    open(fa, "w").write(">r1\nACGTACGTACGTACGTACGTACGTACGT\n")
    r = subprocess.run([salt, "-d", "-c", prefix, fa], capture_output=True)
    assert r.returncode != 0 and b"FASTA" in r.stderr


@pytest.mark.parametrize("k", [12, 16, 25, 33, 34, 40])
def test_cli_seed_lengths_equal_the_oracle(k, oracle_cli, tmp_path):
    """The seed length is the INDEX's (`salt-idx -k`, default 25; `.R.seedLen`): k = 12 and 16 end inside the W-mer table (no walk
    at all), 25 is the indexer's default, 33 / 34 straddle the in-register seed limit of k_seed, 40 takes its per-base path.  SAM
    of the C++ CLI against the CPU oracle's, SE with two strides and PE; the oracle equals the real reference on the SE rows for
    all six k (checked in the build container)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", str(k), os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    se = [os.path.join(LAMBDA, "reads_ragged.fq")]
    pe = [os.path.join(LAMBDA, "reads_pe_1.fq"), os.path.join(LAMBDA, "reads_pe_2.fq")]
    for args, files in ((["-d", "-c"], se), (["-d", "-c", "-r", "7"], se), (["-d", "-c", "-p", "-a", "350", "-b", "650"], pe)):
        got = subprocess.run([salt] + args + [prefix] + files, capture_output=True, env=MATRIX_ENV)
        want = subprocess.run([oracle_cli] + args + [prefix] + files, capture_output=True)
        assert got.returncode == want.returncode == 0, (k, args, got.stderr[-300:])
        g, w = strip(got.stdout).split(b"\n"), strip(want.stdout).split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        assert not bad and len(g) == len(w), (k, args, len(bad), [(g[i][:200], w[i][:200]) for i in bad[:2]])


def test_cli_with_the_smallest_kmer_table_has_no_wild_loads(tmp_path):
    """A locate whose `pos - offset` wraps below 0 passes the reference's range check (alnse.c:672-673) and is only dropped by
    the candidate rule; used as an address it reads ~2 GiB past the mixRef, which the 64 GiB W-mer table behind it hides.  With
    SALT_GPU_LKT_LEN=12 (268 MB table) such a load faults: the reads hanging over the genome's start must still give the
    reference's SAM."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    env = dict(os.environ, SALT_GPU_LKT_LEN="12")
    for case in ("span_default", "ragged_r7_s10"):
        args, files = EXTRA_CASES[case]
        out = subprocess.run([salt] + args + [prefix] + [os.path.join(LAMBDA, f) for f in files], capture_output=True, env=env)
        assert out.returncode == 0, out.stderr[-300:]
        got = b"".join(l for l in out.stdout.splitlines(keepends=True) if not l.startswith(b"@PG"))
        assert got == open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read(), case


@pytest.mark.parametrize("rate,edge", [(0.15, False), (0.5, False), (0.01, True)])
def test_cli_on_snp_dense_indexes_equals_the_oracle(rate, edge, oracle_cli, tmp_path):
    """The lambda genome with a SNP at 15 % / 50 % of the positions (1-3 alternative alleles; windows with more than 5 SNPs are
    skipped by the indexer, localPattern.c:246-250, so the R index thins out again at 50 %) and with SNPs packed into the first and
    last 30 bases of both contigs: the R searches, the 4-bit masks in verify / LV / SW and XV tags carry the load.  SAM of the C++
    CLI against the CPU oracle's (SE two strides, PE); the oracle equals the real reference on these rows (build container)."""
    import random
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    rng = random.Random(int(rate * 1000) + edge)
    conts, name, seq = [], None, []
    for l in open(os.path.join(LAMBDA, "genome.fa")):
        if l.startswith(">"):
            if name:
                conts.append((name, "".join(seq)))
            name, seq = l[1:].strip(), []
        else:
            seq.append(l.strip())
    conts.append((name, "".join(seq)))
    lines = []
    for cn, s in conts:
        for p, c in enumerate(s):
            if c == "N" or not (rng.random() < rate or (edge and (p < 30 or p >= len(s) - 30))):
                continue
            r = rng.random()
            al = sorted([c] + rng.sample([x for x in "ACGT" if x != c], 1 if r < 0.7 else 2 if r < 0.9 else 3))
            lines.append("%s\t%d\t%s\t%s\n" % (cn, p + 1, "/".join(al), c))
    snp, prefix = str(tmp_path / "snps.txt"), str(tmp_path / "idx")
    open(snp, "w").write("".join(lines))
    subprocess.run([salt_idx, "-k", "19", os.path.join(LAMBDA, "genome.fa"), snp, prefix], check=True, stderr=subprocess.DEVNULL)
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    se = [os.path.join(LAMBDA, "reads_se.fq")]
    pe = [os.path.join(LAMBDA, "reads_pe_1.fq"), os.path.join(LAMBDA, "reads_pe_2.fq")]
    for args, files in ((["-d", "-c"], se), (["-d", "-c", "-r", "5"], se), (["-d", "-c", "-p", "-a", "350", "-b", "650"], pe)):
        got = subprocess.run([salt] + args + [prefix] + files, capture_output=True, env=MATRIX_ENV)
        want = subprocess.run([oracle_cli] + args + [prefix] + files, capture_output=True)
        assert got.returncode == want.returncode == 0, (args, got.stderr[-300:])
        g, w = strip(got.stdout).split(b"\n"), strip(want.stdout).split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        assert not bad and len(g) == len(w), (args, len(bad), [(g[i][:200], w[i][:200]) for i in bad[:2]])


def test_bench_two_ranks_rehearsal_on_one_gpu(tmp_path):
    """The N > 1 path of bench.py -- rank 0 builds and packs the index, the compact image is broadcast, rank 1 attaches it and
    tabulates its own W-mer table, both time their shard, MAX over ranks -- with two ranks sharing this box's one GPU (gloo instead
    of RCCL, which refuses two ranks on one device).  The multi-GPU runs themselves are the driver's."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SALT_BENCH_SAME_GPU="1", SALT_BENCH_BACKEND="gloo", SALT_BENCH_WORKLOAD="mini", SALT_GPU_LKT_LEN="14",
               SALT_BENCH_CACHE=str(tmp_path))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29531", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--no-cpu", "--e2e-reads", "0"],
                         capture_output=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-600:]
    line = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["scaling"] == "weak" and line["steps"] == 4


def test_bench_line_keeps_its_contract_on_the_mini_workload(tmp_path):
    """bench.py --full at N = 1 on the small workload: ONE JSON line with the driver's keys, the roofline and cpu_baseline objects, the
    paired-end leg, both end-to-end legs (each also with its stream on /dev/null) and parity on a timed step."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SALT_BENCH_WORKLOAD="mini", SALT_GPU_LKT_LEN="14", SALT_BENCH_CACHE=str(tmp_path))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "4", "--warmup", "1", "--cpu-sample", "5000", "--e2e-reads", "40000",
                          "--e2e-pairs", "10000", "--pe-pairs", "5000", "--pe-steps", "4", "--pe-batches", "2", "--pe-check", "1000"],
                         capture_output=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-800:]
    lines = [l for l in out.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["metric"] == "Mreads/s" or d["unit"] == "Mreads/s"
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1 and d["value"] > 0 and d["higher_is_better"] is True and "workload" in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["achieved"] > 0 and r["peak"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r
    c = d["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("port", "reference") and c["sample"]
    assert d["parity"]["path"] == "timed step" and d["parity"]["mismatching_reads"] == 0
    assert d["pe"]["value"] > 0 and d["pe"]["parity"]["mismatching_mates"] == 0 and "roofline" in d["pe"]
    assert d["e2e"]["value"] > 0 and d["e2e"]["value_devnull"] > 0 and d["e2e_pe"]["value"] > 0 and d["e2e_pe"]["value_devnull"] > 0


def test_bench_plain_run_is_lean_and_dumps_the_same_rows_twice(tmp_path):
    """bench.py without --full: the headline line only (no serialized, counter, CPU, paired-end or end-to-end legs), --steps timed
    steps, and --dump-outputs writes the last timed step's rows as float32 / float64 .npy files within 64 MB -- the same files from
    two runs with the same arguments."""
    import json
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SALT_BENCH_WORKLOAD="mini", SALT_GPU_LKT_LEN="14", SALT_BENCH_CACHE=str(tmp_path / "cache"))
    dumps = []
    for run in range(2):
        dd = tmp_path / ("dump%d" % run)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(dd)],
                             capture_output=True, env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-800:]
        lines = [l for l in out.stdout.decode().splitlines() if l.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "Mreads/s"
        assert d["higher_is_better"] is True and d["dtype"] == "u32" and d["metric"]
        for k in ("roofline", "cpu_baseline", "parity", "pe", "e2e", "e2e_pe", "kernel_ms_serialized", "queue_counts"):
            assert k not in d, k
        files = sorted(os.listdir(dd))
        assert "pos.npy" in files and "cigar.npy" in files and "read_index.npy" in files
        assert sum(os.path.getsize(dd / f) for f in files) <= 64 * 10**6
        arrs = {f: np.load(dd / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert (arrs["pos.npy"] != 0xFFFFFFFF).mean() > 0.9
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prefix = str(tmp_path_factory.mktemp("lamidx") / "idx")
    subprocess.run([os.path.join(root, "salt_amd", "bin", "salt-idx"), "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix],
                   check=True, stderr=subprocess.DEVNULL)
    return prefix


@pytest.mark.parametrize("case", ["se_default", "se_r1_m500", "se_refonly", "se_r5_s4_m16", "se_plain_t4"])
def test_cli_text_path_and_host_pipeline_give_the_reference_sam(case, lambda_cli_index, tmp_path):
    """The two SE pipelines of `salt` against the reference's SAM: the text path (FASTQ parsed and SAM formatted by kernels; here with
    chunks of a few KB so that hundreds of chunk boundaries fall inside records, to a pipe and to a regular file) and
    the host pipeline (SALT_HOST_PIPELINE=1: the parser that also reads gzip / multi-line records)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt = os.path.join(root, "salt_amd", "bin", "salt")
    args = read_cases()[case]
    want = open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    cmd = [salt] + args + [lambda_cli_index, os.path.join(LAMBDA, "reads_se.fq")]
    for env in (dict(os.environ, SALT_CHUNK_BYTES="3001"), dict(os.environ, SALT_CHUNK_BYTES="70000"), dict(os.environ, SALT_HOST_PIPELINE="1")):
        out = subprocess.run(cmd, capture_output=True, env=env)
        assert out.returncode == 0, out.stderr[-400:]
        assert strip(out.stdout) == want, (case, env.get("SALT_CHUNK_BYTES"), env.get("SALT_HOST_PIPELINE"))
        if "SALT_HOST_PIPELINE" not in env:
            assert b"text path" in out.stderr
    f = tmp_path / "out.sam"
    with open(f, "wb") as fo:
        out = subprocess.run(cmd, stdout=fo, stderr=subprocess.PIPE, env=dict(os.environ, SALT_CHUNK_BYTES="5000"))
    assert out.returncode == 0 and b"blocks written in turn" in out.stderr, out.stderr[-400:]
    assert strip(open(f, "rb").read()) == want


def test_cli_text_path_records_that_outgrow_their_slot(tmp_path):
    """k_sam_len formats a record's head (flag ... CIGAR) and tail (the tags) into a fixed slot (96 + 224 bytes) that k_sam_write copies; a
    record that outgrows it is written whole by one lane.  A contig name of 120 characters overflows the head of every record mapped
    there and the XA list of every read with hits there: the text path must still print what the host pipeline prints (SE and PE)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt, salt_idx = os.path.join(root, "salt_amd", "bin", "salt"), os.path.join(root, "salt_amd", "bin", "salt-idx")
    fa = open(os.path.join(LAMBDA, "genome.fa"), "rb").read().split(b"\n")
    names = [l[1:].split()[0] for l in fa if l.startswith(b">")]
    # (the SNP file's chromosome names are cut at 31 characters, hapmap.c: the first contig keeps its name and its SNPs, the second gets the
    # long name and none)
    long_of = {n: (n if k == 0 else n + b"_" + b"x" * (119 - len(n))) for k, n in enumerate(names)}
    (tmp_path / "g.fa").write_bytes(b"\n".join((b">" + long_of[l[1:].split()[0]]) if l.startswith(b">") else l for l in fa))
    snps = open(os.path.join(LAMBDA, "snps.txt"), "rb").read().split(b"\n")
    (tmp_path / "s.txt").write_bytes(b"\n".join(l for l in snps if l.split(b"\t")[0] == names[0]) + b"\n")
    prefix = str(tmp_path / "idx")
    subprocess.run([salt_idx, "-k", "19", str(tmp_path / "g.fa"), str(tmp_path / "s.txt"), prefix], check=True, stderr=subprocess.DEVNULL)
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    for args in (["-d", "-c", prefix, os.path.join(LAMBDA, "reads_se.fq")],
                 ["-d", "-c", "-p", "-a", "350", "-b", "650", prefix, os.path.join(LAMBDA, "reads_pe_1.fq"), os.path.join(LAMBDA, "reads_pe_2.fq")]):
        a = subprocess.run([salt] + args, capture_output=True, env=dict(os.environ, SALT_CHUNK_BYTES="50000"))
        b = subprocess.run([salt] + args, capture_output=True, env=dict(os.environ, SALT_HOST_PIPELINE="1"))
        assert a.returncode == 0 and b.returncode == 0, (a.stderr[-300:], b.stderr[-300:])
        assert b"text path" in a.stderr and b"text path" not in b.stderr
        assert strip(a.stdout) == strip(b.stdout)
        body = [l for l in a.stdout.split(b"\n") if l and not l.startswith(b"@")]
        assert sum(1 for l in body if len(l.split(b"\t")[2]) == 120) > 100         # heads beyond the slot were there to be written


def test_cli_text_path_reads_crlf_and_a_last_record_without_newline(lambda_cli_index, tmp_path):
    """CRLF line ends and a file that ends without a newline, through the text path (chunked) and the host pipeline alike."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt = os.path.join(root, "salt_amd", "bin", "salt")
    src = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().splitlines()[:800]
    fq = tmp_path / "crlf.fq"
    fq.write_bytes(b"\r\n".join(src))                      # no newline after the last quality line
    cmd = [salt, "-d", "-c", lambda_cli_index, str(fq)]
    strip = lambda out: b"".join(l for l in out.splitlines(keepends=True) if not l.startswith(b"@PG"))
    a = subprocess.run(cmd, capture_output=True, env=dict(os.environ, SALT_CHUNK_BYTES="4000"))
    b = subprocess.run(cmd, capture_output=True, env=dict(os.environ, SALT_HOST_PIPELINE="1"))
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-300:], b.stderr[-300:])
    assert b"text path" in a.stderr and strip(a.stdout) == strip(b.stdout)
    want = open(os.path.join(LAMBDA, "expect_se_default.sam"), "rb").read().split(b"\n")
    got = strip(a.stdout).split(b"\n")
    n_hdr = sum(1 for l in want if l.startswith(b"@"))
    assert got[:n_hdr + 200] == want[:n_hdr + 200]


def test_cli_text_path_regrows_its_workspace_when_records_get_shorter(lambda_cli_index, tmp_path):
    """Workspaces of the text path are sized from the file's first records; a file whose head has 500-byte records and whose body has
    230-byte ones puts more reads into a chunk than that promised: the worker re-creates its workspace and the SAM is unchanged."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    salt = os.path.join(root, "salt_amd", "bin", "salt")
    src = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().splitlines()
    recs = [src[i:i + 4] for i in range(0, len(src) - 3, 4)]
    out = []
    for rep in range(16):
        for j, r in enumerate(recs):
            name = b"@r%d_%d" % (rep, j) + (b"_" + b"x" * 280 if rep == 0 and j < 200 else b"")
            out += [name, r[1], b"+", r[3]]
    fq = tmp_path / "mixed.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    assert fq.stat().st_size > 6 << 20
    cmd = [salt, "-d", "-c", "-t", "4", lambda_cli_index, str(fq)]
    strip = lambda o: b"".join(l for l in o.splitlines(keepends=True) if not l.startswith(b"@PG"))
    a = subprocess.run(cmd, capture_output=True, env=dict(os.environ, SALT_CHUNK_MB="4", SALT_TEXT_TRACE="1"))
    b = subprocess.run(cmd, capture_output=True, env=dict(os.environ, SALT_HOST_PIPELINE="1"))
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-300:], b.stderr[-300:])
    assert b"workspace re-created" in a.stderr, a.stderr[-600:]
    assert strip(a.stdout) == strip(b.stdout)


def test_gpu_context_table_rules_rows_out_without_changing_a_result(tmp_path):
    """The context table (c_ctx, salt_device.h) lets k_heavy drop located rows whose window has more than 3 mismatches for certain.
    A tandem-repeat genome (every seed hits hundreds of diverged copies) with one SNP per ~60 bases (contexts full of special sites),
    reads with N, reads at both ends of the genome: every field equals the oracle's, equals the run without the table, and the table
    did rule rows out."""
    import sys
    import salt_amd
    from salt_amd import workload
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import oracle_py
    genome = workload.make_tandem(divergence=0.08)
    pos, mask = workload.make_snps(genome, 20000, seed=6)
    fa, snp, prefix = str(tmp_path / "g.fa"), str(tmp_path / "s.txt"), str(tmp_path / "idx")
    workload.write_fasta(fa, "tandem", genome)
    workload.write_snps(snp, "tandem", genome, pos, mask)
    subprocess.run([os.path.join(root, "salt_amd", "bin", "salt-idx"), "-k", "21", fa, snp, prefix], check=True, stderr=subprocess.DEVNULL)
    seqs, offs, _, _ = workload.make_reads(genome, pos, mask, 3000, 100, seed=21)
    seqs = seqs.copy()
    rng = np.random.default_rng(4)
    for r in rng.choice(3000, 300, replace=False):              # N inside the contexts of some reads
        seqs[int(offs[r]) + rng.integers(0, 100, 3)] = 4
    ends = np.concatenate([genome[:100], genome[-100:], genome[1:101], genome[-101:-1]]).astype(np.uint8)
    seqs = np.concatenate([seqs, ends]); offs = np.concatenate([offs, offs[-1] + 100 * np.arange(1, 5, dtype=np.uint32)]).astype(np.uint32)
    n = len(offs) - 1
    idx = salt_amd.Index.reload(prefix)
    opt, _ = salt_amd.AlnOpt.from_argv([], idx.l_seed)
    opt.collect_counters = 1
    got = {}
    for no_ctx in ("0", "1"):
        os.environ["SALT_GPU_NO_CTX"] = no_ctx
        try:
            aln = salt_amd.GpuAligner(idx, device=0, max_reads=n, max_bases=int(offs[-1]) + 64)
            aln.counters()
            got[no_ctx] = (aln.alnse_core1(opt, seqs, offs).copy(), aln.counters())
            aln.close()
        finally:
            del os.environ["SALT_GPU_NO_CTX"]
    assert got["0"][1]["d_ctx_rejected"] > 10000 and got["0"][1]["d_ctx_rows"] > got["0"][1]["d_ctx_rejected"], got["0"][1]
    assert got["1"][1]["d_ctx_rows"] == 0
    assert got["0"][0].tobytes() == got["1"][0].tobytes()
    ora = oracle_py.Oracle(prefix)
    want = ora.align(ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref), seqs, offs, n_threads=8)
    ora.close()
    idx.destroy()
    bad = oracle_py.compare(got["0"][0], want)
    assert len(bad) == 0, bad[:5]


def test_gpu_more_gapped_reads_than_k_gap_slots_take_the_overflow_pass(monkeypatch):
    """k_heavy's usual shape hands gapped reads to k_gap through a slot each (as many as the workspace has reads, up to 2^20) and rows in
    a pool; a read that finds neither goes to the overflow queue and is finished by the all-in-one shape launched behind it.  90 000
    reads with an indel each in ONE batch with the slots cut to 20 000 (SALT_GPU_GAP_SLOTS): every field against the oracle."""
    import salt_amd
    monkeypatch.setenv("SALT_GPU_GAP_SLOTS", "20000")
    rng = np.random.default_rng(17)
    genome = []
    with open(os.path.join(LAMBDA, "genome.fa")) as f:
        cur = []
        for line in f:
            if line.startswith(">"):
                if cur:
                    genome.append("".join(cur))
                cur = []
            else:
                cur.append(line.strip())
        genome.append("".join(cur))
    code = np.frombuffer(genome[0].encode(), dtype=np.uint8)
    g = np.full(len(code), 4, dtype=np.uint8)
    for i, c in enumerate(b"ACGT"):
        g[(code == c) | (code == c + 32)] = i
    n, L = 90_000, 100
    start = rng.integers(0, len(g) - L - 8, n)
    p = rng.integers(20, 80, n)
    idx = start[:, None] + np.arange(L)[None, :]
    idx = np.where(np.arange(L)[None, :] >= p[:, None], idx + 2, idx)          # a 2-base deletion at p
    seqs = g[idx].reshape(-1)
    offs = (np.arange(n + 1, dtype=np.uint64) * L).astype(np.uint32)
    res, want, bad = _oracle_compare(os.path.join(LAMBDA, "idx"), seqs, offs)
    assert len(bad) == 0, (len(bad), bad[:5])
    assert int((want["is_gap"] == 1).sum()) > 70_000                            # 50 000 and more of them took the overflow pass
