"""k_heavy's chain from the pop to the located rows (salt_amd/csrc/salt_align.hip: heavy_body, align_general, build_candidates and
the seed-interval sort, which runs in lanes for lists of up to 64 seeds).  Every field against the CPU oracle on a genome made for
the shapes where that code can go wrong: families of 2, 3, 4, 8, 17, 63, 64, 65 and 300 copies of a unit (equal interval sizes: the order of equal keys decides
which rows lie in front of the cap), short units of 1 - 5 copies, a copy cut off by the genome's end (rows the range filter
removes in front of the cap), a stretch with a SNP every 12 bases (reads that have R intervals only), and -m set around the row
totals of the families.  The heavy counters of three batches are held to the values the parent of the change gave for them
(tests/golden/heavy_chain_counters.json; `python tests/test_gpu_heavy_chain.py --record` writes the file).
Settings go in through the environment, read when the index is attached / the workspace is made; SALT_GPU_HEAVY_BIG is read once a
process and gets a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLDEN_COUNTERS = os.path.join(ROOT, "tests", "golden", "heavy_chain_counters.json")

pytestmark = pytest.mark.gpu

K = 19
L = 100
FAMILIES = (2, 3, 4, 8, 17, 63, 64, 65, 300)
UNIT = 150
SETTINGS = ("SALT_GPU_ALL_HEAVY", "SALT_GPU_HEAVY_PER_CU", "SALT_GPU_HEAVY_BIG", "SALT_GPU_NO_CTX", "SALT_GPU_NO_RCTX", "SALT_GPU_GAP_SLOTS")


def make_genome():
    """-> (genome codes, SNP positions, SNP masks, {family size: [copy starts]}, start of the dense-SNP stretch)."""
    rng = np.random.Generator(np.random.PCG64(2020))
    parts, at, starts = [], 0, {}

    def put(a):
        nonlocal at
        parts.append(np.asarray(a, dtype=np.uint8)); at += len(a)

    put(rng.integers(0, 4, size=20000))
    for fi, copies in enumerate(FAMILIES):
        unit = rng.integers(0, 4, size=UNIT).astype(np.uint8)
        starts[copies] = []
        for c in range(copies):
            u = unit.copy()
            if fi % 2 == 1 and c % 3 == 1:                      # every other family: a third of the copies differ in two bases, so
                for q in rng.integers(0, UNIT, size=2):         # the seeds of one read have intervals of different sizes
                    u[q] = (u[q] + 1) & 3
            starts[copies].append(at)
            put(u); put(rng.integers(0, 4, size=int(rng.integers(30, 70))))
    for _ in range(40):                                          # short units of 1 - 5 copies: several small intervals share a trip
        unit = rng.integers(0, 4, size=25).astype(np.uint8)
        for c in range(int(rng.integers(1, 6))):
            put(unit); put(rng.integers(0, 4, size=int(rng.integers(5, 40))))
    dense = at
    put(rng.integers(0, 4, size=400))                            # a SNP every 12 bases goes here
    put(rng.integers(0, 4, size=3000))
    # the genome's last bases: the first 130 of the 17-family's and of the 300-family's unit, so that a read from those families has
    # rows whose window runs past the end
    g0 = np.concatenate(parts)
    put(g0[starts[300][0]:starts[300][0] + UNIT]); put(rng.integers(0, 4, size=37)); put(g0[starts[17][0]:starts[17][0] + 130])
    genome = np.concatenate(parts)
    pos = np.sort(rng.choice(len(genome), size=500, replace=False))
    pos = np.unique(np.concatenate([pos, np.arange(dense + 6, dense + 400, 12)]))
    ref = genome[pos]
    alt = (ref + rng.integers(1, 4, size=len(pos))) & 3
    mask = ((1 << ref) | (1 << alt)).astype(np.uint8)
    return genome, pos.astype(np.int64), mask, starts, dense


def reads_at(genome, pos, mask, start, rng, alt_share=0.5, err=0.004, length=L):
    """Reads of `length` bases at the given starts: a listed allele at every SNP site (the other one with probability alt_share), a few
    substitutions, either strand."""
    site = np.zeros(len(genome), dtype=np.uint8); site[pos] = mask
    idx = np.asarray(start)[:, None] + np.arange(length)[None, :]
    frag = genome[idx].copy()
    m = site[idx]
    flip = (m != 0) & (rng.random(frag.shape) < alt_share)
    other = np.zeros_like(frag)
    for b in range(4):
        other[((m >> b) & 1).astype(bool) & (frag != b)] = b
    frag[flip] = other[flip]
    e = rng.random(frag.shape) < err
    frag[e] = (frag[e] + rng.integers(1, 4, size=int(e.sum()))) & 3
    rc = rng.random(len(frag)) < 0.5
    frag[rc] = 3 - frag[rc][:, ::-1]
    return frag.astype(np.uint8)


def pack(rows):
    offs = np.zeros(len(rows) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in rows])
    return (np.concatenate(rows) if len(rows) else np.zeros(0, np.uint8)).astype(np.uint8), offs


def family_batch(fx, n, seed, families=FAMILIES):
    """n reads: most from the families' copies (any offset inside the unit), some from the short units and the dense-SNP stretch
    (all alternative alleles: no C interval survives), some from anywhere, the genome's very end among them."""
    genome, pos, mask, starts, dense = fx["genome"], fx["pos"], fx["mask"], fx["starts"], fx["dense"]
    rng = np.random.Generator(np.random.PCG64(seed))
    st = []
    for i in range(n):
        k = i % 10
        if k < 6:
            f = families[int(rng.integers(0, len(families)))]
            st.append(starts[f][int(rng.integers(0, len(starts[f])))] + int(rng.integers(0, UNIT - L + 1)))
        elif k == 6:
            st.append(int(rng.integers(starts[300][-1] + UNIT, dense - L)))
        elif k == 7:
            st.append(dense + int(rng.integers(0, 300)))
        elif k == 8:
            st.append(len(genome) - L - int(rng.integers(0, 60)))
        else:
            st.append(int(rng.integers(0, len(genome) - L)))
    st = np.array(st)
    rows = reads_at(genome, pos, mask, st, rng)
    alt_only = reads_at(genome, pos, mask, st, rng, alt_share=1.0, err=0.0)
    sel = (np.arange(n) % 10) == 7
    rows[sel] = alt_only[sel]
    return pack(list(rows))


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    import torch
    import salt_amd
    from salt_amd import api, workload
    d = tmp_path_factory.mktemp("heavy_chain")
    genome, pos, mask, starts, dense = make_genome()
    prefix = str(d / "idx")
    contigs, groups = workload.as_builder_input(genome, pos, mask, 1)
    api.idx_build_mem(contigs, groups, prefix, K, gpu_device=torch.cuda.current_device(), flags=api.IDX_NO_LP)
    f = dict(dir=str(d), prefix=prefix, genome=genome, pos=pos, mask=mask, starts=starts, dense=dense, want={})
    import oracle_py
    f["ora"] = oracle_py.Oracle(prefix)
    saved = {k: os.environ.pop(k) for k in SETTINGS + ("SALT_GPU_LKT_LEN",) if k in os.environ}
    # every attach tabulates the W-mer table of k_seed: W = 12 (16 MB) instead of the device's default (seconds a workspace); the heavy
    # kernels never see it
    os.environ["SALT_GPU_LKT_LEN"] = saved.get("SALT_GPU_LKT_LEN", "12")
    yield f
    f["ora"].close()
    for k in SETTINGS + ("SALT_GPU_LKT_LEN",):
        os.environ.pop(k, None)
    os.environ.update(saved)


def set_env(env):
    for k in SETTINGS:
        os.environ.pop(k, None)
    os.environ.update(env)


def want_se(fx, key, optargs, seqs, offs):
    """The oracle's rows of a batch, computed once."""
    import salt_amd
    k = (key, tuple(optargs))
    if k not in fx["want"]:
        opt, _ = salt_amd.AlnOpt.from_argv(list(optargs), K)
        oo = fx["ora"].opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
        w = fx["ora"].align(oo, seqs, offs, n_threads=8)
        w.setflags(write=False)
        fx["want"][k] = w
    return fx["want"][k]


def gpu_se(fx, env, jobs, counters=False, calls=1):
    """Rows (and counters, and the length of k_heavy's queue) of the jobs (optargs, seqs, offs), in turn, `calls` rounds, on ONE
    workspace made under `env`."""
    import salt_amd
    set_env(env)
    idx = salt_amd.Index.reload(fx["prefix"], rebuild_lkt=False)
    try:
        aln = salt_amd.GpuAligner(idx, device=0, max_reads=max(max(len(o) - 1 for _, _, o in jobs), 1), max_bases=max(max(int(o[-1]) for _, _, o in jobs), 1) + 64)
        try:
            out = []
            for _ in range(calls):
                for optargs, seqs, offs in jobs:
                    opt, _ = salt_amd.AlnOpt.from_argv(list(optargs), idx.l_seed)
                    opt.collect_counters = 1 if counters else 0
                    if counters:
                        aln.counters()
                    res = aln.alnse_core1(opt, seqs, offs).copy()
                    out.append((res, aln.counters() if counters else None, len(aln.heavy_reads())))
            return out
        finally:
            aln.close()
    finally:
        idx.destroy()
        set_env({})


def cap_values(fx):
    """-m around the rows a read inside a family has on its strand (seeds x copies): cap - 1, cap, cap + 1 and cap + 64 * 4 + 1 rows for
    the families of 8 and 17 equal intervals, the small caps that fall inside the first interval, and the default."""
    seeds = (L - K) // K + 1                                     # the default stride is the seed length (aln.c:223)
    v = {1, 2, 3, 16, 17, 18, 63, 64, 65, 1000}
    for copies in (8, 17):
        t = seeds * copies
        v |= {t - 1, t, t + 1}
    t = seeds * 65                                               # 325 rows: 64 * 4 + 1 rows in front of the cap, and the cap on the interval's edge
    v |= {t - 64 * 4 - 1, t - 65, t}
    return sorted(v)


ENVS = [{"SALT_GPU_ALL_HEAVY": "1"}, {"SALT_GPU_ALL_HEAVY": "1", "SALT_GPU_HEAVY_PER_CU": "1"}, {"SALT_GPU_ALL_HEAVY": "1", "SALT_GPU_HEAVY_PER_CU": "3"},
        {"SALT_GPU_ALL_HEAVY": "1", "SALT_GPU_NO_CTX": "1"}, {"SALT_GPU_ALL_HEAVY": "1", "SALT_GPU_NO_RCTX": "1"}, {}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "+".join("%s=%s" % (k[9:], v) for k, v in e.items()) or "default")
def test_caps_around_the_families_row_totals(fx, env):
    """1 200 reads, every -m of cap_values: the sort's order of equal keys and the cap inside an interval, on its edge, behind rows the
    genome's end filtered out."""
    import oracle_py
    seqs, offs = family_batch(fx, 1200, seed=3)
    caps = cap_values(fx)
    out = gpu_se(fx, env, [(["-m", str(m)], seqs, offs) for m in caps])
    for m, (res, _, _) in zip(caps, out):
        bad = oracle_py.compare(res, want_se(fx, "fam1200", ["-m", str(m)], seqs, offs))
        assert len(bad) == 0, (env, m, bad[:10])
    assert (want_se(fx, "fam1200", ["-m", "1000"], seqs, offs)["pos"] != 0xFFFFFFFF).mean() > 0.8


def counter_batches(fx):
    return [(["-m", "64"], family_batch(fx, 1500, seed=11)), (["-m", "200"], family_batch(fx, 1500, seed=12, families=(8, 17, 63, 64, 65))), ([], family_batch(fx, 1500, seed=13))]


def heavy_counters(fx):
    out = []
    for optargs, (seqs, offs) in counter_batches(fx):
        (_, c, _), = gpu_se(fx, {"SALT_GPU_ALL_HEAVY": "1"}, [(optargs, seqs, offs)], counters=True)
        out.append({k: int(c[k]) for k in ("d_sa_heavy", "d_ctx_rows", "d_ctx_rejected", "d_verify_heavy", "sa_c", "sa_r", "loci", "verify")})
    return out


def test_heavy_counters_equal_the_parents(fx):
    """Rows looked up, context rows read and rejected, candidates verified: what the parent library counted for the same batches."""
    want = json.load(open(GOLDEN_COUNTERS))
    got = heavy_counters(fx)
    print(got)
    assert got == want
    assert all(c["d_ctx_rows"] > 10000 and c["d_ctx_rejected"] > 0 and c["d_sa_heavy"] >= c["d_ctx_rows"] for c in got)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4097])
def test_queue_lengths_and_reads_that_leave_early(fx, n):
    """The queue k_heavy pops from holds n reads (with SALT_GPU_ALL_HEAVY the queue is the batch) at one block a CU and at the usual
    grid: fewer items than blocks, as many as a range's heads, more than blocks.  The batch's last reads leave early: too short for a
    seed, all N.  n = 0: 64 exact reads from unique sequence through the default path, k_light finishes them and the queue stays empty."""
    import oracle_py
    rng = np.random.Generator(np.random.PCG64(50 + n))
    if n == 0:
        st = rng.integers(100, 19000, size=64)
        clean = fx["pos"][(fx["pos"] < 20000)]
        st = np.array([s for s in st if not ((clean >= s) & (clean < s + L)).any()][:32])
        seqs, offs = pack(list(reads_at(fx["genome"], fx["pos"], fx["mask"], st, rng, alt_share=0.0, err=0.0)))
        (res, _, queued), = gpu_se(fx, {}, [([], seqs, offs)])
        assert queued == 0
        assert len(oracle_py.compare(res, want_se(fx, "q0", [], seqs, offs))) == 0
        return
    s, o = family_batch(fx, n, seed=60 + n)
    rows = [s[o[i]:o[i + 1]] for i in range(n)]
    if n >= 2:
        rows[-1] = np.full(L, 4, dtype=np.uint8)                 # all N
        rows[-2] = rows[-2][:K - 1]                              # too short for a seed
    seqs, offs = pack(rows)
    want = want_se(fx, "q%d" % n, ["-m", "100"], seqs, offs)
    for env in ({"SALT_GPU_ALL_HEAVY": "1", "SALT_GPU_HEAVY_PER_CU": "1"}, {"SALT_GPU_ALL_HEAVY": "1"}):
        for res, _, _ in gpu_se(fx, env, [(["-m", "100"], seqs, offs)], calls=2):
            bad = oracle_py.compare(res, want)
            assert len(bad) == 0, (n, env, bad[:10])


def test_long_all_n_read_at_the_end_and_more_seed_slots(fx):
    """A batch whose longest read has 300 bases (more seed slots a strand than the 100-base batches have) and more than 200 N (left
    untouched, alnse.c:1328), behind ordinary reads."""
    import oracle_py
    s, o = family_batch(fx, 300, seed=71)
    rows = [s[o[i]:o[i + 1]] for i in range(300)] + [np.full(300, 4, dtype=np.uint8)]
    seqs, offs = pack(rows)
    want = want_se(fx, "longn", ["-m", "100"], seqs, offs)
    for env in ({"SALT_GPU_ALL_HEAVY": "1"}, {}):
        (res, _, _), = gpu_se(fx, env, [(["-m", "100"], seqs, offs)])
        assert len(oracle_py.compare(res, want)) == 0, env
        assert res["skipped"][-1] == 1


def test_gapped_reads_between_ordinary_ones_with_few_gap_slots(fx):
    """Every fifth read has a deletion of two bases (nothing matches gap-free: it is handed to k_gap); with two k_gap slots most of them
    go to the overflow queue and the pass behind k_heavy."""
    import oracle_py
    s, o = family_batch(fx, 600, seed=81)
    rng = np.random.Generator(np.random.PCG64(82))
    rows = [s[o[i]:o[i + 1]] for i in range(600)]
    st = rng.integers(100, 19000, size=600)
    uniq = reads_at(fx["genome"], fx["pos"], fx["mask"], st, rng, length=L + 2)
    for i in range(0, 600, 5):
        rows[i] = np.concatenate([uniq[i][:50], uniq[i][52:]])
    seqs, offs = pack(rows)
    want = want_se(fx, "gapmix", [], seqs, offs)
    assert int((want["is_gap"] == 1).sum()) >= 60
    for env in ({"SALT_GPU_ALL_HEAVY": "1", "SALT_GPU_GAP_SLOTS": "2"}, {"SALT_GPU_GAP_SLOTS": "2"}, {"SALT_GPU_ALL_HEAVY": "1"}):
        (res, _, _), = gpu_se(fx, env, [([], seqs, offs)])
        bad = oracle_py.compare(res, want)
        assert len(bad) == 0, (env, bad[:10])


def test_two_batches_take_turns_on_one_workspace(fx):
    """Nothing fetched ahead survives a call: batches of 700 and 333 reads, twice each, alternately, one workspace."""
    import oracle_py
    a, b = family_batch(fx, 700, seed=91), family_batch(fx, 333, seed=92)
    wants = [want_se(fx, "turnA", ["-m", "64"], *a), want_se(fx, "turnB", ["-m", "64"], *b)]
    for env in ({"SALT_GPU_ALL_HEAVY": "1"}, {}):
        out = gpu_se(fx, env, [(["-m", "64"],) + a, (["-m", "64"],) + b], calls=2)
        for i, (res, _, _) in enumerate(out):
            assert len(oracle_py.compare(res, wants[i % 2])) == 0, (env, i)


def test_pairs_through_k_heavy_pe(fx):
    """The same genome as 2 x 150 pairs, one batch: k_heavy_pe runs build_candidates with the paired-end caps."""
    import salt_amd
    import oracle_py
    from salt_amd import workload
    seqs, offs, *_ = workload.make_pairs(fx["genome"], fx["pos"], fx["mask"], 1000, 150, seed=5)
    set_env({})
    idx = salt_amd.Index.reload(fx["prefix"], rebuild_lkt=False)
    try:
        for optargs in (["-p"], ["-p", "-m", "40"]):
            opt, _ = salt_amd.AlnOpt.from_argv(optargs, idx.l_seed)
            aln = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1)
            try:
                res = aln.alnpe_core1(opt, idx, seqs, offs)
            finally:
                aln.close()
            oo = fx["ora"].opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
            want = fx["ora"].align_pe(oo, seqs, offs, opt.min_tlen, opt.max_tlen, n_threads=8)
            bad = oracle_py.compare(res, want, pe=True)
            assert len(bad) == 0, (optargs, bad[:10])
    finally:
        idx.destroy()


def test_locate_cap_above_the_lds_list_goes_through_k_heavy_glob(fx):
    """-m 5000 (above SALT_MAX_LOCATE = 1 024): the located rows of a strand go to the block's global list."""
    import oracle_py
    seqs, offs = family_batch(fx, 400, seed=95, families=(64, 65, 300))
    want = want_se(fx, "glob", ["-m", "5000"], seqs, offs)
    for env in ({"SALT_GPU_ALL_HEAVY": "1"}, {}):
        (res, _, _), = gpu_se(fx, env, [(["-m", "5000"], seqs, offs)])
        assert len(oracle_py.compare(res, want)) == 0, env


def test_all_in_one_shape_in_a_child_process(fx, tmp_path):
    """SALT_GPU_HEAVY_BIG=1 (read once a process): k_heavy_big takes every read, lists of up to 512 seeds, the LDS form of the sort's
    stack.  The child writes its rows, the oracle's are compared here."""
    import salt_amd
    import oracle_py
    seqs, offs = family_batch(fx, 800, seed=97)
    np.save(str(tmp_path / "seqs.npy"), seqs); np.save(str(tmp_path / "offs.npy"), offs)
    env = dict(os.environ, SALT_GPU_HEAVY_BIG="1", SALT_GPU_ALL_HEAVY="1")
    for optargs in (["-m", "17"], ["-r", "1", "-m", "300"]):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", fx["prefix"], str(tmp_path)] + optargs, check=True, env=env, timeout=120)
        res = np.load(str(tmp_path / "res.npy")).view(salt_amd.RESULT_DTYPE).reshape(-1)
        bad = oracle_py.compare(res, want_se(fx, "big", optargs, seqs, offs))
        assert len(bad) == 0, (optargs, bad[:10])


def _child(prefix, d, optargs):
    import salt_amd
    seqs, offs = np.load(os.path.join(d, "seqs.npy")), np.load(os.path.join(d, "offs.npy"))
    idx = salt_amd.Index.reload(prefix, rebuild_lkt=False)
    opt, _ = salt_amd.AlnOpt.from_argv(list(optargs), idx.l_seed)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1, max_bases=int(offs[-1]) + 64)
    res = aln.alnse_core1(opt, seqs, offs).copy()
    aln.close(); idx.destroy()
    np.save(os.path.join(d, "res.npy"), res.view(np.uint8))


def _record():
    """Writes tests/golden/heavy_chain_counters.json from the library in place (run with the parent's library)."""
    import tempfile
    import torch
    import salt_amd
    from salt_amd import api, workload
    torch.cuda.init()
    os.environ.setdefault("SALT_GPU_LKT_LEN", "12")
    d = tempfile.mkdtemp()
    genome, pos, mask, starts, dense = make_genome()
    prefix = os.path.join(d, "idx")
    contigs, groups = workload.as_builder_input(genome, pos, mask, 1)
    api.idx_build_mem(contigs, groups, prefix, K, gpu_device=0, flags=api.IDX_NO_LP)
    f = dict(prefix=prefix, genome=genome, pos=pos, mask=mask, starts=starts, dense=dense)
    out = heavy_counters(f)
    json.dump(out, open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN_COUNTERS, "w"), indent=1)
    print(out)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        _child(sys.argv[2], sys.argv[3], sys.argv[4:])
    elif sys.argv[1] == "--record":
        _record()
