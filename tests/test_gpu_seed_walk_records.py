"""Walk records that carry the seed's bases: k_seed stores a seed's five tb words (three 2-bit words, two N-flag words) with its queue
record, and k_seed_walk begins the walk from the record alone, without a fetch from the read's tb record.

Everything goes through the C ABI and is held against the CPU oracle, every field (oracle_py.compare), with no differing read
allowed.  Every case runs with SALT_GPU_WALK_BLOCKS=64 (256 waves, 4 per queue segment), so that a wave's slice is many records long
and its lanes refill in mid-flight.  The exact device counters of the seed stage do not count the tb fetch that left the walk: they
are held, without tolerance, against tests/golden/seed_walk_counters.json, which the library of the commit BEFORE the record change
wrote (the file names it)."""
import json
import os

import numpy as np
import pytest

from test_gpu_seed_walk import SEED_CTRS, _Bench, _mixed_genome, _mixed_reads, _oracle_py, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "seed_walk_counters.json")
WALK = {"SALT_GPU_WALK_BLOCKS": "64"}
K_MIXED = 21
STRIDES = (5, 7, 13)
# the strides of the issue, each plain and with a small max_seed / locate cap (extension steps: bases in front of the seed)
OPTSETS = [["-r", str(r)] + extra for r in STRIDES for extra in ([], ["-s", "2", "-m", "200"])]


def _env(no_unique):
    return dict(WALK, SALT_GPU_NO_UNIQUE="1") if no_unique else dict(WALK)


def _mixed_index(tmp, k):
    import salt_amd
    from salt_amd import workload
    genome, rep0, pa0 = _mixed_genome()
    pos, mask = workload.make_snps(genome, 300, seed=5)
    contigs, groups = workload.as_builder_input(genome, pos, mask)
    prefix = os.path.join(str(tmp), "idx%d" % k)
    salt_amd.idx_build_mem(contigs, groups, prefix, k, flags=salt_amd.IDX_NO_LP)
    seqs, offs = _mixed_reads(genome, rep0, pa0, k)
    return prefix, seqs, offs


def _seed_counters(b, monkeypatch, no_unique, optargs):
    """The five seed-stage counters of one call over all of b's reads; the rows are held against the oracle on the way."""
    monkeypatch.delenv("SALT_GPU_NO_UNIQUE", raising=False)
    ws = b.workspace(monkeypatch, _env(no_unique))
    try:
        _run(b, ws, optargs, counters=True)
        c = ws.counters()
        return {k: int(c[k]) for k in SEED_CTRS}
    finally:
        ws.close()


def _golden(name):
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["commit"], g
    return g["cases"][name]


def mixed_case_name(w, no_unique):
    return "mixed_k21_r7_W%s%s" % (w or "default", "_no_unique" if no_unique else "")


def tiny_case_name(no_unique):
    return "tiny_20000_seed7%s" % ("_no_unique" if no_unique else "")


# ---- the mixed genome at k = 21, attached once per W ---------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[None, "12"], ids=["Wdefault", "W12"])
def mixed21(request, tmp_path_factory):
    prefix, seqs, offs = _mixed_index(tmp_path_factory.mktemp("mixed21"), K_MIXED)
    b = _Bench(prefix, seqs, offs, env={} if request.param is None else {"SALT_GPU_LKT_LEN": request.param})
    b.w = request.param
    yield b
    b.close()


def test_strides_reach_the_word_boundaries():
    """What the option sets below place where: with 150-base reads the seed starts s = slot * stride of the strides 5, 7 and 13 take every
    residue modulo 16 (every shift of the 2-bit words) and 30 of the 32 residues modulo 32 (the N-flag words); 12 and 22 are reached
    by no slot of these strides, so the placement test adds stride 1, which takes them all.  The last slots start in the last word
    pair of a strand's tb words (150 bases: 2-bit words 0 .. 9, a seed's three words end at word wb + 2)."""
    L, k = 150, K_MIXED
    starts = {s for r in STRIDES for s in range(0, L - k + 1, r)}
    assert {s % 16 for s in starts} == set(range(16))
    assert set(range(32)) - {s % 32 for s in starts} == {12, 22}
    assert {s % 32 for s in range(0, L - k + 1)} == set(range(32))
    assert (max(starts) >> 4) + 2 == ((L + 15) >> 4) - 1                          # the last slot's third word is the strand's last


@pytest.mark.parametrize("no_unique", [False, True], ids=["resolve", "no_unique"])
def test_every_placement_of_a_seed_in_its_words(mixed21, monkeypatch, no_unique):
    """Unique sequence, the 37-base tandem repeat, poly-A, reads of 21 .. 150 bases with an N at every fifth base, seeds at strides 5, 7
    and 13 (and 1): the head bases, the one-row resolve (context record and text path) and the extension read the record's words at
    every shift.  The workspace's first call runs at the default stride; the -r 5 call behind it has more seed slots than the seed
    arrays and the queue were sized for and goes through their regrow."""
    monkeypatch.delenv("SALT_GPU_NO_UNIQUE", raising=False)
    ws = mixed21.workspace(monkeypatch, _env(no_unique))
    try:
        _run(mixed21, ws, [])
        for optargs in OPTSETS + [["-r", "1"]]:
            _run(mixed21, ws, optargs)
    finally:
        ws.close()


@pytest.mark.parametrize("no_unique", [False, True], ids=["resolve", "no_unique"])
def test_mixed_counters_equal_the_parents(mixed21, monkeypatch, no_unique):
    """-r 7 on the mixed genome: W-mer gathers, Occ blocks of both indexes, suffix-array and text loads, equal to what the commit
    before the record change counted."""
    got = _seed_counters(mixed21, monkeypatch, no_unique, ["-r", "7"])
    want = _golden(mixed_case_name(mixed21.w, no_unique))
    print(got, want)
    assert got == want


# ---- seeds past the in-register limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_unique", [False, True], ids=["resolve", "no_unique"])
def test_seeds_past_the_in_register_limit(tmp_path, monkeypatch, no_unique):
    """k = 34 at W = 12 with -r 9: a walk takes nothing from the record's words and every base from tb, step by step."""
    prefix, seqs, offs = _mixed_index(tmp_path, 34)
    b = _Bench(prefix, seqs, offs, env={"SALT_GPU_LKT_LEN": "12"})
    try:
        monkeypatch.delenv("SALT_GPU_NO_UNIQUE", raising=False)
        ws = b.workspace(monkeypatch, _env(no_unique))
        try:
            _run(b, ws, ["-r", "9"])
        finally:
            ws.close()
    finally:
        b.close()


# ---- the `tiny` workload ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_wl(tmp_path_factory):
    from salt_amd import workload
    return workload.prepare("tiny", str(tmp_path_factory.mktemp("wl")))


@pytest.fixture(scope="module")
def tiny(tiny_wl):
    """The `tiny` workload's index with 20 000 reads of make_reads(..., seed=7)."""
    from salt_amd import workload
    w = tiny_wl
    seqs, offs, _, _ = workload.make_reads(w["genome"], w["snp_pos"], w["snp_mask"], 20000, w["read_len"], seed=7)
    b = _Bench(w["prefix"], seqs, offs)
    yield b
    b.close()


def test_two_calls_of_different_sizes_on_one_workspace(tiny, monkeypatch):
    """20 000 reads, 3 reads, 20 000 again: one memset per call zeroes the batch's control words, k_heavy's queue ranges and the walk
    queues' counters.  A stale walk counter or range head shows as a differing read or a read aligned twice."""
    monkeypatch.delenv("SALT_GPU_NO_UNIQUE", raising=False)
    ws = tiny.workspace(monkeypatch, dict(WALK))
    try:
        for n in (20000, 3, 20000):
            _run(tiny, ws, [], n)
            qc = ws.queue_counts()
            print(n, qc)
    finally:
        ws.close()


@pytest.mark.parametrize("no_unique", [True, False], ids=["no_unique", "resolve"])
def test_tiny_counters_equal_the_parents(tiny, monkeypatch, no_unique):
    """20 000 reads at the default options, every C search walking and with the one-row resolves."""
    got = _seed_counters(tiny, monkeypatch, no_unique, [])
    want = _golden(tiny_case_name(no_unique))
    print(got, want)
    assert got == want


def test_mates_walk_from_their_records(tiny_wl, monkeypatch):
    """2 000 pairs of 2 x 150 bases as the benchmark's paired-end leg makes them (3 % damaged, 1 % orphan mates), `-p -a 250 -b 550`,
    every C search walking: the paired-end step runs the same two seed kernels on the 2n mates."""
    import salt_amd
    import torch
    from salt_amd import workload
    w = tiny_wl
    dev = torch.device("cuda:0")
    genome = torch.from_numpy(np.ascontiguousarray(w["genome"])).to(dev)
    pos = torch.from_numpy(np.asarray(w["snp_pos"]).astype(np.int64)).to(dev)
    mask = torch.from_numpy(np.asarray(w["snp_mask"]).astype(np.uint8)).to(dev)
    site = workload.make_site_map(genome.numel(), pos, mask)
    seqs, offs = workload.make_pairs_hash(genome, site, 2000, 150, seed=3, batch=0, damaged=0.03, orphan=0.01)[:2]
    seqs, offs = seqs.cpu().numpy().astype(np.uint8), offs.cpu().numpy().astype(np.uint32)
    del genome, pos, mask, site
    for k, v in _env(True).items():
        monkeypatch.setenv(k, v)
    idx = salt_amd.Index.reload(w["prefix"])
    opt, _ = salt_amd.AlnOpt.from_argv(["-p", "-a", "250", "-b", "550"], idx.l_seed)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1, max_bases=int(offs[-1]) + 64)
    try:
        res = aln.alnpe_core1(opt, idx, seqs, offs)
    finally:
        aln.close()
    oracle_py = _oracle_py()
    ora = oracle_py.Oracle(w["prefix"])
    oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
    want = ora.align_pe(oo, seqs, offs, opt.min_tlen, opt.max_tlen, n_threads=16)
    ora.close()
    idx.destroy()
    bad = oracle_py.compare(res, want, pe=True)
    assert len(bad) == 0, (len(bad), bad[:10])
    assert (res["pos"] != 0xFFFFFFFF).mean() > 0.9
