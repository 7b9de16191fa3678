"""k_seed_walk in turns: one step per lane a turn, idle lanes refilled from the wave's static slice of the walk queues.

Everything goes through the C ABI and is held against the CPU oracle, every field (oracle_py.compare), with no differing read
allowed.  SALT_GPU_WALK_BLOCKS sets the walk kernel's grid (64 blocks = 256 waves, 4 per queue segment), so that on small inputs
a wave's slice is many times 64 records long and its lanes refill again and again; SALT_GPU_NO_UNIQUE makes every C search walk
its head bases instead of resolving one-row intervals.  Both are read when a workspace is created."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MANY = 20000
SEED_CTRS = ("d_wlkt", "d_cocc_seed", "d_rocc_seed", "d_sa_seed", "d_text_seed")


def _oracle_py():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    return oracle_py


class _Bench:
    """One attached index, the oracle beside it, and the oracle's rows per (reads, options), computed once."""

    def __init__(self, prefix, seqs, offs, env=None):
        import salt_amd
        import torch
        torch.cuda.empty_cache()                            # what the generators and the device suffix sorter of earlier tests left cached
        self.salt = salt_amd
        self.prefix, self.seqs, self.offs = prefix, seqs, offs
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            self.idx = salt_amd.Index.reload(prefix, rebuild_lkt=False)
            self.base = salt_amd.GpuAligner(self.idx, device=0, max_reads=64, max_bases=64 * 160)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        self.ora = _oracle_py().Oracle(prefix)
        self._want = {}

    def opt(self, optargs, counters=False):
        o, _ = self.salt.AlnOpt.from_argv(list(optargs), self.idx.l_seed)
        o.collect_counters = 1 if counters else 0
        return o

    def want(self, optargs, n=None):
        key = tuple(optargs)
        if key not in self._want:
            o = self.opt(optargs)
            oo = self.ora.opt(l_overlap=o.l_overlap, max_seed=o.max_seed, max_locate=o.max_locate, seed_only_ref=o.seed_only_ref)
            self._want[key] = self.ora.align(oo, self.seqs, self.offs, n_threads=8)
        w = self._want[key]
        return w if n is None else w[:n]

    def workspace(self, monkeypatch, env, n=None):
        """A workspace of its own on the attached index, created under `env`."""
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        n = len(self.offs) - 1 if n is None else n
        return self.base.fork(max_reads=max(n, 1), max_bases=int(self.offs[n]) + 64)

    def close(self):
        self.ora.close()
        self.base.close()
        self.idx.destroy()


# These come first in the file: k = 16 attaches a 64 GiB W-mer table, which wants the device free of this module's other index.
# ---- long and short walks in one wave ----------------------------------------------------------------------------------------------
def _mixed_genome():
    """Unique sequence, a tandem repeat (300 nearly identical copies of a 37-base unit: intervals stay above max_seed, so the extension
    runs until it has used all the bases in front of the seed), a poly-A stretch, unique sequence again."""
    rng = np.random.Generator(np.random.PCG64(2024))
    uniq = lambda n: rng.integers(0, 4, size=n).astype(np.uint8)
    unit = uniq(37)
    rep = np.tile(unit, 300)
    m = rng.random(len(rep)) < 0.002
    rep[m] = (rep[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
    return np.concatenate([uniq(30000), rep, uniq(500), np.zeros(2500, dtype=np.uint8), uniq(30000)]), 30000, 30000 + len(rep) + 500


def _mixed_reads(genome, rep0, pa0, k):
    rng = np.random.Generator(np.random.PCG64(7 + k))
    lens = sorted({k, max(41, k + 7), 100, 150})
    reads = []
    for L in lens:
        for j in range(40):
            kind = j % 4
            if kind == 0:
                p = rep0 + int(rng.integers(0, 37 * 290 - L))                  # inside the repeat
            elif kind == 1:
                p = pa0 + int(rng.integers(0, 2500 - L))                       # inside the poly-A stretch
            elif kind == 2:
                p = int(rng.integers(0, 30000 - L))                            # unique
            else:
                p = rep0 - int(rng.integers(1, L))                             # across the repeat's edge
            r = genome[p:p + L].copy()
            if j % 8 >= 4:
                r = np.where(r[::-1] < 4, 3 - r[::-1], r[::-1]).astype(np.uint8)
            reads.append(r)
            # one N at a time, every 5th base: in the W-mer, in the head bases and in the bases the extension consumes, for every slot
            if j < 8:
                for q in range(j % 5, L, 5):
                    rn = r.copy(); rn[q] = 4
                    reads.append(rn)
    offs = np.zeros(len(reads) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads), offs


@pytest.mark.parametrize("k,w", [(21, None), (21, "12"), (16, "16"), (33, "12"), (34, "12")])
def test_long_and_short_walks_in_one_wave(tmp_path, monkeypatch, k, w):
    """Reads inside a tandem repeat (extension until ext == s), inside poly-A, unique reads and reads with an N in the W-mer, the head
    bases or the extension bases, 21 .. 150 bases long, side by side in the same waves.  k = 16 at W = 16 has no head steps (extension
    only), k = 33 / 34 straddle the in-register seed limit, W = 12 gives up to 22 head steps and one-row resolves of more than 16 bases
    (two text pieces)."""
    import salt_amd
    from salt_amd import workload
    genome, rep0, pa0 = _mixed_genome()
    pos, mask = workload.make_snps(genome, 300, seed=5)
    contigs, groups = workload.as_builder_input(genome, pos, mask)
    prefix = str(tmp_path / "idx")
    salt_amd.idx_build_mem(contigs, groups, prefix, k, flags=salt_amd.IDX_NO_LP)
    seqs, offs = _mixed_reads(genome, rep0, pa0, k)
    b = _Bench(prefix, seqs, offs, env={} if w is None else {"SALT_GPU_LKT_LEN": w})
    try:
        for optargs in ([], ["-s", "2", "-m", "200"]):
            for env in ({"SALT_GPU_WALK_BLOCKS": "64"}, {"SALT_GPU_WALK_BLOCKS": "64", "SALT_GPU_NO_UNIQUE": "1"}):
                monkeypatch.delenv("SALT_GPU_NO_UNIQUE", raising=False)
                ws = b.workspace(monkeypatch, env)
                try:
                    _run(b, ws, optargs)
                finally:
                    ws.close()
    finally:
        b.close()


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """The `tiny` workload's genome and index as test_gpu_parity.py prepares them, with 20 000 reads."""
    from salt_amd import workload
    w = workload.prepare("tiny", str(tmp_path_factory.mktemp("wl")))
    seqs, offs, _, _ = workload.make_reads(w["genome"], w["snp_pos"], w["snp_mask"], N_MANY, w["read_len"], seed=7)
    b = _Bench(w["prefix"], seqs, offs)
    yield b
    b.close()


def _run(b, ws, optargs, n=None, calls=1, counters=False):
    n = len(b.offs) - 1 if n is None else n
    opt = b.opt(optargs, counters)
    oracle_py = _oracle_py()
    for _ in range(calls):
        if counters:
            ws.counters()                                   # reading resets them
        res = ws.alnse_core1(opt, b.seqs[:int(b.offs[n])], b.offs[:n + 1])
        bad = oracle_py.compare(res, b.want(optargs, n))
        assert len(bad) == 0, (optargs, n, bad[:10])
    return res


@pytest.mark.parametrize("optargs", [[], ["-s", "2", "-m", "200"]])
def test_lanes_refill_many_times(tiny, monkeypatch, optargs):
    """20 000 reads whose every C seed walks, on 256 waves: a wave's slice holds several hundred records, so every lane takes a new
    record many times while its neighbours are in the middle of theirs."""
    ws = tiny.workspace(monkeypatch, {"SALT_GPU_NO_UNIQUE": "1", "SALT_GPU_WALK_BLOCKS": "64"})
    try:
        res = _run(tiny, ws, optargs)
        assert (res["pos"] != 0xFFFFFFFF).mean() > 0.9
        qc = ws.queue_counts()
        print("longest R list %d, longest C list %d" % (qc[1], qc[3]))
        assert max(qc[1], qc[3]) >= 4 * 64 * 4, qc           # 4 waves on the segment: each slice at least four times the lanes
    finally:
        ws.close()


@pytest.mark.parametrize("blocks", [None, "64"])
@pytest.mark.parametrize("n", [1, 3, 70])
def test_fewer_records_than_lanes_and_none(tiny, monkeypatch, n, blocks):
    """1, 3 and 70 reads: most slices are empty and some hold one record; two calls on one workspace (the queue counters are
    zeroed per call)."""
    ws = tiny.workspace(monkeypatch, {} if blocks is None else {"SALT_GPU_WALK_BLOCKS": blocks}, n)
    try:
        _run(tiny, ws, [], n, calls=2)
    finally:
        ws.close()


def test_seed_only_ref_has_no_r_walks(tiny, monkeypatch):
    """-v: the R lists stay empty."""
    ws = tiny.workspace(monkeypatch, {"SALT_GPU_WALK_BLOCKS": "64"}, 4000)
    try:
        _run(tiny, ws, ["-v"], 4000)
        assert ws.queue_counts()[1] == 0
    finally:
        ws.close()


def test_one_row_resolve_through_suffix_array_and_text(tiny, monkeypatch):
    """Without the context table the one-row resolve is two steps: the suffix-array entry, then the text."""
    b = _Bench(tiny.prefix, tiny.seqs, tiny.offs, env={"SALT_GPU_NO_CTX": "1"})
    b._want = tiny._want
    try:
        ws = b.workspace(monkeypatch, {"SALT_GPU_WALK_BLOCKS": "64"}, 4000)
        try:
            opt = b.opt([], True)
            ws.counters()
            res = ws.alnse_core1(opt, b.seqs[:int(b.offs[4000])], b.offs[:4001])
            ctr = ws.counters()
            assert len(_oracle_py().compare(res, tiny.want([], 4000))) == 0
            assert ctr["d_text_seed"] > 0 and ctr["d_sa_seed"] > 0, ctr
        finally:
            ws.close()
    finally:
        b.ora.close(); b.base.close(); b.idx.destroy()


def test_a_walk_makes_the_same_fetches_wherever_it_runs(tiny, monkeypatch):
    """The seed stage's access counters of the refill case at 64 blocks and at the default grid are equal."""
    got = []
    for env in ({"SALT_GPU_NO_UNIQUE": "1", "SALT_GPU_WALK_BLOCKS": "64"}, {"SALT_GPU_NO_UNIQUE": "1"}):
        monkeypatch.delenv("SALT_GPU_WALK_BLOCKS", raising=False)
        ws = tiny.workspace(monkeypatch, env)
        try:
            _run(tiny, ws, [], counters=True)
            c = ws.counters()
            got.append({k: c[k] for k in SEED_CTRS})
        finally:
            ws.close()
    print(got)
    assert got[0] == got[1]
    assert got[0]["d_cocc_seed"] > 0 and got[0]["d_rocc_seed"] > 0
