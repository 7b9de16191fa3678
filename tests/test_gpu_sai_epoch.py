"""R seed rows that carry their call's epoch, and the R rows' context records in single end.

k_seed writes no R row any more: k_seed_walk stores the rows of the R walks that end alive with the call's epoch above the flag, and
every reader (k_light, k_light2, build_candidates) takes a row whose epoch is not the call's for a dead one (sai_r_row, salt_device.h).
The R context table (r_ctx) is built when an index is attached, so the single-end instantiations of build_candidates locate their R
rows through it.

Everything goes through the C ABI and is held against the CPU oracle, every field (oracle_py.compare), with no differing read allowed.

What makes a stale row show: a batch of reads cut from the genome verifies at none of the places another batch's rows point to, so
on such batches alone a reader without the epoch test would still give the oracle's rows.  Both batches of the stale-row tests
therefore hold, at the same read indices, PLANTED reads of three seeds (57 bases at k = 19) over one isolated SNP site:
  A: the alternative allele at the site and one substitution in each of the two other seeds.  Both C searches of those die, the C search
     of the seed over the site dies on the allele, its R search lives: the read's only hit comes through an R row (the oracle finds
     nothing with -v, which leaves the R searches out).  That row points 2 bases in front of the read (R_SHIFT below).
  B: the plain genome cut where A's row points, one substitution in EVERY seed: all six searches die and the oracle leaves the read
     unmapped, but at 3 mismatches it verifies gap-free where A's row of the same (read, strand, slot) points.
A reader that took A's row for a live one in call B maps that read.  Both facts about the planted reads are checked with the oracle
on the CPU before anything runs on the GPU."""
import copy
import os

import numpy as np
import pytest

from test_gpu_seed_walk import SEED_CTRS, _Bench, _mixed_genome, _mixed_reads, _oracle_py, _run

pytestmark = pytest.mark.gpu

N_CALL = 2000
PLANT_EVERY = 10                      # read indices 0, 10, 20 ... hold the planted reads: 200 of the 2 000
EPOCH_MAX = (1 << 24) - 1
K_MIXED = 21
UNMAPPED = 0xFFFFFFFF


def _revcomp(r):
    r = r[::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


R_SHIFT = 2          # a row of the R index gives the place 2 bases in front of the read's (the reference's positions of its local patterns,
                     # which the builder and the oracle keep): such a hit is found by the gapped pass, as the oracle's rows of batch A show


def _planted(genome, pos, mask, k, n, seed):
    """n triples (a, b, where a's R row points) of 3k-base reads over isolated two-allele SNP sites, as the module's docstring describes
    them.  Only sites whose alternative allele is the lower base code: the others' windows give no live row (the oracle check of the
    `ab` fixture is what holds this up, not this comment)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pos = np.asarray(pos).astype(np.int64)
    gap_l = np.diff(pos, prepend=-10 ** 9)
    gap_r = np.diff(pos, append=10 ** 9)
    ref = genome[pos].astype(np.int64)
    alt_lower = np.array([bin(int(m)).count("1") == 2 and (int(m) & ((1 << int(r)) - 1)) != 0 for m, r in zip(mask, ref)])
    ok = np.nonzero(alt_lower & (gap_l > 4 * k) & (gap_r > 4 * k) & (pos > 4 * k) & (pos < len(genome) - 4 * k))[0]
    assert len(ok) >= n, (len(ok), n)
    sites = rng.choice(ok, size=n, replace=False)
    out = []
    for i, si in enumerate(sites):
        p, m = int(pos[si]), int(mask[si])
        alt = [x for x in range(4) if (m >> x) & 1 and x != int(genome[p])][0]
        slot = i % 3
        start = p - (k * slot + 9)
        a = genome[start:start + 3 * k].copy()
        a[p - start] = alt
        b = genome[start - R_SHIFT:start - R_SHIFT + 3 * k].copy()     # the plain genome where a's row points
        for t in range(3):
            if t != slot:
                a[k * t + 9] = (a[k * t + 9] + 1) & 3
            b[k * t + 4] = (b[k * t + 4] + 1 + (i >> 1) % 3) & 3     # never the SNP site, which is base k * slot + 11 of b
        if i & 1:
            a, b = _revcomp(a), _revcomp(b)
        out.append((a, b, start - R_SHIFT))
    return out


def _batch(reads100, L, planted, which):
    """The batch's reads with every PLANT_EVERY-th one replaced by a planted read."""
    reads = [reads100[i * L:(i + 1) * L] for i in range(len(reads100) // L)]
    for j, pr in enumerate(planted):
        reads[j * PLANT_EVERY] = pr[which]
    offs = np.zeros(len(reads) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


@pytest.fixture(scope="module")
def tiny_wl(tmp_path_factory):
    from salt_amd import workload
    return workload.prepare("tiny", str(tmp_path_factory.mktemp("wl")))


@pytest.fixture(scope="module")
def ab(tiny_wl):
    """(bench of batch A, the same bench seen with batch B, indices of the planted reads): one attached index, the oracle's rows once."""
    from salt_amd import workload
    w = tiny_wl
    L, k = w["read_len"], 19
    genome, pos, mask = np.asarray(w["genome"]), np.asarray(w["snp_pos"]), np.asarray(w["snp_mask"])
    planted = _planted(genome, pos, mask, k, N_CALL // PLANT_EVERY, seed=31)
    ra = workload.make_reads(genome, pos, mask, N_CALL, L, seed=11)[0]                 # over the SNP sites, listed alleles
    rb = workload.make_reads(genome, pos[:0], mask[:0], N_CALL, L, seed=12)[0]         # the plain genome, at other places
    sa, oa = _batch(ra, L, planted, 0)
    sb, ob = _batch(rb, L, planted, 1)
    a = _Bench(w["prefix"], sa, oa)
    b = copy.copy(a)
    b.seqs, b.offs, b._want = sb, ob, {}
    idx = np.arange(0, N_CALL, PLANT_EVERY)
    # ---- on the CPU: A's planted reads are found through an R seed and through nothing else, B's are not found at all ----
    o = a.opt([])
    v = a.ora.align(a.ora.opt(l_overlap=o.l_overlap, max_seed=o.max_seed, max_locate=o.max_locate, seed_only_ref=1), sa, oa, n_threads=8)
    wa, wb = a.want([]), b.want([])
    through_r = (wa["pos"][idx] != UNMAPPED) & (v["pos"][idx] == UNMAPPED) & (wa["pos"][idx] == np.array([pr[2] for pr in planted], dtype=np.uint32))
    print("planted reads: %d of %d of A map through an R seed only; %d of B are mapped" % (through_r.sum(), len(idx), (wb["pos"][idx] != UNMAPPED).sum()))
    assert through_r.sum() >= len(idx) * 3 // 4, through_r.sum()
    assert (wb["pos"][idx[through_r]] == UNMAPPED).all()
    yield a, b, idx
    a.close()


def _same_rows(x, y):
    """Rows of two GPU calls, every field the oracle comparison looks at."""
    for f in ("pos", "strand", "n_diff", "is_gap", "mapq", "b0", "b1", "n_hits", "n_cigar"):
        assert np.array_equal(x[f], y[f]), f
    for s in range(2):
        for j in range(5):
            live = x["n_hits"][:, s] > j
            for f in ("pos", "n_diff", "is_gap"):
                assert np.array_equal(x["hits"][f][:, s, j][live], y["hits"][f][:, s, j][live]), (f, s, j)
    for i in np.nonzero(x["pos"] != UNMAPPED)[0]:
        n = int(x["n_cigar"][i])
        assert np.array_equal(x["cigar"][i][:n], y["cigar"][i][:n]), i


# ---- 1. stale R rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reader", ["k_light2", "k_light", "k_heavy"])
def test_rows_of_another_call_are_dead(ab, monkeypatch, reader):
    """A, B, A on one workspace: call B finds A's live R rows where its own R searches died and nobody wrote a dead row.  Each call equals
    the oracle and the rows a fresh workspace gives.  k_light2 reads the rows in the default path, k_light when the access counters
    are on, build_candidates (k_heavy) first when SALT_GPU_ALL_HEAVY=1 skips the light kernel."""
    a, b, idx = ab
    monkeypatch.delenv("SALT_GPU_ALL_HEAVY", raising=False)
    env = {"SALT_GPU_ALL_HEAVY": "1"} if reader == "k_heavy" else {}
    counters = reader == "k_light"
    ws = a.workspace(monkeypatch, env)
    try:
        got = [_run(x, ws, [], counters=counters).copy() for x in (a, b, a)]
    finally:
        ws.close()
    for x, g in ((a, got[0]), (b, got[1])):
        fresh = a.workspace(monkeypatch, env)
        try:
            _same_rows(g, _run(x, fresh, [], counters=counters))
        finally:
            fresh.close()
    _same_rows(got[0], got[2])
    assert (got[0]["pos"][idx] != UNMAPPED).sum() >= len(idx) * 3 // 4            # A's planted reads were found (through their R rows)
    assert (got[1]["pos"][idx] != UNMAPPED).sum() <= len(idx) // 4                 # B's were not (the oracle comparison has said so read by read)


# ---- 2. sizes and regrow --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(tiny_wl):
    from salt_amd import workload
    w = tiny_wl
    seqs, offs, _, _ = workload.make_reads(w["genome"], w["snp_pos"], w["snp_mask"], 20000, w["read_len"], seed=7)
    b = _Bench(w["prefix"], seqs, offs)
    yield b
    b.close()


def test_sizes_and_regrow(tiny, monkeypatch):
    """20 000, 3, 20 000 reads on one workspace: the short call leaves the long call's R rows in place behind its own three reads' and
    the third call finds them there.  Then -r 5: 17 seed slots a strand where the arrays were sized for 5, so both row arrays are
    allocated anew and the R rows zeroed before the call's kernels run."""
    ws = tiny.workspace(monkeypatch, {})
    try:
        for n in (20000, 3, 20000):
            _run(tiny, ws, [], n)
        _run(tiny, ws, ["-r", "5"])
        _run(tiny, ws, [])
    finally:
        ws.close()


# ---- 3. the epoch restarts -------------------------------------------------------------------------------------------------------------
def test_epoch_wrap(ab, monkeypatch):
    """SALT_GPU_SAI_EPOCH = 2^24 - 2: the calls run at epochs 2^24 - 2, 2^24 - 1 (the last one), 1 (the R rows zeroed in front of
    k_seed) and 2, alternating A and B."""
    a, b, idx = ab
    monkeypatch.delenv("SALT_GPU_ALL_HEAVY", raising=False)
    ws = a.workspace(monkeypatch, {"SALT_GPU_SAI_EPOCH": str(EPOCH_MAX - 1)})
    monkeypatch.delenv("SALT_GPU_SAI_EPOCH")
    try:
        for x, e in zip((a, b, a, b), (EPOCH_MAX - 1, EPOCH_MAX, 1, 2)):
            assert ws.epoch() == e, (ws.epoch(), e)
            _run(x, ws, [])
        assert ws.epoch() == 3
    finally:
        ws.close()


# ---- 4. single-end R contexts -----------------------------------------------------------------------------------------------------------
def _repeat_snp_index(tmp, k):
    """The mixed genome with a SNP at base 18 of every unit of its tandem repeat (copies 5 .. 294) beside 300 scattered ones, and reads
    from inside the repeat that carry the alternative alleles: the R search of a seed over such a site ends on an interval of some
    290 rows, the copies' contexts."""
    import salt_amd
    from salt_amd import workload
    genome, rep0, pa0 = _mixed_genome()
    rep1 = rep0 + 37 * 300
    p0, m0 = workload.make_snps(genome, 300, seed=5)
    keep = (p0 < rep0 - 2 * k) | (p0 >= rep1 + 2 * k)
    pr = rep0 + 37 * np.arange(5, 295, dtype=np.int64) + 18
    ref = genome[pr].astype(np.int64)
    mr = ((1 << ref) | (1 << ((ref + 1) & 3))).astype(np.uint8)
    pos = np.concatenate([p0[keep], pr])
    mask = np.concatenate([m0[keep], mr])
    order = np.argsort(pos)
    pos, mask = pos[order], mask[order]
    contigs, groups = workload.as_builder_input(genome, pos, mask)
    prefix = os.path.join(str(tmp), "idx%d" % k)
    salt_amd.idx_build_mem(contigs, groups, prefix, k, flags=salt_amd.IDX_NO_LP)
    seqs, offs = _mixed_reads(genome, rep0, pa0, k)
    reads = [seqs[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    rng = np.random.Generator(np.random.PCG64(99))
    alt = genome.copy()
    alt[pr] = (alt[pr] + 1) & 3
    first_rep = len(reads)
    for j in range(48):
        L = (100, 150, 63)[j % 3]
        p = rep0 + 37 * 10 + int(rng.integers(0, 37 * 270 - L))
        r = alt[p:p + L].copy()
        if j % 4 == 1:                                       # one alternative allele only
            r = genome[p:p + L].copy()
            q = pr[(pr >= p) & (pr < p + L)][0] - p
            r[q] = alt[p + q]
        if j & 1:
            r = _revcomp(r)
        reads.append(r)
    offs = np.zeros(len(reads) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return prefix, np.concatenate(reads).astype(np.uint8), offs, first_rep


HEAVY_CTRS = ("d_sa_heavy", "d_verify_heavy", "d_ctx_rows", "d_ctx_rejected")


def _r_ctx(aln):
    """(device pointer or None, bytes) of the R context table of a GpuAligner's index."""
    return aln.r_ctx()


def test_single_end_r_contexts(tmp_path, monkeypatch):
    """R intervals of more than 64 rows reach k_heavy, attached once with the R context table (the default now) and once without it
    (SALT_GPU_NO_RCTX=1): both equal the oracle at the default options and at -s 2 -m 200, where the locate cap bites inside an R
    interval.  The table changes which loads serve the rows and how many windows are verified, nothing else: more rows through
    context records, no more verified windows, the same suffix-array / R-position loads and the same seed stage."""
    prefix, seqs, offs, first_rep = _repeat_snp_index(tmp_path, K_MIXED)
    monkeypatch.delenv("SALT_GPU_NO_RCTX", raising=False)
    monkeypatch.delenv("SALT_GPU_ALL_HEAVY", raising=False)
    ctrs = {}
    want = None
    for no_rctx in (False, True):
        b = _Bench(prefix, seqs, offs, env={"SALT_GPU_NO_RCTX": "1"} if no_rctx else {})
        try:
            if want is None:
                # on the CPU: reads whose list of R rows is longer than 64 exist (one oracle call per read of the added ones)
                o = b.opt([])
                oo = b.ora.opt(l_overlap=o.l_overlap, max_seed=o.max_seed, max_locate=o.max_locate)
                n_sar = [b.ora.align(oo, seqs[offs[i]:offs[i + 1]], np.array([0, offs[i + 1] - offs[i]], dtype=np.uint32), counters=True)[1]["n_saR"]
                         for i in range(first_rep, len(offs) - 1)]
                print("R rows located per added read (oracle):", n_sar)
                assert sum(x > 64 for x in n_sar) >= 8, n_sar
                want = b._want
            b._want = want                                             # the oracle's rows once for both attachments
            p, nbytes = _r_ctx(b.base)
            assert (p is None) == no_rctx and (nbytes == 0) == no_rctx, (p, nbytes)
            for optargs in ([], ["-s", "2", "-m", "200"]):
                ws = b.workspace(monkeypatch, {})
                try:
                    _run(b, ws, optargs, counters=True)
                    c = ws.counters()
                    ctrs[(no_rctx, tuple(optargs))] = {k: int(c[k]) for k in SEED_CTRS + HEAVY_CTRS}
                    _run(b, ws, optargs)                               # and through k_light2
                finally:
                    ws.close()
        finally:
            b.close()
    for optargs in ((), ("-s", "2", "-m", "200")):
        w, wo = ctrs[(False, optargs)], ctrs[(True, optargs)]
        print(optargs, "with r_ctx", w, "without", wo)
        assert w["d_ctx_rows"] > wo["d_ctx_rows"]
        assert w["d_verify_heavy"] <= wo["d_verify_heavy"]
        assert w["d_sa_heavy"] == wo["d_sa_heavy"]
        for k in SEED_CTRS:
            assert w[k] == wo[k], k


# ---- 5. paired end on an index that has its table from attach --------------------------------------------------------------------------
def test_paired_end_keeps_the_table_of_attach(tiny_wl, monkeypatch):
    """2 000 pairs of 2 x 150 bases as the benchmark's paired-end leg makes them: salt_gpu_index_set_pac finds the R context table in
    place and builds no second one (the same device pointer before and after), and the mates equal the oracle's."""
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
    monkeypatch.delenv("SALT_GPU_NO_RCTX", raising=False)
    idx = salt_amd.Index.reload(w["prefix"])
    opt, _ = salt_amd.AlnOpt.from_argv(["-p", "-a", "250", "-b", "550"], idx.l_seed)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=len(offs) - 1, max_bases=int(offs[-1]) + 64)
    try:
        before = _r_ctx(aln)
        assert before[0] is not None and before[1] > 0, before
        res = aln.alnpe_core1(opt, idx, seqs, offs)
        assert _r_ctx(aln) == before
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
    assert (res["pos"] != UNMAPPED).mean() > 0.9
