"""The light pass with four reads a wave (k_light4, 16 lanes a read) and the retry launch behind it (k_light_retry).

launch_light takes the quarter shape for reads of at most 120 bases with at most 4 seed slots a strand; SALT_GPU_NO_LIGHT4=1 restores
the half-wave shape, SALT_GPU_L4_WAVES (1, 2, 4) sets the waves of a workgroup.  A read one of whose four seed lists enumerates more
than L4_ROWS = 16 suffix-array rows (and none more than 64) does not fit a quarter's record: the quarter pushes it to a retry list
and the half-wave body finishes it; above 64 rows the read goes to k_heavy as before.  Every read is finished by exactly one of the
three, and k_heavy receives what it received before.

Every row here is held to the CPU oracle (oracle_py.compare, no differing read) and to the rows of the same batch under
SALT_GPU_NO_LIGHT4=1; the reads queued for k_heavy must be the same reads, and the retry count (queue_counts()[4]) the number of
reads the CPU put into the retry class.  The switches are read once per process, so each setting runs in a child process of its own
(this file as a script), one after another, each under a time limit.

Index: k = 21 over lambda's contig A with 300 SNP sites, and behind it exact copies of 150-base units (1, 2, 4, 8, 14, 16 and 17
copies), dispersed in random order between random flanks of 200 bases.  Seeds at stride 21, so a read of 100 bases has 4 seed slots a
strand.  A read cut from inside a unit with c copies has 4 seeds of c rows each: a C list of 4c rows; a read that starts 21 bases in
front of a copy's end has one seed of c rows and three of one row: c + 3.

The batch "kinds" holds each kind of read below at every quarter position 0..3 of a wave, the four reads of a wave all of different
kinds (21 kinds, 84 reads, and 4 ordinary ones: a batch of 32 cannot hold them):
  all_n      100 N: below the N limit, goes on without seeds, queued for k_heavy
  short      shorter than k: queued
  nowhere    random bases: no hit, queued
  one_sub    a cut from lambda with one substitution
  tot4, tot5     lists of 4 and of 5 rows: the small / general boundary of a quarter (4 rows a list: one lane a row)
  tot16, tot17   the quarter / retry boundary
  tot64, tot68   the light / heavy boundary
  alt        a cut over listed SNPs in two or more of its seeds, with their alternative alleles: those seeds have rows in the R lists
             only, the others in the C lists; finished in the light pass
  alt_only   the same with a substitution in each seed without a site (two at the most): the C lists are empty, only the R lists
             hold its rows.  The oracle finds no gap-free hit for such a read, so it is queued all the same
  and the reverse-strand twin of each of the last nine (rc_...).
The batch "mixed" is the same 88 reads and four all-N reads of 230 bases, one at every quarter position: the batch is longer than the
quarter shape allows, so nothing may reach the retry list.  The "edge" batches (ordinary reads and cuts from the unit with 8 copies: a
list of 32 rows, or 40 with 5 seeds) sit on the shape's limits: 104 bases (4 seed slots: quarter) and 105 (5: half-wave) at stride 21,
120 bases (15 words a strand: quarter) and 121 (16: half-wave) at stride 33; which shape ran shows in the retry count.
What the reads are (row totals by counting seeds in the genome text, what the oracle makes of each kind) is checked on the CPU before
anything runs on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 21
L4_ROWS = 16
UNMAPPED = 0xFFFFFFFF
SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 257)
COPIES = (1, 2, 4, 8, 14, 16, 17)
UNIT, FLANK = 150, 200
# batch -> (read length of its cuts, seed stride, quarter shape expected)
EDGES = {"edge104": (104, 21, True), "edge105": (105, 21, False), "edge120": (120, 33, True), "edge121": (121, 33, False)}
CHILD_LIMIT_S = 120


def _revcomp(r):
    r = r[::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


def _pack(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


def _genome():
    """lambda's contig A, then the copies of the units in random order, a random flank in front of each and one behind the last.
    Returns the genome, lambda's length and {copies: start of every copy}."""
    from conftest import LAMBDA
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    seq, n_contigs = [], 0
    with open(os.path.join(LAMBDA, "genome.fa")) as f:
        for line in f:
            if line.startswith(">"):
                n_contigs += 1
                if n_contigs > 1:
                    break
                continue
            seq.append(line.strip().upper())
    lam = np.array([code[c] for c in "".join(seq)], dtype=np.uint8)
    rng = np.random.Generator(np.random.PCG64(1604))
    units = {c: rng.integers(0, 4, size=UNIT).astype(np.uint8) for c in COPIES}
    order = rng.permutation(np.array([c for c in COPIES for _ in range(c)]))
    parts, at, n = [lam], {c: [] for c in COPIES}, len(lam)
    for c in order:
        parts.append(rng.integers(0, 4, size=FLANK).astype(np.uint8))
        n += FLANK
        at[int(c)].append(n)
        parts.append(units[int(c)])
        n += UNIT
    parts.append(rng.integers(0, 4, size=FLANK).astype(np.uint8))
    return np.concatenate(parts), len(lam), at


def _count(text, seed):
    n, i = 0, text.find(seed)
    while i >= 0:
        n, i = n + 1, text.find(seed, i + 1)
    return n


def _c_rows(text, r, stride):
    """rows of the two C lists of read r (forward, reverse): the occurrences of its seeds in the genome text"""
    if len(r) < K:
        return 0, 0
    spr = (len(r) - K) // stride + 1
    return tuple(sum(_count(text, bytes(x[stride * i:stride * i + K])) for i in range(spr) if (x[stride * i:stride * i + K] < 4).all())
                 for x in (r, _revcomp(r)))


def _batches(genome, n_lam, at, pos, mask):
    """name -> (seqs, offs); and for "kinds": {kind: its four read indices}"""
    rng = np.random.Generator(np.random.PCG64(16))
    site = np.zeros(len(genome), dtype=np.uint8)
    site[pos] = mask

    def lam_cut(L, subs):
        while True:
            p = int(rng.integers(0, n_lam - L))
            if not site[p:p + L].any():
                break
        r = genome[p:p + L].copy()
        for q in rng.choice(L, size=subs, replace=False):
            r[q] = (r[q] + 1 + int(rng.integers(0, 3))) & 3
        return r

    def ordinary(L):
        p = int(rng.integers(0, n_lam - L))
        r = genome[p:p + L].copy()
        for q in rng.choice(L, size=int(rng.integers(0, 3)), replace=False):
            r[q] = (r[q] + 1 + int(rng.integers(0, 3))) & 3
        return r if rng.random() < 0.5 else _revcomp(r)

    def inside(c, L=100):                                     # wholly inside a copy: every seed has c rows
        p = at[c][int(rng.integers(0, c))] + int(rng.integers(0, UNIT - L + 1))
        return genome[p:p + L].copy()

    def tail(c):                                              # the first seed is the copy's last 21 bases, the others lie in the flank
        p = at[c][int(rng.integers(0, c))] + UNIT - K
        return genome[p:p + 100].copy()

    def alt(only):
        while True:
            p = int(pos[int(rng.integers(0, len(pos)))]) - int(rng.integers(0, 4 * K))
            if p < 0 or p + 100 > n_lam:
                continue
            sites = np.nonzero(site[p:p + 100])[0]
            slots = {int(q) // K for q in sites if q < 4 * K}
            if len(slots) < 2:
                continue                                      # sites in two seeds at least: at most two substitutions
            r = genome[p:p + 100].copy()
            for q in sites:
                r[q] = [a for a in range(4) if (int(site[p + q]) >> a) & 1 and a != int(genome[p + q])][0]
            for i in (set(range(4)) - slots if only else ()):
                q = K * i + int(rng.integers(0, K))
                r[q] = (r[q] + 1 + int(rng.integers(0, 3))) & 3
            return r

    base = {"one_sub": lambda: lam_cut(100, 1), "tot4": lambda: inside(1), "tot5": lambda: tail(2), "tot16": lambda: inside(4),
            "tot17": lambda: tail(14), "tot64": lambda: inside(16), "tot68": lambda: inside(17), "alt": lambda: alt(False), "alt_only": lambda: alt(True)}
    kinds = {"all_n": lambda: np.full(100, 4, dtype=np.uint8), "short": lambda: lam_cut(100, 0)[:K - 7],
             "nowhere": lambda: rng.integers(0, 4, size=100).astype(np.uint8)}
    kinds.update(base)
    kinds.update({"rc_" + k: (lambda f=f: _revcomp(f())) for k, f in base.items()})
    names = list(kinds)
    assert len(names) == 21
    # wave w, quarter q holds kind (w + 5 q) mod 21: every kind at every quarter position, four different kinds a wave
    special, where = [], {k: [] for k in names}
    for w in range(21):
        for q in range(4):
            k = names[(w + 5 * q) % 21]
            where[k].append(len(special))
            special.append(kinds[k]())
    assert all(sorted(i % 4 for i in v) == [0, 1, 2, 3] for v in where.values())
    special += [ordinary(100) for _ in range(4)]
    pool = [ordinary(100) for _ in range(SIZES[-1])]
    out = {"n%d" % n: _pack(pool[:n]) for n in SIZES}
    out["kinds"] = _pack(special)
    out["mixed"] = _pack(special + [np.full(230, 4, dtype=np.uint8) for _ in range(4)])
    for name, (L, stride, _) in EDGES.items():
        rs = [ordinary(L) for _ in range(13)]
        for i in (0, 5, 6, 11):                               # the four quarter positions
            rs[i] = inside(8, L) if i != 6 else _revcomp(inside(8, L))
        out[name] = _pack(rs)
    return out, where


def _stride(name):
    return EDGES[name][1] if name in EDGES else K


def _retry_class(text, seqs, offs, stride):
    """reads of a quarter-shaped batch that go to the retry list, by their C lists (the planted units carry no SNP site, and a read
    from lambda has a few rows a list)"""
    n = 0
    for i in range(len(offs) - 1):
        r = seqs[offs[i]:offs[i + 1]]
        n += L4_ROWS < max(_c_rows(text, r, stride)) <= 64
    return n


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The index, the batches, the oracle's rows for them, the CPU checks of what the batches are, and the rows of the NO_LIGHT4 child."""
    import salt_amd
    from salt_amd import workload
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    tmp = tmp_path_factory.mktemp("light_quarter")
    genome, n_lam, at = _genome()
    pos, mask = workload.make_snps(genome[:n_lam], 300, seed=16)
    contigs, groups = workload.as_builder_input(genome, pos, mask)
    prefix = str(tmp / "idx")
    salt_amd.idx_build_mem(contigs, groups, prefix, K, flags=salt_amd.IDX_NO_LP)
    text = bytes(genome)
    batches, where = _batches(genome, n_lam, at, pos, mask)
    ora = oracle_py.Oracle(prefix)
    want, retry = {}, {}
    for name, (seqs, offs) in batches.items():
        stride = _stride(name)
        lens = np.diff(offs.astype(np.int64))
        quarter = (int(lens.max()) - K) // stride + 1 <= 4 and (int(lens.max()) + 7) // 8 <= 15      # launch_light's condition
        assert quarter == (EDGES[name][2] if name in EDGES else name != "mixed"), name
        retry[name] = _retry_class(text, seqs, offs, stride) if quarter else 0
        want[name] = ora.align(ora.opt(l_overlap=stride), seqs, offs, n_threads=4)
    ora.close()
    # ---- what the reads are, on the CPU ----
    assert (want["n257"]["pos"] != UNMAPPED).mean() > 0.95
    seqs, offs = batches["kinds"]
    sp = want["kinds"]
    rows = lambda i: _c_rows(text, seqs[offs[i]:offs[i + 1]], K)
    for k in ("all_n", "short", "nowhere"):
        for i in where[k]:
            assert sp["pos"][i] == UNMAPPED and rows(i) == (0, 0), (k, i)
    for k, n in (("tot4", 4), ("tot5", 5), ("tot16", 16), ("tot17", 17), ("tot64", 64), ("tot68", 68)):
        for i in where[k]:
            assert rows(i) == (n, 0) and sp["pos"][i] != UNMAPPED and sp["n_diff"][i] == 0 and sp["is_gap"][i] == 0, (k, i, rows(i))
        for i in where["rc_" + k]:
            assert rows(i) == (0, n) and sp["pos"][i] != UNMAPPED and sp["n_diff"][i] == 0 and sp["is_gap"][i] == 0, (k, i, rows(i))
    for i in where["one_sub"] + where["rc_one_sub"]:
        assert sp["pos"][i] != UNMAPPED and sp["is_gap"][i] == 0 and sp["n_diff"][i] == 1 and max(rows(i)) in (3, 4), i
    for i in where["alt"] + where["rc_alt"]:                    # two of its seeds at least are not in the text; no difference all the same
        assert max(rows(i)) <= 2 and sp["pos"][i] != UNMAPPED and sp["is_gap"][i] == 0 and sp["n_diff"][i] == 0, (i, rows(i), sp["n_diff"][i])
    for i in where["alt_only"] + where["rc_alt_only"]:          # no seed of it in the text; no gap-free hit
        assert rows(i) == (0, 0) and (sp["pos"][i] == UNMAPPED or sp["is_gap"][i] == 1), (i, sp["n_diff"][i])
    assert retry["kinds"] == 16 and retry["mixed"] == 0                   # tot17, tot64 and their twins at four positions each
    assert all(retry[k] == (4 if EDGES[k][2] else 0) for k in EDGES) and all(retry["n%d" % n] == 0 for n in SIZES), retry
    np.savez(os.path.join(str(tmp), "batches.npz"), **{"s_" + k: s for k, (s, o) in batches.items()}, **{"o_" + k: o for k, (s, o) in batches.items()})
    w = {"prefix": prefix, "tmp": str(tmp), "batches": batches, "where": where, "want": want, "retry": retry}
    w["no_light4"] = _child(w, "no_light4", {"SALT_GPU_NO_LIGHT4": "1"}, list(batches))
    return w


def _child(w, tag, env, names):
    """One process for one setting: the batches `names` through the C ABI.  name -> (rows, ids of the reads queued for k_heavy, retry count)"""
    import salt_amd
    out = os.path.join(w["tmp"], tag + ".npz")
    e = {k: v for k, v in os.environ.items() if k not in ("SALT_GPU_L2_WAVES", "SALT_GPU_NO_LIGHT2", "SALT_GPU_NO_LIGHT4", "SALT_GPU_L4_WAVES")}
    e["SALT_GPU_LKT_LEN"] = os.environ.get("SALT_GPU_LKT_LEN", "14")         # a small W-mer table: the seeds are not the subject
    p = subprocess.run([sys.executable, os.path.abspath(__file__), w["prefix"], w["tmp"], out] + list(names), env=dict(e, **env),
                       capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    assert p.returncode == 0, (tag, p.returncode, p.stdout[-400:], p.stderr[-800:])
    z = np.load(out)
    return {k: (z["r_" + k].view(salt_amd.RESULT_DTYPE), z["q_" + k], int(z["t_" + k])) for k in names}


def _hold(w, got, tag):
    import oracle_py
    for name, (rows, queued, n_retry) in got.items():
        bad = oracle_py.compare(rows, w["want"][name])
        assert len(bad) == 0, (tag, name, bad[:8])
        ref, ref_queued, ref_retry = w["no_light4"][name]
        assert ref_retry == 0, (name, ref_retry)
        assert np.array_equal(queued, ref_queued), (tag, name, queued, ref_queued)     # k_heavy receives the same reads
        want_retry = 0 if tag == "no_light4" else w["retry"][name]                     # the half-wave shape leaves nothing to a retry
        assert n_retry == want_retry, (tag, name, n_retry, want_retry)
        mapped = rows["pos"] != UNMAPPED
        for f in ("pos", "strand", "n_diff", "is_gap", "mapq", "b0", "b1", "n_cigar", "skipped", "seq_start", "seq_end"):
            assert np.array_equal(rows[f][mapped | (f in ("pos", "skipped"))], ref[f][mapped | (f in ("pos", "skipped"))]), (tag, name, f)
        assert np.array_equal(rows["n_hits"][mapped], ref["n_hits"][mapped]), (tag, name)
        for i in np.nonzero(mapped)[0]:
            for s in range(2):
                n = int(rows["n_hits"][i, s])
                assert rows["hits"][i, s, :n].tobytes() == ref["hits"][i, s, :n].tobytes(), (tag, name, i)
            n = int(rows["n_cigar"][i])
            assert np.array_equal(rows["cigar"][i][:n], ref["cigar"][i][:n]), (tag, name, i)
    if "kinds" in got:
        queued = got["kinds"][1]
        for k, v in w["where"].items():                                                # who finished which kind
            heavy = k in ("all_n", "short", "nowhere", "tot68", "rc_tot68", "alt_only", "rc_alt_only")
            assert all((i in queued) == heavy for i in v), (tag, k, queued)


@pytest.mark.gpu
def test_gpu_light_half_wave_rows_equal_the_oracle(world):
    """SALT_GPU_NO_LIGHT4=1, the rows every other setting is compared with: against the oracle, nothing on the retry list."""
    _hold(world, world["no_light4"], "no_light4")


@pytest.mark.gpu
def test_gpu_light_quarter_equals_the_oracle_and_the_half_wave_shape(world):
    """No switch set: k_light4<2> and k_light_retry on every batch -- sizes 1 .. 9 and 257 (idle quarters, an idle second wave, many
    workgroups), the kinds, the mixed-length batch (not eligible) and the four batches on the shape's limits."""
    got = _child(world, "default", {}, list(world["batches"]))
    assert got["kinds"][2] > 0
    _hold(world, got, "default")


@pytest.mark.gpu
@pytest.mark.parametrize("waves", ["1", "4"])
def test_gpu_light_quarter_workgroups_of_one_and_four_waves(world, waves):
    """SALT_GPU_L4_WAVES=1 / 4 on the batch of kinds."""
    got = _child(world, "l4_waves_" + waves, {"SALT_GPU_L4_WAVES": waves}, ["kinds"])
    assert got["kinds"][2] > 0
    _hold(world, got, "l4_waves_" + waves)


def _main(prefix, tmp, out, names):
    sys.path.insert(0, ROOT)
    import salt_amd
    z = np.load(os.path.join(tmp, "batches.npz"))
    idx = salt_amd.Index.reload(prefix, rebuild_lkt=False)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=SIZES[-1], max_bases=SIZES[-1] * 256)
    res = {}
    for name in names:
        opt = salt_amd.AlnOpt(l_seed=K, l_overlap=_stride(name))
        res["r_" + name] = aln.alnse_core1(opt, z["s_" + name], z["o_" + name]).copy().view(np.uint8)
        res["q_" + name] = np.sort(aln.heavy_reads())
        res["t_" + name] = np.uint32(aln.queue_counts()[4])
    np.savez(out, **res)
    aln.close()
    idx.destroy()


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:])
