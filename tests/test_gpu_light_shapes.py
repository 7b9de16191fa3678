"""The four launch shapes of the light pass on their smallest batches.

launch_light picks one of k_light2<2, 4> (reads up to 120 bases, at most 8 seed slots a strand: the default), k_light2<1, 4>
(SALT_GPU_L2_WAVES=1), k_light2<2, 8> (reads up to 248 bases) and k_light (SALT_GPU_NO_LIGHT2=1, and whatever the others do not take).
All four are one body (light_read in salt_align.hip) at two lane-group widths, so all four are held to the same rows here: every field
against the CPU oracle (oracle_py.compare, no differing read allowed) and against the rows of the default shape.

The switches are read once per process, so a shape runs in a child process of its own (this file run as a script), one after another,
each under a time limit.  The genome is lambda's contig A with a planted block of 100 exact copies of a 150-base unit behind it.

Batches per read set: the first 1, 2, 3, 5 and 257 ordinary reads (an idle second half-wave, an idle last wave, many workgroups), and
one batch of 16 that holds, next to ordinary reads, each of these kinds at both parities of the read index (once in the lower and once
in the upper half of a wave, beside a neighbour of another kind, which takes another path):
  all-N        no seed at all.  At 100 bases the N limit of single-end reads (200) cannot be passed, the read goes on without seeds and is
               queued; in the 150-base set it is 230 bases long and passes the limit: its half-wave leaves early (skipped), the other goes on
  short        shorter than the seed: queued at once
  nowhere      random bases, no gap-free hit: queued
  repeat       cut from the planted block: every seed enumerates 100 rows (more than the 64 a list may hold here): queued
  one-sub      a genome cut with one substitution: finished in the light pass
What the oracle makes of these reads (unmapped / mapped, and the seed count of the repeat read in the genome text) is checked on the
CPU before anything runs on the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 19
UNMAPPED = 0xFFFFFFFF
SIZES = (1, 2, 3, 5, 257)
# read set -> (read length, seed stride l_overlap, words of a strand the shape allows, length of the all-N read)
SETS = {"r100": (100, K, 15, 100), "r150": (150, 31, 31, 230)}
# shape -> (environment of the child, read sets)
SHAPES = {"l2_waves_1": ({"SALT_GPU_L2_WAVES": "1"}, ("r100",)), "no_light2": ({"SALT_GPU_NO_LIGHT2": "1"}, ("r100", "r150"))}
CHILD_LIMIT_S = 120


def _revcomp(r):
    r = r[::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


def _pack(reads):
    offs = np.zeros(len(reads) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


def _genome():
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
    rng = np.random.Generator(np.random.PCG64(514))
    flank = lambda: rng.integers(0, 4, size=400).astype(np.uint8)
    block = np.tile(rng.integers(0, 4, size=150).astype(np.uint8), 100)
    rep0 = len(lam) + 400
    return np.concatenate([lam, flank(), block, flank()]), len(lam), rep0, len(block)


def _batches(genome, n_lam, rep0, n_rep, name):
    """name -> list of (seqs, offs) and, for the batch of 16, {kind: the two read indices}"""
    L, _, _, n_len = SETS[name]
    rng = np.random.Generator(np.random.PCG64(L))

    def cut(lo, hi, subs):
        p = int(rng.integers(lo, hi - L))
        r = genome[p:p + L].copy()
        for q in rng.choice(L, size=subs, replace=False):
            r[q] = (r[q] + 1 + int(rng.integers(0, 3))) & 3
        return r if rng.random() < 0.5 else _revcomp(r)

    ordinary = [cut(0, n_lam, int(rng.integers(0, 3))) for _ in range(SIZES[-1])]
    out = [_pack(ordinary[:n]) for n in SIZES]
    kinds = {"all_n": lambda: np.full(n_len, 4, dtype=np.uint8), "short": lambda: cut(0, n_lam, 0)[:K - 7],
             "nowhere": lambda: rng.integers(0, 4, size=L).astype(np.uint8), "repeat": lambda: cut(rep0, rep0 + n_rep, 0),
             "one_sub": lambda: cut(0, n_lam, 1)}
    # kind j at read 2j and again at read 2(j + 1) + 1 (mod 10): each kind at both parities, the two reads of a wave of different kinds
    special, where = [cut(0, n_lam, 0) for _ in range(16)], {}
    for j, k in enumerate(kinds):
        where[k] = [2 * j, (2 * j + 3) % 10]
        for i in where[k]:
            special[i] = kinds[k]()
    assert all(sorted(x % 2 for x in v) == [0, 1] for v in where.values()) and len({i for v in where.values() for i in v}) == 10, where
    out.append(_pack(special))
    return out, where


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The index, the batches of both read sets, the oracle's rows for them (with the CPU checks of what the batches are), and the
    rows of the default shape."""
    import salt_amd
    from salt_amd import workload
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    tmp = tmp_path_factory.mktemp("light_shapes")
    genome, n_lam, rep0, n_rep = _genome()
    pos, mask = workload.make_snps(genome[:n_lam], 200, seed=9)
    contigs, groups = workload.as_builder_input(genome, pos, mask)
    prefix = str(tmp / "idx")
    salt_amd.idx_build_mem(contigs, groups, prefix, K, flags=salt_amd.IDX_NO_LP)
    text = bytes(genome)
    ora = oracle_py.Oracle(prefix)
    w = {"prefix": prefix, "tmp": str(tmp), "sets": {}}
    for name, (L, stride, words, n_len) in SETS.items():
        batches, where = _batches(genome, n_lam, rep0, n_rep, name)
        oo = ora.opt(l_overlap=stride)
        want = []
        for seqs, offs in batches:
            lens = np.diff(offs.astype(np.int64))
            # launch_light's condition for the shape: seed slots a strand (salt_gpu.hip: (max_len - k) / stride + 1) and words a strand
            assert (int(lens.max()) - K) // stride + 1 <= 8 and (int(lens.max()) + 7) // 8 <= words, (name, lens.max())
            want.append(ora.align(oo, seqs, offs, n_threads=4))
        assert (want[-2]["pos"] != UNMAPPED).mean() > 0.95                   # the ordinary reads are ordinary
        seqs, offs = batches[-1]
        sp = want[-1]
        for i in where["all_n"] + where["short"] + where["nowhere"]:
            assert sp["pos"][i] == UNMAPPED, (name, i)
        for i in where["repeat"]:
            r = seqs[offs[i]:offs[i + 1]]
            assert max(text.count(bytes(x[:K])) for x in (r, _revcomp(r))) > 64 and sp["pos"][i] != UNMAPPED, (name, i)
        for i in where["one_sub"]:
            assert sp["pos"][i] != UNMAPPED and sp["is_gap"][i] == 0 and sp["n_diff"][i] <= 1, (name, i)
        np.savez(os.path.join(w["tmp"], name + ".npz"), **{"s%d" % b: s for b, (s, o) in enumerate(batches)}, **{"o%d" % b: o for b, (s, o) in enumerate(batches)})
        w["sets"][name] = (batches, where, want)
    ora.close()
    w["default"] = _child(w, "default", {}, tuple(SETS))
    return w


def _child(w, tag, env, sets):
    """One process for one shape: the batches of `sets` through the C ABI.  name -> list of (rows, ids of the reads the light pass queued)"""
    import salt_amd
    out = os.path.join(w["tmp"], tag)
    e = {k: v for k, v in os.environ.items() if k not in ("SALT_GPU_L2_WAVES", "SALT_GPU_NO_LIGHT2")}
    e["SALT_GPU_LKT_LEN"] = os.environ.get("SALT_GPU_LKT_LEN", "14")         # a 4 GiB W-mer table a child instead of 64 GiB: the seeds are not the subject
    p = subprocess.run([sys.executable, os.path.abspath(__file__), w["prefix"], w["tmp"], out] + list(sets), env=dict(e, **env),
                       capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    assert p.returncode == 0, (tag, p.returncode, p.stdout[-400:], p.stderr[-800:])
    res = {}
    for name in sets:
        z = np.load(out + "_" + name + ".npz")
        res[name] = [(z["r%d" % b].view(salt_amd.RESULT_DTYPE), z["q%d" % b]) for b in range(len(SIZES) + 1)]
    return res


def _hold(w, got, name, tag):
    import oracle_py
    import salt_amd
    batches, where, want = w["sets"][name]
    for b, (rows, queued) in enumerate(got[name]):
        bad = oracle_py.compare(rows, want[b])
        assert len(bad) == 0, (tag, name, b, bad[:8])
        ref = w["default"][name][b][0]
        mapped = rows["pos"] != UNMAPPED
        for f in ("pos", "strand", "n_diff", "is_gap", "mapq", "b0", "b1", "n_cigar", "skipped", "seq_start", "seq_end"):
            assert np.array_equal(rows[f][mapped | (f in ("pos", "skipped"))], ref[f][mapped | (f in ("pos", "skipped"))]), (tag, name, b, f)
        assert np.array_equal(rows["n_hits"][mapped], ref["n_hits"][mapped]), (tag, name, b)
        for i in np.nonzero(mapped)[0]:
            for s in range(2):
                n = int(rows["n_hits"][i, s])
                assert rows["hits"][i, s, :n].tobytes() == ref["hits"][i, s, :n].tobytes(), (tag, name, b, i)
            n = int(rows["n_cigar"][i])
            assert np.array_equal(rows["cigar"][i][:n], ref["cigar"][i][:n]), (tag, name, b, i)
    rows, queued = got[name][-1]
    n_long = SETS[name][3] > 200
    for i in where["all_n"]:                   # past the N limit: left at once and not queued, unless it is too long for the kernel (k_light: 160)
        assert bool(rows["skipped"][i]) == n_long and (i in queued) == (not n_long or tag == "no_light2"), (tag, name, i)
    for k in ("short", "nowhere", "repeat"):
        assert all(i in queued for i in where[k]), (tag, name, k, queued)
    assert not any(i in queued for i in where["one_sub"]), (tag, name, queued)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SETS))
def test_gpu_light2_default_shapes_equal_the_oracle(world, name):
    """k_light2<2, 4> on the 100-base batches, k_light2<2, 8> on the 150-base ones (no switch set)."""
    _hold(world, world["default"], name, "default")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gpu_light_switched_shapes_equal_the_oracle_and_the_default_shape(world, shape):
    """k_light2<1, 4> (SALT_GPU_L2_WAVES=1) on the 100-base batches; k_light (SALT_GPU_NO_LIGHT2=1) on both read sets."""
    env, sets = SHAPES[shape]
    got = _child(world, shape, env, sets)
    for name in sets:
        _hold(world, got, name, shape)


def _main(prefix, tmp, out, sets):
    sys.path.insert(0, ROOT)
    import salt_amd
    idx = salt_amd.Index.reload(prefix, rebuild_lkt=False)
    aln = salt_amd.GpuAligner(idx, device=0, max_reads=SIZES[-1], max_bases=SIZES[-1] * 256)
    for name in sets:
        z = np.load(os.path.join(tmp, name + ".npz"))
        opt = salt_amd.AlnOpt(l_seed=K, l_overlap=SETS[name][1])
        res = {}
        for b in range(len(SIZES) + 1):
            res["r%d" % b] = aln.alnse_core1(opt, z["s%d" % b], z["o%d" % b]).copy().view(np.uint8)
            res["q%d" % b] = np.sort(aln.heavy_reads())
        np.savez(out + "_" + name + ".npz", **res)
    aln.close()
    idx.destroy()


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:])
