"""The context record (salt_amd/csrc/salt_ctx_record.h) run on the host by tools/ctx_model.cc, with the functions the kernels use:
whenever a record rejects a candidate window, the oracle's masked Hamming count of the WHOLE window (so_ed_mismatch(..., 3)) is -1.
Zero false rejections, for every geometry of the short list the record was chosen from, reads of 100 and 150 bases, seed lengths 21
and 19, every seed offset 0 .. L - k, windows at both ends of the genome; and the filter is not vacuous.  (The kernels themselves:
test_gpu_ctx_geometry.py, test_gpu_parity.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

# name -> (n_front, a_start as (seed lengths, extra bases), n_behind, bits of side A's special-site count)
GEOMETRIES = {
    "default": None,                                  # what the header defines: (9, 2 k, 37), 2 + 2 bits
    "f23_a1k_b23": (23, (1, 0), 23, 2),               # the symmetric record the default replaced
    "f9_a2k8_b37": (9, (2, 8), 37, 3),
    "f9_a3k_b37": (9, (3, 0), 37, 3),
    "f9_a2k_b37": (9, (2, 0), 37, 3),
    "f12_a3k_b34": (12, (3, 0), 34, 3),
    "f9_a3k_b37_ns22": (9, (3, 0), 37, 2),
}
# Share of the (window, seed offset) pairs with more than 3 mismatches that the record rejects on the inputs below, as observed when the
# geometries were written; the test asks for that less a fifth, and for one half at the least.  Seed offsets are uniform here, which
# favours the symmetric record; the located rows of a real run are not (tools/ctx_geometry_model.py).
_OBSERVED = {"default": 0.698, "f23_a1k_b23": 0.780, "f9_a2k8_b37": 0.660, "f9_a3k_b37": 0.619, "f9_a2k_b37": 0.687, "f12_a3k_b34": 0.636,
             "f9_a3k_b37_ns22": 0.637}


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctxmodel")
    exes = {}
    for name, g in GEOMETRIES.items():
        defs = [] if g is None else ["-DCTX_N_FRONT=%d" % g[0], "-DCTX_A_SEEDS=%d" % g[1][0], "-DCTX_A_EXTRA=%d" % g[1][1], "-DCTX_NS_BITS_A=%d" % g[3]]
        exes[name] = str(d / ("ctx_model_" + name))
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + defs + ["-o", exes[name], os.path.join(ROOT, "tools", "ctx_model.cc")], check=True)
    return exes


def make_genome(rng, snp_every):
    """Random flanks around 40 copies of a 300-base family at 10 % divergence (so that a read has near-miss windows as well as its own
    and random ones), one SNP per `snp_every` bases with the genome base listed, three N runs (mask 15: everything matches)."""
    fam = rng.integers(0, 4, 300).astype(np.uint8)
    copies = np.tile(fam, 40)
    m = rng.random(len(copies)) < 0.10
    copies[m] = (copies[m] + rng.integers(1, 4, int(m.sum()))) & 3
    genome = np.concatenate([rng.integers(0, 4, 1500).astype(np.uint8), copies, rng.integers(0, 4, 1500).astype(np.uint8)])
    G = len(genome)
    mask = (1 << genome).astype(np.uint8)
    pos = rng.choice(G, G // snp_every, replace=False)
    mask[pos] |= (1 << ((genome[pos] + rng.integers(1, 4, len(pos))) & 3)).astype(np.uint8)
    tri = pos[rng.random(len(pos)) < 0.1]
    mask[tri] |= (1 << ((genome[tri] + rng.integers(1, 4, len(tri))) & 3)).astype(np.uint8)
    for start, n in ((40, 12), (G // 2, 30), (G - 70, 8)):
        mask[start:start + n] = 15
    return genome, mask


def make_windows(rng, genome, mask, L):
    """(pos, read) pairs: reads taken at `src` with a random listed allele at every special site, 0 .. 8 substitutions and sometimes N,
    each set against its own position, against the same offset in another copy of the family, and against a random position."""
    G = len(genome)
    src = np.concatenate([np.arange(0, 31, 3), np.arange(G - L - 30, G - L + 1, 3), rng.integers(0, G - L, 60), 1500 + rng.integers(0, 300 * 40 - L, 140)])
    wins = []
    for i, s in enumerate(src):
        s = int(s)
        read = genome[s:s + L].copy()
        for p in np.nonzero(mask[s:s + L] != (1 << read))[0]:
            listed = [c for c in range(4) if (mask[s + p] >> c) & 1]
            read[p] = listed[rng.integers(0, len(listed))]
        sub = rng.choice(L, i % 9, replace=False)
        read[sub] = (read[sub] + rng.integers(1, 4, len(sub))) & 3
        if i % 7 == 0:
            read[rng.choice(L, 3, replace=False)] = 4
        other = 1500 + (s - 1500) % 300 + 300 * int(rng.integers(0, 39)) if 1500 <= s < 1500 + 300 * 39 else int(rng.integers(0, G - L))
        for pos in (s, min(other, G - L), int(rng.integers(0, G - L))):
            wins.append((pos, read))
    return wins


def run_model(exe, genome, mask, wins, L, k):
    blob = np.array([len(genome), len(wins), L, k], dtype=np.uint32).tobytes() + genome.tobytes() + mask.tobytes()
    blob += b"".join(np.uint32(p).tobytes() + r.tobytes() for p, r in wins)
    p = subprocess.run([exe], input=blob, capture_output=True)
    assert p.returncode == 0, "ctx_model exit %d (2: side B does not hold the genome in front of the suffix)" % p.returncode
    head, _, body = p.stdout.partition(b"\n")
    return [int(x) for x in head.split()], np.frombuffer(body, dtype=np.uint8).reshape(len(wins), L - k + 1)


def pack_ref(mask):
    m = np.concatenate([mask, np.zeros(-len(mask) % 8 + 8, dtype=np.uint8)]).astype(np.uint32).reshape(-1, 8)
    return np.ascontiguousarray((m << (4 * np.arange(8, dtype=np.uint32))).sum(axis=1).astype(np.uint32))


def shares(oracle_lib, models, name):
    """For one geometry: (false rejections, rejected pairs, pairs whose window truly has more than 3 mismatches), over both SNP densities,
    both read lengths and both seed lengths."""
    false_rej, rejected, over = [], 0, 0
    for snp_every in (60, 200):
        rng = np.random.default_rng(1000 + snp_every)
        genome, mask = make_genome(rng, snp_every)
        ref = pack_ref(mask)
        refp = ref.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        for L in (100, 150):
            wins = make_windows(rng, genome, mask, L)
            ed = np.array([oracle_lib.so_ed_mismatch(refp, ctypes.c_uint32(p), r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint32(L), 3)
                           for p, r in wins])
            assert (ed == -1).sum() > len(wins) // 2 and (ed >= 0).sum() > len(wins) // 8          # both kinds of window are there
            for k in (21, 19):
                geo, rej = run_model(models[name], genome, mask, wins, L, k)
                want = GEOMETRIES[name] or (9, (2, 0), 37, 2)
                assert geo == [want[0], want[1][0] * k + want[1][1], want[2], want[3]], geo
                for w in np.nonzero(rej.any(axis=1) & (ed != -1))[0]:
                    false_rej.append((snp_every, L, k, wins[w][0], np.nonzero(rej[w])[0].tolist(), int(ed[w])))
                rejected += int(rej[ed == -1].sum())
                over += int((ed == -1).sum()) * rej.shape[1]
    return false_rej, rejected, over


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_record_never_rejects_a_window_the_oracle_accepts_and_rejects_most_others(name, models, oracle_lib):
    false_rej, rejected, over = shares(oracle_lib, models, name)
    share = rejected / over
    print("%s: rejected %d of %d (window, offset) pairs with more than 3 mismatches = %.3f" % (name, rejected, over, share))
    assert not false_rej, false_rej[:5]
    assert share >= 0.5 and share >= _OBSERVED[name] - 0.2 * _OBSERVED[name], (share, _OBSERVED[name])
