#!/usr/bin/env python3
"""Monte Carlo of the context record's geometry (salt_amd/csrc/salt_ctx_record.h) on the bench workload's repeat family: where should
the record's 46 bases lie so that ctx_reject drops the most located rows?  numpy only, no FM index: the copies of a family share
family coordinates, so a suffix-array row of a seed's interval is a copy that matches the seed, at the same offset.

The model, as the reference does it:
  * `--copies` copies of one `--family`-base family, each at its own divergence drawn from 5 .. 15 %;
  * `--reads` reads of `--read-len` bases drawn from inside a copy, 0.5 % substitutions;
  * seeds of k bases at read offsets 0, k, 2 k, ... (alnse_seed_overlap); a seed whose interval holds more than max_seed + 1 rows is
    extended to the LEFT, one base at a time, while it does and while ext < s -- so the seed of slot 0 is never extended;
  * intervals located smallest first until max_locate rows are located (the rows of the interval that crosses the cap: a random part);
  * per geometry (n_front, a_start, n_behind): the share of located rows whose mismatches VISIBLE to the record exceed 3 -- side B
    faces read bases off - 1 .. off - n_front, side A faces off + a_start .. off + a_start + n_behind - 1, inside [0, L) only.
It prints that share per geometry, the share of rows whose whole window has more than 3 mismatches (what no record can beat), and
the histogram of (read offset of the suffix, matched length) of the located rows, which is what decides the geometry.

Left out: SNP sites and N (every position counts), the R index, reads that only partly overlap a copy, reverse strands.

  python tools/ctx_geometry_model.py --read-len 100        # 40 s on one CPU core with the defaults; --copies 1e5 for a quick look
  python tools/ctx_geometry_model.py --read-len 150 --geometry 9,63,37 --geometry 12,63,34
"""
import argparse

import numpy as np

BASES = 46


def default_geometries(k):
    """The short list the record was chosen from (profiles/r05/ab_ctx_geometry.log), and the symmetric record before it; a_start in seed lengths."""
    return [(23, k, 23), (23, 3 * k, 23), (9, 2 * k, 37), (9, 2 * k + 8, 37), (9, 3 * k, 37), (12, 3 * k, 34), (5, 2 * k + 8, 41), (0, 2 * k, 46)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--copies", type=float, default=1.03e6, help="copies of the family (the bench workload: 1.03 M)")
    ap.add_argument("--reads", type=int, default=150)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--family", type=int, default=300, help="bases of the family")
    ap.add_argument("-k", type=int, default=21, help="seed length = seed stride")
    ap.add_argument("--max-seed", type=int, default=50)
    ap.add_argument("--max-locate", type=int, default=1000)
    ap.add_argument("--geometry", action="append", default=[], metavar="N_FRONT,A_START,N_BEHIND", help="instead of the short list; may repeat")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    n_copy, L, K, fam_len = int(a.copies), a.read_len, a.k, a.family
    geoms = [tuple(int(x) for x in g.split(",")) for g in a.geometry] or default_geometries(K)
    for nb, a0, na in geoms:
        if nb + na != BASES or a0 < K:
            ap.error("geometry %d,%d,%d: n_front + n_behind must be %d and side A must start behind the seed" % (nb, a0, na, BASES))

    fam = rng.integers(0, 4, fam_len, dtype=np.uint8)
    div = rng.uniform(0.05, 0.15, n_copy)
    mut = rng.random((n_copy, fam_len), dtype=np.float32) < div[:, None]
    copies = np.where(mut, (fam[None, :] + rng.integers(1, 4, (n_copy, fam_len), dtype=np.uint8)) & 3, fam[None, :]).astype(np.uint8)
    del mut

    tot_rows = ideal = 0
    rej = {g: 0 for g in geoms}
    hist = {}
    slots = range(0, L - K + 1, K)
    for _ in range(a.reads):
        x = int(rng.integers(0, n_copy))
        o = int(rng.integers(0, fam_len - L + 1))
        read = copies[x, o:o + L].copy()
        e = rng.random(L) < 0.005
        read[e] = (read[e] + rng.integers(1, 4, int(e.sum()))) & 3
        eq = copies[:, o:o + L] == read[None, :]                   # [copy, read base]
        lists = []
        for s in slots:
            m = np.flatnonzero(eq[:, s:s + K].all(axis=1))
            if len(m) == 0:
                continue
            ext = 0
            while len(m) - 1 > a.max_seed and ext < s:
                m2 = m[eq[m, s - ext - 1]]
                if len(m2) == 0:
                    break
                m = m2
                ext += 1
            lists.append((len(m), s - ext, K + ext, m))
        lists.sort(key=lambda t: t[0])
        n = 0
        for size, off, mlen, m in lists:
            if n >= a.max_locate:
                break
            take = m if n + size <= a.max_locate else rng.choice(m, a.max_locate - n, replace=False)
            n += len(take)
            hist[(off, mlen)] = hist.get((off, mlen), 0) + len(take)
            mm = ~eq[take]                                          # mismatches of the whole window
            ideal += int((mm.sum(axis=1) > 3).sum())
            tot_rows += len(take)
            for g in geoms:
                nb, a0, na = g
                fr = mm[:, max(0, off - nb):off].sum(axis=1)
                lo, hi = min(L, off + a0), min(L, off + a0 + na)
                rej[g] += int(((fr + (mm[:, lo:hi].sum(axis=1) if hi > lo else 0)) > 3).sum())

    print("copies %d, reads %d x %d bases, k %d, located rows %d (%.0f per read)" % (n_copy, a.reads, L, K, tot_rows, tot_rows / a.reads))
    print("rows whose window really has > 3 mismatches: %.3f" % (ideal / max(1, tot_rows)))
    for nb, a0, na in geoms:
        print("  %2d in front, behind = [%3d, %3d)   rejected %.3f" % (nb, a0, a0 + na, rej[(nb, a0, na)] / max(1, tot_rows)))
    top = sorted(hist.items(), key=lambda kv: -kv[1])[:12]
    print("located rows by (read offset of the suffix, matched length):", [(k, round(v / max(1, tot_rows), 3)) for k, v in top])


if __name__ == "__main__":
    main()
