#!/usr/bin/env python3
"""A dbSNP-shaped VCF over one of the synthetic workloads of salt_amd/workload.py, and the equivalent four-column SNP file: the input of the
`salt-idx --vcf` measurement (profiles/r25/vcf.md).  Sorted by contig and position; one record per SNP of the workload (98 % bi-allelic,
2 % with two ALT alleles joined by a comma) and, beside every tenth, a deletion record at the same position (about 10 % non-SNV records);
ID rs<9 digits>, QUAL and FILTER '.', an INFO field of 150 .. 250 bytes cut out of a dbSNP-like text.  Everything is made with array
operations, so the GRCh38-sized workload (16 M lines, 4 GB) takes a minute, not an hour.

    python tools/vcf_synth.py --config grch38_mini --out DIR      writes DIR/ref.fa, DIR/sites.vcf, DIR/snps.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from salt_amd import workload                                  # noqa: E402

INFO = (b"RS=775809821;RSPOS=10177;dbSNPBuildID=144;SSR=0;SAO=0;VP=0x050000020005170026000200;GENEINFO=DDX11L1:100287102;WGT=1;VC=SNV;R5;ASP;VLD;"
        b"G5A;G5;KGPhase3;CAF=0.5747,0.4253;COMMON=1;TOPMED=0.71,0.29;")


def _put(out, at, text):
    """the same bytes into every line: out[at[i] + j] = text[j]; returns the column behind them"""
    for j, ch in enumerate(text):
        out[at + j] = ch
    return at + len(text)


def _digits(out, at, v, nd):
    """v (all of nd decimal digits) in decimal at out[at[i] ..]"""
    for d in range(nd):
        out[at + d] = 48 + (v // 10 ** (nd - 1 - d)) % 10
    return at + nd


def _layout(width):
    """(buffer pre-filled with the INFO text repeated, offset of every line) for lines of the given widths, each ending in a newline"""
    off = np.concatenate([[0], np.cumsum(width)])
    out = np.resize(np.frombuffer(INFO, dtype=np.uint8), int(off[-1]))
    out[off[1:] - 1] = 10
    return out, off[:-1]


def synth(config="grch38_mini", device="cpu"):
    """(contigs as salt_amd.idx_build_mem takes them, the VCF's bytes, the SNP file's bytes) -- uint8 arrays"""
    import torch
    c = workload.CONFIGS[config]
    n_contigs = c.get("contigs", 1)
    g = workload.make_genome_hash(c["genome_len"], device=device)
    pos_t, mask_t = workload.make_snps_hash(g, c["n_snps"])
    genome, pos, mask = g.cpu().numpy(), pos_t.cpu().numpy(), mask_t.cpu().numpy()
    del g, pos_t, mask_t
    if device != "cpu":
        torch.cuda.empty_cache()
    bounds = np.array(workload.contig_bounds(len(genome), n_contigs), dtype=np.int64)
    names = ["synth1" if n_contigs == 1 else "synth%d" % (i + 1) for i in range(n_contigs)]
    contigs = [(names[i], workload.ACGT[genome[bounds[i]:bounds[i + 1]]]) for i in range(n_contigs)]
    ci = np.searchsorted(bounds, pos, side="right") - 1
    p1 = pos - bounds[ci] + 1                                   # 1-based position in its contig
    ref = genome[pos]
    alts = [(mask >> b) & 1 for b in range(4)]
    for b in range(4):
        alts[b] = alts[b] & (ref != b)
    n_alt = sum(a.astype(np.int64) for a in alts)
    first = np.select([alts[0] == 1, alts[1] == 1, alts[2] == 1], [0, 1, 2], 3)
    last = np.select([alts[3] == 1, alts[2] == 1, alts[1] == 1], [3, 2, 1], 0)
    letters = workload.ACGT
    nl = np.array([len(n) for n in names])[ci]
    nd = 1 + sum((p1 >= 10 ** k).astype(np.int64) for k in range(1, 11))
    name_tab = np.zeros((n_contigs, 8), dtype=np.uint8)
    for i, n in enumerate(names):
        name_tab[i, :len(n)] = np.frombuffer(n.encode(), dtype=np.uint8)

    # ---- the SNP file: name, 1-based pos, alleles in ACGT order joined by '/', ref ----
    n_al = n_alt + 1
    width = nl + 1 + nd + 1 + (2 * n_al - 1) + 1 + 1 + 1
    snp, off = _layout(width)
    for L in np.unique(nl):
        for D in np.unique(nd[nl == L]):
            for A in (2, 3):
                sel = np.flatnonzero((nl == L) & (nd == D) & (n_al == A))
                if not len(sel):
                    continue
                at = off[sel]
                for j in range(L):
                    snp[at + j] = name_tab[ci[sel], j]
                at = _put(snp, at + L, b"\t")
                at = _put(snp, _digits(snp, at, p1[sel], D), b"\t")
                m = mask[sel].astype(np.int64)
                k = np.zeros(len(sel), dtype=np.int64)
                for b in range(4):                               # the b-th base goes to slot k of the lines that list it
                    has = (m >> b) & 1 == 1
                    snp[at[has] + 2 * k[has]] = letters[b]
                    k += has
                for s in range(A - 1):
                    snp[at + 2 * s + 1] = ord("/")
                at = _put(snp, at + 2 * A - 1, b"\t")
                snp[at] = letters[ref[sel]]

    # ---- the VCF: a deletion record beside every tenth SNP, in front of it ----
    has_del = (np.arange(len(pos)) % 10 == 0) & (pos + 1 < bounds[ci + 1])
    rec = np.repeat(np.arange(len(pos)), 1 + has_del.astype(np.int64))
    is_del = np.zeros(len(rec), dtype=bool)
    is_del[np.flatnonzero(rec[1:] == rec[:-1])] = True           # the first of two records of one SNP
    n = len(rec)
    rng = np.random.default_rng(25)
    info = rng.integers(150, 251, size=n)
    kind = np.where(is_del, 0, n_alt[rec])                       # 0: deletion (REF two bases, ALT one), 1: one ALT, 2: two ALTs
    body = np.where(kind == 0, 2 + 1 + 1, np.where(kind == 1, 1 + 1 + 1, 1 + 1 + 3))
    width = nl[rec] + 1 + nd[rec] + 1 + 11 + 1 + body + 1 + 1 + 1 + 1 + 1 + info + 1
    vcf, off = _layout(width)
    rs = 100000000 + np.arange(n, dtype=np.int64) * 7
    nxt = genome[np.minimum(pos + 1, len(genome) - 1)]
    for L in np.unique(nl):
        for D in np.unique(nd[nl == L]):
            for K in (0, 1, 2):
                sel = np.flatnonzero((nl[rec] == L) & (nd[rec] == D) & (kind == K))
                if not len(sel):
                    continue
                r = rec[sel]
                at = off[sel]
                for j in range(L):
                    vcf[at + j] = name_tab[ci[r], j]
                at = _put(vcf, at + L, b"\t")
                at = _put(vcf, _digits(vcf, at, p1[r], D), b"\trs")
                at = _put(vcf, _digits(vcf, at, rs[sel], 9), b"\t")
                vcf[at] = letters[ref[r]]
                if K == 0:
                    vcf[at + 1] = letters[nxt[r]]
                    at = _put(vcf, at + 2, b"\t")
                    vcf[at] = letters[ref[r]]
                    at = at + 1
                else:
                    at = _put(vcf, at + 1, b"\t")
                    vcf[at] = letters[first[r]]
                    at = at + 1
                    if K == 2:
                        at = _put(vcf, at, b",")
                        vcf[at] = letters[last[r]]
                        at = at + 1
                _put(vcf, at, b"\t.\t.\t")
    head = b"##fileformat=VCFv4.2\n##source=salt vcf_synth\n" + b"".join(b"##contig=<ID=%s,length=%d>\n" % (nm.encode(), len(s)) for nm, s in contigs)
    head += b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    return contigs, np.concatenate([np.frombuffer(head, dtype=np.uint8), vcf]), snp


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", default="grch38_mini", choices=sorted(workload.CONFIGS))
    ap.add_argument("--device", default="cpu", help="torch device the workload's generator runs on (cpu, cuda)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    contigs, vcf, snp = synth(a.config, a.device)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ref.fa"), "wb") as f:
        for name, seq in contigs:
            f.write(b">" + name.encode() + b"\n")
            full = len(seq) // 80 * 80
            f.write(np.concatenate([seq[:full].reshape(-1, 80), np.full((full // 80, 1), 10, dtype=np.uint8)], axis=1).tobytes())
            if full < len(seq):
                f.write(seq[full:].tobytes() + b"\n")
    vcf.tofile(os.path.join(a.out, "sites.vcf"))
    snp.tofile(os.path.join(a.out, "snps.txt"))
    print("%d contigs, %d bases, %d VCF bytes, %d SNP-file bytes -> %s" % (len(contigs), sum(len(s) for _, s in contigs), len(vcf), len(snp), a.out))


if __name__ == "__main__":
    main()
