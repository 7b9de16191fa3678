#!/usr/bin/env python3
"""What --trim-pair-overlap costs (next to trim_rate.py, which times the per-read steps).  Two blocks of 2 x L-base mates cut from the lambda
fixture's genome, 32 MiB of FASTQ together by default: a third of the pairs read through an insert of 20 to L - 1 bases into their adapters
and random tails, the rest lie over inserts of 300 to 500 bases and take the full scan of the candidates; 1 % substitutions.

  trim_pair_rate.py host   [L] [MiB]          salt_trim_fastq_pair on one host thread over the blocks, three runs: Mpairs/s (no GPU needed)
  trim_pair_rate.py device [L] [MiB] [calls]  paired-end text calls on the blocks, legs alternating: nothing on; --trim-adapter alone
                                              (k_fq_trim, what there was before); the pair rule; the pre-trimmed blocks with nothing on.  Under
                                              `rocprofv3 --kernel-trace --stats -- python tools/trim_pair_rate.py device` the trace holds
                                              k_fq_trim_pair beside k_fq_trim and the four parse kernels on the same blocks.  Against a
                                              library without the pair rule (the parent commit's) only the first two legs run."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import salt_amd

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LAMBDA = os.path.join(ROOT, "tests", "golden", "lambda")
ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ADAPTER2 = "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
PE_ARGS = ["-d", "-p", "-c", "-a", "20", "-b", "650"]


def blocks(mib, L, seed=1):
    rng = np.random.default_rng(seed)
    fa = open(os.path.join(LAMBDA, "genome.fa"), "rb").read().split(b">")[1]
    genome = np.frombuffer(b"".join(fa.split(b"\n")[1:]).upper(), dtype=np.uint8)
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    n = (mib << 20) // (2 * (2 * L + 16))
    ins = np.where(rng.integers(0, 3, n) == 0, rng.integers(20, L, n), rng.integers(300, 501, n))
    start = rng.integers(0, len(genome) - 501, n)
    col = np.arange(L)[None, :]
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for mate, ad in ((0, ADAPTER), (1, ADAPTER2)):
        at = start[:, None] + col if mate == 0 else (start + ins)[:, None] - 1 - col
        seq = genome[np.clip(at, 0, len(genome) - 1)]
        if mate:
            seq = comp[seq]
        fill = np.concatenate([np.frombuffer(ad.encode(), dtype=np.uint8)[None, :].repeat(n, 0), letters[rng.integers(0, 4, (n, L))]], axis=1)
        behind = col >= ins[:, None]
        seq[behind] = np.take_along_axis(fill, np.clip(col - ins[:, None], 0, fill.shape[1] - 1), axis=1)[behind]
        sub = rng.random((n, L)) < 0.01
        seq[sub] = letters[rng.integers(0, 4, (n, L))][sub]
        rec = np.full((n, 2 * L + 16), ord("\n"), dtype=np.uint8)
        rec[:, :10] = np.frombuffer(b"".join(b"@r%08d" % i for i in range(n)), dtype=np.uint8).reshape(n, 10)
        rec[:, 11:11 + L] = seq; rec[:, 12 + L] = ord("+"); rec[:, 14 + L:14 + 2 * L] = ord("I")
        out.append(rec[:, :15 + 2 * L].tobytes())
    return out[0], out[1], n


what = sys.argv[1] if len(sys.argv) > 1 else "host"
L = int(sys.argv[2]) if len(sys.argv) > 2 else 100
mib = int(sys.argv[3]) if len(sys.argv) > 3 else 32
fq1, fq2, n = blocks(mib, L)
has_pair = hasattr(salt_amd, "trim_fastq_pair")
if what == "host":
    pairs = np.zeros(8, dtype=np.uint64)
    secs = []
    for _ in range(3):
        t0 = time.perf_counter(); out = salt_amd.trim_fastq_pair(fq1, fq2, pair_counts=pairs); secs.append(time.perf_counter() - t0)
    print("salt_trim_fastq_pair, one thread, %d pairs of 2 x %d bases (%d bytes -> %d): %s s = %s Mpairs/s" %
          (n, L, len(fq1) + len(fq2), len(out[0]) + len(out[1]), " ".join("%.3f" % s for s in secs), " ".join("%.3f" % (n / s / 1e6) for s in secs)))
    print("pair counters of one run:", dict(zip(salt_amd.TRIM_PAIR_COUNTERS, (pairs // 3).tolist())))
    sys.exit(0)
calls = int(sys.argv[4]) if len(sys.argv) > 4 else 5
import torch
torch.cuda.init()
idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
aln = salt_amd.GpuAligner(idx, max_reads=2 * n + 64, max_bases=(2 * n + 64) * L)
aln.set_contigs(idx)
aln.set_pac(idx)
opt = salt_amd.AlnOpt.from_argv(PE_ARGS, idx.l_seed)[0]


def call(a, b, adapter=False, pair=False):
    aln.set_trim(**(dict(adapter=ADAPTER, adapter2=ADAPTER2) if adapter else {}))
    if has_pair:
        aln.set_trim_pair() if pair else aln.set_trim_pair(None)
    t0 = time.perf_counter(); sam, pairs = aln.align_pe_text(opt, idx, a, b); dt = (time.perf_counter() - t0) * 1e3
    return dt, sam


legs = {"untrimmed, nothing on": (fq1, fq2, False, False), "untrimmed, --trim-adapter (k_fq_trim)": (fq1, fq2, True, False)}
if has_pair:
    pre = salt_amd.trim_fastq_pair(fq1, fq2)
    legs["untrimmed, pair rule (k_fq_trim_pair)"] = (fq1, fq2, False, True)
    legs["pre-trimmed, nothing on"] = (pre[0], pre[1], False, False)
for args in legs.values():
    call(*args)                                                   # warm: buffers grown, code objects loaded
ms = {k: [] for k in legs}
sams = {}
for _ in range(calls):
    for k, args in legs.items():
        dt, sams[k] = call(*args)
        ms[k].append(dt)
print("align_pe_text on %d pairs of 2 x %d bases (%d bytes), ms per call, legs alternating%s" % (n, L, len(fq1) + len(fq2),
      "; block with the pair rule == block of the pre-trimmed text: %s" % (sams["untrimmed, pair rule (k_fq_trim_pair)"] == sams["pre-trimmed, nothing on"]) if has_pair else ""))
for k, v in ms.items():
    print("  %-40s %s   mean %.2f" % (k, " ".join("%.2f" % x for x in v), sum(v) / len(v)))
if has_pair:
    aln.set_trim()
    aln.set_trim_pair()
    aln.trim_pair_counts(reset=True)
    spans = []
    for _ in range(calls):
        t0 = time.perf_counter(); aln.trim_pair_spans(fq1, fq2); spans.append((time.perf_counter() - t0) * 1e3)
    print("trim_pair_spans (copy in, k_fq_count, k_fq_lines, k_fq_parse, k_fq_trim_pair, spans back), ms per call: %s" % " ".join("%.2f" % x for x in spans))
    print("pair counters of one call:", dict(zip(salt_amd.TRIM_PAIR_COUNTERS, (aln.trim_pair_counts() // calls).tolist())))
aln.close()
