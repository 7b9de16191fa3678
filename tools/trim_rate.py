#!/usr/bin/env python3
"""What trimming costs.  A chunk of 100-base reads cut from the lambda fixture's genome (32 MiB of FASTQ by default), a third of them cut to
a random insert and filled up with a 33-base adapter and random bases, a third with a low-quality tail.

  trim_rate.py host   [MiB]          salt_trim_fastq on one host thread over the chunk, three runs: Mreads/s (no GPU needed)
  trim_rate.py device [MiB] [calls]  text calls on the chunk with trimming off and on, alternating: ms per call, and the difference; run it
                                     under `rocprofv3 --kernel-trace --stats -- python tools/trim_rate.py device` for k_fq_trim's own
                                     time beside k_fq_count, k_fq_lines, k_fq_parse and k_fq_codes of the same trace
  trim_rate.py write  FILE [MiB]     the chunk and its pre-trimmed copy as FILE and FILE.trimmed, for timing the `salt` binary on both"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import salt_amd

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
LAMBDA = os.path.join(ROOT, "tests", "golden", "lambda")
ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
TRIM = dict(adapter=ADAPTER, qual=20)


def chunk(mib, L=100, seed=1):
    rng = np.random.default_rng(seed)
    fa = open(os.path.join(LAMBDA, "genome.fa"), "rb").read().split(b">")[1]
    genome = np.frombuffer(b"".join(fa.split(b"\n")[1:]), dtype=np.uint8)
    n = (mib << 20) // (2 * L + 16)
    start = rng.integers(0, len(genome) - L, n)
    seq = genome[start[:, None] + np.arange(L)[None, :]].copy()
    qual = np.full((n, L), ord("I"), dtype=np.uint8)
    kind = rng.integers(0, 3, n)
    ins = rng.integers(1, 100, n)
    fill = np.concatenate([np.frombuffer(ADAPTER.encode(), dtype=np.uint8)[None, :].repeat(n, 0), np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L))]], axis=1)
    col = np.arange(L)[None, :]
    behind = (kind == 0)[:, None] & (col >= ins[:, None])
    seq[behind] = np.take_along_axis(fill, np.clip(col - ins[:, None], 0, fill.shape[1] - 1), axis=1)[behind]
    tail = rng.integers(1, L + 1, n)
    low = (kind == 1)[:, None] & (col >= (L - tail)[:, None])
    qual[low] = (33 + rng.integers(2, 11, (n, L)))[low].astype(np.uint8)
    rec = np.full((n, 2 * L + 16), ord("\n"), dtype=np.uint8)
    names = np.frombuffer(b"".join(b"@r%08d" % i for i in range(n)), dtype=np.uint8).reshape(n, 10)
    rec[:, :10] = names; rec[:, 11:11 + L] = seq; rec[:, 12 + L] = ord("+"); rec[:, 14 + L:14 + 2 * L] = qual
    return rec[:, :15 + 2 * L].tobytes(), n


what = sys.argv[1] if len(sys.argv) > 1 else "host"
if what == "write":
    mib = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    fq, n = chunk(mib)
    open(sys.argv[2], "wb").write(fq)
    open(sys.argv[2] + ".trimmed", "wb").write(salt_amd.trim_fastq(fq, **TRIM))
    print("%d reads, %d bytes -> %s, %s.trimmed" % (n, len(fq), sys.argv[2], sys.argv[2]))
    sys.exit(0)
mib = int(sys.argv[2]) if len(sys.argv) > 2 else 32
fq, n = chunk(mib)
if what == "host":
    counts = np.zeros((2, 8), dtype=np.uint64)
    secs = []
    for _ in range(3):
        t0 = time.perf_counter(); out = salt_amd.trim_fastq(fq, counts=counts, **TRIM); secs.append(time.perf_counter() - t0)
    print("salt_trim_fastq, one thread, %d reads of 100 bases (%d bytes -> %d): %s s = %s Mreads/s" %
          (n, len(fq), len(out), " ".join("%.3f" % s for s in secs), " ".join("%.2f" % (n / s / 1e6) for s in secs)))
    print("counters of one run:", dict(zip(salt_amd.TRIM_COUNTERS, (counts[0] // 3).tolist())))
    sys.exit(0)
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 5
import torch
torch.cuda.init()
idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
aln = salt_amd.GpuAligner(idx, max_reads=n + 64, max_bases=(n + 64) * 100)
aln.set_contigs(idx)
opt = salt_amd.AlnOpt(l_seed=idx.l_seed, print_xa_cigar=1, print_nm_md=1)
pre = salt_amd.trim_fastq(fq, **TRIM)


def call(text, trim):
    aln.set_trim(**(TRIM if trim else {}))
    t0 = time.perf_counter(); sam, reads = aln.align_se_text(opt, text); dt = (time.perf_counter() - t0) * 1e3
    return dt, sam


call(fq, True); call(pre, False); call(fq, False)                 # warm: buffers grown, code objects loaded
ms = {"untrimmed, off": [], "untrimmed, trimming on": [], "pre-trimmed, off": []}
same = True
for _ in range(calls):
    ms["untrimmed, off"].append(call(fq, False)[0])
    dt, a = call(fq, True); ms["untrimmed, trimming on"].append(dt)
    dt, b = call(pre, False); ms["pre-trimmed, off"].append(dt)
    same = same and a == b
print("align_se_text on %d reads of 100 bases (%d bytes), ms per call, legs alternating; trimmed block == block of the pre-trimmed text: %s" % (n, len(fq), same))
for k, v in ms.items():
    print("  %-24s %s   mean %.2f" % (k, " ".join("%.2f" % x for x in v), sum(v) / len(v)))
spans = []
aln.set_trim(**TRIM)
for _ in range(calls):
    t0 = time.perf_counter(); aln.trim_spans(fq); spans.append((time.perf_counter() - t0) * 1e3)
print("trim_spans (copy in, k_fq_count, k_fq_lines, k_fq_parse, k_fq_trim, spans back), ms per call: %s" % " ".join("%.2f" % x for x in spans))
print("counters:", dict(zip(salt_amd.TRIM_COUNTERS, aln.trim_counts()[0].tolist())))
aln.close()
