#!/usr/bin/env python3
"""What --indels costs (run on the GPU box): the resident single-end path on the benchmark's workload, steps dealt to four workspaces /
streams as bench.py deals them; legs with every tally off and with one tally on -- the indel table, and beside it the SNP candidates (the
sibling with the same walk and its own difference array) -- alternating in one session; device memory before and behind
the enable; k_indel_add alone, as the time of taking a step's adds back (salt_gpu_ws_indel_uncount: the same kernel and a stream
synchronisation); the time and size of the text; then the same legs on reads that are ALL gapped (a two-base deletion or insertion in
the middle of every read of a smaller batch), where the table and not the row head is what the kernel spends its time on.

usage: indel_rate.py [workload] [steps per leg] [legs] [log2 slots] [gapped reads a step]          (grch38, 24, 3, 24, 50000)"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
torch.cuda.init()
import salt_amd
from salt_amd import workload

name = sys.argv[1] if len(sys.argv) > 1 else "grch38"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
log2_slots = int(sys.argv[4]) if len(sys.argv) > 4 else 24
n_gap = int(sys.argv[5]) if len(sys.argv) > 5 else 50000
cfg = workload.CONFIGS[name]
L, n = cfg["read_len"], cfg["n_reads"]
dev = torch.device("cuda", 0)
g, p, m = workload.generate_device(name, dev)
w = workload.prepare(name, os.environ.get("SALT_BENCH_CACHE", "/tmp/salt_bench_cache"), gpu_device=0, arrays=(g, p, m))
site = workload.make_site_map(g.numel(), p, m)
n_batches, n_streams = 4, 4
batches = [workload.make_reads_hash(g, site, n, L, seed=1, batch=b)[:2] for b in range(n_batches)]


def gapped(b):
    """a batch of n_gap reads of L - 2 or L + 2 bases: the benchmark's reads with bases 50 and 51 taken out (even reads) or two bases
    put in behind base 50 (odd reads)"""
    r = workload.make_reads_hash(g, site, n_gap, L, seed=5, batch=b)[0].reshape(n_gap, L)
    dele = torch.cat([r[:, :50], r[:, 52:], torch.full((n_gap, 4), 4, dtype=torch.uint8, device=dev)], dim=1)      # L + 2 columns, the last four unused
    ins = torch.cat([r[:, :50], (3 - r[:, 48:50]), r[:, 50:]], dim=1)
    even = (torch.arange(n_gap, device=dev) % 2 == 0)
    rows = torch.where(even[:, None], dele, ins)
    lens = torch.where(even, torch.full((n_gap,), L - 2, device=dev), torch.full((n_gap,), L + 2, device=dev))
    offs = torch.zeros(n_gap + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(lens, 0)
    keep = torch.arange(L + 2, device=dev)[None, :] < lens[:, None]
    return torch.cat([rows[keep], torch.zeros(64, dtype=torch.uint8, device=dev)]).contiguous(), offs.to(torch.int32)


gap_batches = [gapped(b) for b in range(n_batches)]
del g, p, m, site
torch.cuda.empty_cache()
idx = salt_amd.Index.reload(w["prefix"], rebuild_lkt=False)
aln = salt_amd.GpuAligner(idx, max_reads=n, max_bases=n * L)
aln.set_contigs(idx)
alns = [aln] + [aln.fork() for _ in range(n_streams - 1)]
streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
res = [torch.zeros(n * salt_amd.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(n_streams)]
opt = salt_amd.AlnOpt(l_seed=cfg["k"])


def step(i, gap=False):
    s, o = (gap_batches if gap else batches)[i % n_batches]
    alns[i % n_streams].align_resident(opt, n_gap if gap else n, L + 2 if gap else L, s.data_ptr(), o.data_ptr(), res[i % n_streams].data_ptr(), streams[i % n_streams].cuda_stream)


def leg(k, gap=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(i, gap)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


fmt = lambda v: " ".join("%.3f" % x for x in v)
leg(8)                                                            # warm: buffers grown, code objects loaded
free0 = torch.cuda.mem_get_info(0)[0]
aln.indel_enable(True, 20, log2_slots)
free1 = torch.cuda.mem_get_info(0)[0]
aln.indel_enable(False, 20)
print("device memory: %.1f MB free before the first enable, %.1f MB behind it: %.1f MB for 2^%d slots of 16 bytes and %d + 1 words of diff"
      % (free0 / 1e6, free1 / 1e6, (free0 - free1) / 1e6, log2_slots, idx.ref_len))
switch = {"indels": lambda on: aln.indel_enable(on, 20), "discover": lambda on: aln.disc_enable(on, 20, 20)}      # (--depth's array no longer fits beside these two at this scale)
for k, f in switch.items():                                       # every table allocated, every tally's code object loaded before the first timed leg
    f(True)
    leg(2)
    f(False)
aln.indel_reset()
for gap, what, k_steps in ((False, "%d reads of %d bases, 0.02 %% of them with an indel" % (n, L), steps), (True, "%d reads of %d +- 2 bases, every one gapped" % (n_gap, L), max(steps // 4, 2))):
    leg(2, gap)
    ms = {k: [] for k in ["off"] + list(switch)}
    for _ in range(legs):
        ms["off"].append(leg(k_steps, gap))
        for k, f in switch.items():
            f(True)
            ms[k].append(leg(k_steps, gap))
            f(False)
    print("ms per step of %s; %d steps a leg, %d streams, legs alternating (every tally off; one tally on, MAPQ >= 20, no qualities):" % (what, k_steps, n_streams))
    base = sum(ms["off"]) / legs
    for k, v in ms.items():
        print("  %-10s %s   mean %.3f = %+.2f %% of a step" % (k, fmt(v), sum(v) / legs, (sum(v) / legs - base) / base * 100))
    st = aln.indel_stats()
    t_fetch, pairs = timed(aln.indel_fetch)
    print("  the table after %d counted steps: tabled %d, dropped %d, long %d, unanchored %d; %d live slots of 2^%d (load %.4f), the largest count %d; fetch (select, sort, copy) %.1f ms"
          % (legs * k_steps, st[0], st[1], st[2], st[3], len(pairs), log2_slots, len(pairs) / float(1 << log2_slots),
             int(((pairs[:, 1] & np.uint64(0xFFFFFFFF)) + (pairs[:, 1] >> np.uint64(32))).max()) if len(pairs) else 0, t_fetch))
    for rule in ((3, 20), (1, 0)):
        t_text, text = timed(lambda: aln.indel_text(*rule))
        t_z, z = timed(lambda: aln.indel_text(*rule, bgzf=True))
        print("  text at min_alt %d, min_pct %d: %d records, %d bytes in %.1f ms; as BGZF %d bytes in %.1f ms" % (rule[0], rule[1], text.count(b"\n"), len(text), t_text, len(z), t_z))
    # the kernel alone: a step's adds taken back (k_indel_add once more with delta 2^64 - 1, and the stream's synchronisation)
    aln.indel_enable(True, 20)
    alone = []
    for i in range(6):
        step(0, gap)
        torch.cuda.synchronize()
        alone.append(timed(aln.indel_uncount)[0])
    aln.indel_enable(False, 20)
    print("  k_indel_add alone (uncount of one step, launch + synchronisation): %s ms; the counters are those of before: %s" % (fmt(alone), np.array_equal(aln.indel_stats(), st)))
    aln.indel_reset()
for a in alns[1:]:
    a.close()
aln.close()
