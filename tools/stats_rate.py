#!/usr/bin/env python3
"""What --stats costs (run on the GPU box): the resident single-end path on the benchmark's workload, steps dealt to four workspaces /
streams as bench.py deals them; legs with every tally off and with one tally on -- the run's summary, and beside it the depth, the SNP
counts and the error profile without qualities -- alternating in one session; then k_stats_add alone, as the time of taking a step's adds
back (salt_gpu_ws_stats_uncount: the same kernel and a stream synchronisation), and what the tables hold.

usage: stats_rate.py [workload] [steps per leg] [legs]          (grch38, 24, 3)"""
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
cfg = workload.CONFIGS[name]
L, n = cfg["read_len"], cfg["n_reads"]
dev = torch.device("cuda", 0)
g, p, m = workload.generate_device(name, dev)
w = workload.prepare(name, os.environ.get("SALT_BENCH_CACHE", "/tmp/salt_bench_cache"), gpu_device=0, arrays=(g, p, m))
site = workload.make_site_map(g.numel(), p, m)
n_batches, n_streams = 4, 4
batches = [workload.make_reads_hash(g, site, n, L, seed=1, batch=b)[:2] for b in range(n_batches)]
del g, p, m, site
torch.cuda.empty_cache()
idx = salt_amd.Index.reload(w["prefix"], rebuild_lkt=False)
aln = salt_amd.GpuAligner(idx, max_reads=n, max_bases=n * L)
aln.set_contigs(idx)
alns = [aln] + [aln.fork() for _ in range(n_streams - 1)]
streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
res = [torch.zeros(n * salt_amd.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(n_streams)]
opt = salt_amd.AlnOpt(l_seed=cfg["k"])


def step(i):
    s, o = batches[i % n_batches]
    alns[i % n_streams].align_resident(opt, n, L, s.data_ptr(), o.data_ptr(), res[i % n_streams].data_ptr(), streams[i % n_streams].cuda_stream)


def leg(k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


leg(8)                                                            # warm: buffers grown, code objects loaded
switch = {"stats": aln.stats_enable, "depth": aln.depth_enable, "snp-counts": aln.snp_enable, "error-profile": aln.errprof_enable}
for k, f in switch.items():                                       # every table allocated, every tally's code object loaded before the first timed leg
    f(True, 0)
    leg(2)
    f(False)
aln.stats_tables(reset=True)
fmt = lambda v: " ".join("%.3f" % x for x in v)
ms = {k: [] for k in ["off"] + list(switch)}
for _ in range(legs):
    ms["off"].append(leg(steps))
    for k, f in switch.items():
        f(True, 0)
        ms[k].append(leg(steps))
        f(False)
print("%d contigs; ms per step of %d reads, %d steps a leg, %d streams, legs alternating (every tally off; one tally on, MAPQ >= 0; the error profile without qualities):"
      % (len(idx.contigs()), n, steps, n_streams))
base = sum(ms["off"]) / legs
for k, v in ms.items():
    print("  %-14s %s   mean %.3f = %+.1f %% of a step" % (k, fmt(v), sum(v) / legs, (sum(v) / legs - base) / base * 100))

cells, ct = aln.stats_tables(reset=True)
T = salt_amd.stats_split(cells)
print("tables after %d counted steps: SN[0] %s; %d MAPQ values, %d GC bins, %d contigs with mapped records"
      % (legs * steps, T["SN"][0].tolist(), int((T["MQ"][0] != 0).sum()), int((T["GC"][0] != 0).sum()), int((ct[:, 0] != 0).sum())))

# the kernel alone: a step's adds taken back (k_stats_add once more with delta 2^64 - 1, and the stream's synchronisation)
aln.stats_enable(True, 0)
alone = []
for i in range(6):
    step(0)
    torch.cuda.synchronize()
    alone.append(timed(aln.stats_uncount))
cells, ct = aln.stats_tables()
aln.stats_enable(False)
print("k_stats_add alone (uncount of one step of %d reads, launch + synchronisation): %s ms; the tables are zero again: %s" % (n, fmt(alone), not cells.any() and not ct.any()))
for a in alns[1:]:
    a.close()
aln.close()
