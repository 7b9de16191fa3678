#!/usr/bin/env python3
"""What --snp-counts costs a step (run on the GPU box): the resident single-end path on the benchmark's workload, steps dealt to four
workspaces / streams as bench.py deals them, with the counting off and on in alternating legs; the site table's size and build time;
how many bases were counted.

usage: snp_counts_rate.py [workload] [steps per leg] [legs]          (grch38, 24, 3)
       SNP_RATE_PROFILE=1: one warm leg with the counting on and nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`,
       which gives k_snp_count's own time."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
torch.cuda.init()
import salt_amd
from salt_amd import workload

name = sys.argv[1] if len(sys.argv) > 1 else "grch38"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
profile = bool(int(os.environ.get("SNP_RATE_PROFILE", "0")))
cfg = workload.CONFIGS[name]
L, n = cfg["read_len"], cfg["n_reads"]
dev = torch.device("cuda", 0)
g, p, m = workload.generate_device(name, dev)
w = workload.prepare(name, os.environ.get("SALT_BENCH_CACHE", "/tmp/salt_bench_cache"), gpu_device=0, arrays=(g, p, m))
site = workload.make_site_map(g.numel(), p, m)
n_batches, n_streams = 4, 4
batches = [workload.make_reads_hash(g, site, n, L, seed=1, batch=b)[:2] for b in range(n_batches)]
ref_len = int(g.numel())
del g, p, m, site
torch.cuda.empty_cache()
idx = salt_amd.Index.reload(w["prefix"], rebuild_lkt=False)
aln = salt_amd.GpuAligner(idx, max_reads=n, max_bases=n * L)
alns = [aln] + [aln.fork() for _ in range(n_streams - 1)]
streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
res = [torch.zeros(n * salt_amd.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(n_streams)]
opt = salt_amd.AlnOpt(l_seed=cfg["k"])


def leg(k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        s, o = batches[i % n_batches]
        alns[i % n_streams].align_resident(opt, n, L, s.data_ptr(), o.data_ptr(), res[i % n_streams].data_ptr(), streams[i % n_streams].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


leg(8)                                                            # warm: buffers grown, code objects loaded
torch.cuda.synchronize()
t0 = time.perf_counter()
aln.snp_enable(True, 0)
torch.cuda.synchronize()
t_build = time.perf_counter() - t0
n_sites = len(aln.snp_sites())
n_win = (ref_len + 63) // 64
print("site table: %d sites of %d positions, %d windows x 16 B = %.1f MB, counts %.1f MB, built in %.1f ms (table + zeroed counts, first enable)"
      % (n_sites, ref_len, n_win, n_win * 16 / 1e6, n_sites * 16 / 1e6, t_build * 1e3))
if profile:
    leg(4)
    ms = leg(steps)
    print("profile leg: %d steps of %d reads with the counting on, %.3f ms per step" % (steps, n, ms))
else:
    off, on = [], []
    for _ in range(legs):
        aln.snp_enable(False)
        off.append(leg(steps))
        aln.snp_enable(True, 0)
        on.append(leg(steps))
    fmt = lambda v: " ".join("%.3f" % x for x in v)
    print("ms per step of %d reads, %d steps a leg, %d streams, legs alternating: off %s | on %s" % (n, steps, n_streams, fmt(off), fmt(on)))
    print("Mreads/s: off %s | on %s" % (" ".join("%.1f" % (n / x / 1e3) for x in off), " ".join("%.1f" % (n / x / 1e3) for x in on)))
counts = aln.snp_counts()
calls = (steps + (4 if profile else 0)) if profile else legs * steps
print("counted: %d bases at %d of the sites in %d counted steps = %.2f adds per read; deepest site %d"
      % (int(counts.sum(dtype="uint64")), int((counts.sum(axis=1) > 0).sum()), calls, float(counts.sum(dtype="uint64")) / max(calls * n, 1), int(counts.sum(axis=1).max())))
for a in alns[1:]:
    a.close()
aln.close()
