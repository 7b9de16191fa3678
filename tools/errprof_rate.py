#!/usr/bin/env python3
"""What --error-profile costs (run on the GPU box): the resident single-end path on the benchmark's workload, steps dealt to four
workspaces / streams as bench.py deals them, with the profile off, on without qualities (q = none) and on with resident qualities
(salt_gpu_ws_set_quals, a device pointer) in alternating legs; the time of the first enable; what the counted steps left in the tables;
k_errprof alone, through salt_gpu_ws_errprof_uncount.

usage: errprof_rate.py [workload] [steps per leg] [legs]          (grch38, 24, 3)"""
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
# qualities as a sequencer reports them: mostly high, a tail of low ones, 2 .. 40
gen = torch.Generator(device=dev).manual_seed(7)
quals = [(33 + 40 - torch.clamp((torch.rand(n * L, device=dev, generator=gen) ** 4 * 39).to(torch.uint8), max=38)).to(torch.uint8) for _ in range(n_batches)]
del g, p, m, site
torch.cuda.empty_cache()
idx = salt_amd.Index.reload(w["prefix"], rebuild_lkt=False)
aln = salt_amd.GpuAligner(idx, max_reads=n, max_bases=n * L)
alns = [aln] + [aln.fork() for _ in range(n_streams - 1)]
streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
res = [torch.zeros(n * salt_amd.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(n_streams)]
opt = salt_amd.AlnOpt(l_seed=cfg["k"])


def leg(k, with_quals=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        s, o = batches[i % n_batches]
        a = alns[i % n_streams]
        if with_quals:
            a.set_quals(quals[i % n_batches].data_ptr(), on_device=True)
        a.align_resident(opt, n, L, s.data_ptr(), o.data_ptr(), res[i % n_streams].data_ptr(), streams[i % n_streams].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


leg(8)                                                            # warm: buffers grown, code objects loaded
torch.cuda.synchronize()
t0 = time.perf_counter()
aln.errprof_enable(True, 0)
torch.cuda.synchronize()
print("tables: %d cells, %.2f MB, first enable %.1f ms, beside %d workspaces" % (int(np.prod(salt_amd.ERRPROF_SHAPE)) + 16, (np.prod(salt_amd.ERRPROF_SHAPE) + 16) * 8 / 1e6,
                                                                            (time.perf_counter() - t0) * 1e3, n_streams))
leg(4, True)                                                      # the kernel's code object
aln.errprof_table(reset=True)
off, none, qual = [], [], []
for _ in range(legs):
    aln.errprof_enable(False)
    off.append(leg(steps))
    aln.errprof_enable(True, 0)
    none.append(leg(steps))
    qual.append(leg(steps, True))
aln.errprof_enable(False)
fmt = lambda v: " ".join("%.3f" % x for x in v)
print("ms per step of %d reads of %d bases, %d steps a leg, %d streams, legs alternating: off %s | on, q = none %s | on, resident quals %s" % (n, L, steps, n_streams, fmt(off), fmt(none), fmt(qual)))
print("Mreads/s: off %s | none %s | quals %s" % tuple(" ".join("%.1f" % (n / x / 1e3) for x in v) for v in (off, none, qual)))
E, R = aln.errprof_table()
counted = 2 * legs * steps
ev, mm = int(E.sum()), int((E * (1 - np.eye(4, dtype=np.uint64))).sum())
print("counted: %d steps = %d reads; R[0] %s; %d base events (%.1f a read seen), %d mismatches (%.4f), q bins used %d, cells non-zero %d, none %d"
      % (counted, counted * n, R[0].tolist(), ev, ev / max(int(R[0, 0]), 1), mm, mm / max(ev, 1), int(np.count_nonzero(E.sum(axis=(0, 1, 3, 4)))), int(np.count_nonzero(E)),
         int(E[:, :, 94].sum())))
# the kernel alone: salt_gpu_ws_errprof_uncount launches exactly k_errprof over the last call's batch (delta -1) and waits for it
alone = {}
aln.errprof_enable(True, 0)
for what in ("none", "quals"):
    ts = []
    for _ in range(5):
        if what == "quals":
            aln.set_quals(quals[0].data_ptr(), on_device=True)
        aln.align_resident(opt, n, L, batches[0][0].data_ptr(), batches[0][1].data_ptr(), res[0].data_ptr(), streams[0].cuda_stream)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aln.errprof_uncount()
        ts.append((time.perf_counter() - t0) * 1e3)
    alone[what] = ts
aln.errprof_enable(False)
print("k_errprof alone on the device (launch + wait of one uncount, ms, five times): q = none %s | resident quals %s" % (fmt(alone["none"]), fmt(alone["quals"])))
for a in alns[1:]:
    a.close()
aln.close()
