#!/usr/bin/env python3
"""What --discover costs (run on the GPU box): the resident single-end path on the benchmark's workload, steps dealt to four workspaces /
streams as bench.py deals them, with device-resident quality bytes handed over before every call; free device memory before and after the
first enable and its time; legs with every tally off and with one tally on -- the SNP candidates, and beside them the depth, the genotype
sums and the error profile -- alternating in one session; k_disc_add alone, as the time of taking a step's adds back
(salt_gpu_ws_disc_uncount: the same kernel and a stream synchronisation); then the text of the arrays as they stand: time to the first and
to the last piece and the bytes, plain and as BGZF, at the defaults and with all sites.

usage: discover_rate.py [workload] [steps per leg] [legs]          (grch38, 24, 3)"""
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
ref_len = int(g.numel())
del g, p, m, site
torch.cuda.empty_cache()
gen = torch.Generator(device=dev)
gen.manual_seed(5)
quals = [torch.randint(33 + 2, 33 + 42, (n * L + 64,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n_batches)]      # Phred 2 .. 41
idx = salt_amd.Index.reload(w["prefix"], rebuild_lkt=False)
aln = salt_amd.GpuAligner(idx, max_reads=n, max_bases=n * L)
aln.set_contigs(idx)
alns = [aln] + [aln.fork() for _ in range(n_streams - 1)]
streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
res = [torch.zeros(n * salt_amd.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev) for _ in range(n_streams)]
opt = salt_amd.AlnOpt(l_seed=cfg["k"])


def step(i):
    s, o = batches[i % n_batches]
    a = alns[i % n_streams]
    a.set_quals(quals[i % n_batches].data_ptr(), on_device=True)
    a.align_resident(opt, n, L, s.data_ptr(), o.data_ptr(), res[i % n_streams].data_ptr(), streams[i % n_streams].cuda_stream)


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
torch.cuda.empty_cache()
free0 = torch.cuda.mem_get_info(dev)[0]
t_build = timed(lambda: aln.disc_enable(True, 20, 20))
free1 = torch.cuda.mem_get_info(dev)[0]
print("candidate arrays: %d positions, alt %.1f GB + diff %.1f GB; free device memory %.1f GB before the first enable, %.1f GB behind it; allocated and zeroed in %.1f ms"
      % (ref_len, ref_len * 8 / 1e9, (ref_len + 1) * 4 / 1e9, free0 / 1e9, free1 / 1e9, t_build))
aln.disc_enable(False)
switch = {"discover": lambda on, q=20: aln.disc_enable(on, q, 20), "depth": aln.depth_enable, "genotype": aln.gt_enable, "error-profile": aln.errprof_enable}
for k, f in switch.items():                                       # every table allocated before the first timed leg
    f(True, 0)
    f(False)
fmt = lambda v: " ".join("%.3f" % x for x in v)
ms = {k: [] for k in ["off"] + list(switch)}
for _ in range(legs):
    ms["off"].append(leg(steps))
    for k, f in switch.items():
        f(True, 20 if k == "discover" else 0)
        ms[k].append(leg(steps))
        f(False)
print("ms per step of %d reads, %d steps a leg, %d streams, legs alternating (every tally off; one tally on; discover at MAPQ >= 20, base quality >= 20):" % (n, steps, n_streams))
base = sum(ms["off"]) / legs
for k, v in ms.items():
    print("  %-14s %s   mean %.3f = %+.1f %% of a step" % (k, fmt(v), sum(v) / legs, (sum(v) / legs - base) / base * 100))

# the kernel alone: a step's adds taken back (k_disc_add once more with the negated addends, and the stream's synchronisation)
aln.disc_enable(True, 20, 20)
alone = []
for i in range(6):
    step(0)
    torch.cuda.synchronize()
    alone.append(timed(aln.disc_uncount))
aln.disc_enable(False)
print("k_disc_add alone (uncount of one step of %d reads, launch + synchronisation): %s ms" % (n, fmt(alone)))
probe = min(ref_len, 1 << 24)
words = aln.disc_fetch(0, 0, probe)
field = lambda k: (words >> np.uint64(21 * k)) & np.uint64(0x1FFFFF)
ev = sum(int(field(k).sum()) for k in range(3))
print("first %d positions: %d events that counted in %d counted steps, %d positions with one; deepest field %d" %
      (probe, ev, legs * steps, int((words != 0).sum()), max(int(field(k).max()) for k in range(3))))
del words

# the text of the arrays as they stand
import ctypes
lib = salt_amd.gpu_lib()
lib.salt_gpu_index_disc_text_begin.argtypes = [ctypes.c_void_p, ctypes.POINTER(salt_amd.api._DiscTextOpt)]
lib.salt_gpu_index_disc_text_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
for min_alt, min_pct, all_sites, bgzf in ((3, 20, 0, 0), (3, 20, 0, 0), (1, 0, 0, 0), (3, 20, 1, 0), (3, 20, 1, 1)):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = salt_amd.api._DiscTextOpt(min_alt, min_pct, all_sites, 0, bgzf)
    assert lib.salt_gpu_index_disc_text_begin(aln._ix, ctypes.byref(o)) == 0, lib.salt_gpu_last_error()
    first, total, pieces = None, 0, 0
    while True:
        ptr, nb = ctypes.c_void_p(), ctypes.c_uint64()
        assert lib.salt_gpu_index_disc_text_next(aln._ix, ctypes.byref(ptr), ctypes.byref(nb)) == 0, lib.salt_gpu_last_error()
        if nb.value == 0:
            break
        if first is None:
            first = time.perf_counter() - t0
        total += nb.value
        pieces += 1
    t_all = time.perf_counter() - t0
    print("text min_alt %d min_pct %d%s %s: %d pieces, %d bytes, first piece after %.1f ms, last after %.1f ms = %.2f G positions/s"
          % (min_alt, min_pct, " all" if all_sites else "", "bgzf " if bgzf else "plain", pieces, total, (first or 0) * 1e3, t_all * 1e3, ref_len / t_all / 1e9))
for a in alns[1:]:
    a.close()
aln.close()
