#!/usr/bin/env python3
"""What --genotype costs (run on the GPU box): the resident single-end path on the benchmark's workload, steps dealt to four workspaces /
streams as bench.py deals them, with device-resident quality bytes handed over before every call; legs with every tally off and with one
tally on -- the genotype sums, and beside them the SNP counts, the depth and the error profile -- alternating in one session; the sums'
size and build time; then the calls and the text of the sums as they stand: time to the first and to the last piece and the bytes, plain
and as BGZF.

usage: genotype_rate.py [workload] [steps per leg] [legs]          (grch38, 24, 3)
       GT_RATE_PROFILE=1: one warm leg with the genotype sums on and nothing else -- the run to put under `rocprofv3 --kernel-trace --stats`,
       which gives k_gt_add's own time."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
torch.cuda.init()
import salt_amd
from salt_amd import workload

name = sys.argv[1] if len(sys.argv) > 1 else "grch38"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
legs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
profile = bool(int(os.environ.get("GT_RATE_PROFILE", "0")))
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


def leg(k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        s, o = batches[i % n_batches]
        a = alns[i % n_streams]
        a.set_quals(quals[i % n_batches].data_ptr(), on_device=True)
        a.align_resident(opt, n, L, s.data_ptr(), o.data_ptr(), res[i % n_streams].data_ptr(), streams[i % n_streams].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


leg(8)                                                            # warm: buffers grown, code objects loaded
t_build = timed(lambda: aln.gt_enable(True, 0))
n_sites = len(aln.snp_sites())
n_win = (ref_len + 63) // 64
print("genotype sums: %d sites of %d positions, site table %d windows x 16 B = %.1f MB, sums %d x 128 B = %.1f MB, built in %.1f ms (table + zeroed sums, first enable)"
      % (n_sites, ref_len, n_win, n_win * 16 / 1e6, n_sites, n_sites * 128 / 1e6, t_build))
aln.gt_enable(False)
switch = {"genotype": aln.gt_enable, "snp-counts": aln.snp_enable, "depth": aln.depth_enable, "error-profile": aln.errprof_enable}
for k, f in switch.items():                                       # every table allocated before the first timed leg
    f(True, 0)
    f(False)
fmt = lambda v: " ".join("%.3f" % x for x in v)
counted = 0
if profile:
    aln.gt_enable(True, 0)
    leg(4)
    print("profile leg: %d steps of %d reads with the genotype sums on, %.3f ms per step" % (steps, n, leg(steps)))
    counted = steps + 4
else:
    ms = {k: [] for k in ["off"] + list(switch)}
    for _ in range(legs):
        ms["off"].append(leg(steps))
        for k, f in switch.items():
            f(True, 0)
            ms[k].append(leg(steps))
            f(False)
    counted = legs * steps
    print("ms per step of %d reads, %d steps a leg, %d streams, legs alternating (every tally off; one tally on):" % (n, steps, n_streams))
    base = sum(ms["off"]) / legs
    for k, v in ms.items():
        print("  %-14s %s   mean %.3f = %+.1f %% of a step" % (k, fmt(v), sum(v) / legs, (sum(v) / legs - base) / base * 100))
aln.gt_enable(False)
sums = aln.gt_fetch(0, min(n_sites, 1 << 20))
ev = int(sums[:, :, 0].sum())
print("first %d sites: %d events in %d counted steps; deepest site %d" % (len(sums), ev, counted, int(sums[:, :, 0].sum(axis=1).max())))
del sums

# the calls and the text of the sums as they stand
import ctypes
lib = salt_amd.gpu_lib()
lib.salt_gpu_index_gt_text_begin.argtypes = [ctypes.c_void_p, ctypes.POINTER(salt_amd.api._GtTextOpt)]
lib.salt_gpu_index_gt_text_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
for bgzf in (0, 1, 0, 1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = salt_amd.api._GtTextOpt(0, bgzf)
    assert lib.salt_gpu_index_gt_text_begin(aln._ix, ctypes.byref(o)) == 0, lib.salt_gpu_last_error()
    first, total, pieces = None, 0, 0
    while True:
        ptr, nb = ctypes.c_void_p(), ctypes.c_uint64()
        assert lib.salt_gpu_index_gt_text_next(aln._ix, ctypes.byref(ptr), ctypes.byref(nb)) == 0, lib.salt_gpu_last_error()
        if nb.value == 0:
            break
        if first is None:
            first = time.perf_counter() - t0
        total += nb.value
        pieces += 1
    t_all = time.perf_counter() - t0
    print("text %s: %d pieces, %d bytes (%.1f per site), first piece after %.1f ms, last after %.1f ms = %.2f GB/s"
          % ("bgzf " if bgzf else "plain", pieces, total, total / max(n_sites, 1), (first or 0) * 1e3, t_all * 1e3, total / t_all / 1e9))
for a in alns[1:]:
    a.close()
aln.close()
