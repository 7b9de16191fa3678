#!/usr/bin/env python3
"""What --depth costs (run on the GPU box): the resident single-end path on the benchmark's workload, steps dealt to four workspaces /
streams as bench.py deals them, with the marking off and on in alternating legs; the time of the first enable and the free memory before
and after it; then the finishing -- per base and --depth-window 1000, as text and as BGZF blocks: time and bytes.

usage: depth_rate.py [workload] [steps per leg] [legs]          (grch38, 24, 3)"""
import ctypes, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
torch.cuda.init()
import salt_amd
from salt_amd import workload
from salt_amd.api import _DepthTextOpt, _gpu_check, gpu_lib

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
        alns[i % n_streams].align_resident(opt, n, L, s.data_ptr(), o.data_ptr(), res[i % n_streams].data_ptr(), streams[i % n_streams].cuda_stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def text(window, bgzf):
    """(seconds, bytes, pieces) of one text of the array as it stands; the pieces are counted, not kept"""
    lib = gpu_lib()
    lib.salt_gpu_index_depth_text_begin.argtypes = [ctypes.c_void_p, ctypes.POINTER(_DepthTextOpt)]
    lib.salt_gpu_index_depth_text_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
    o = _DepthTextOpt(window, 0, 1 if bgzf else 0)
    t0 = time.perf_counter()
    _gpu_check(lib.salt_gpu_index_depth_text_begin(aln._ix, ctypes.byref(o)))
    total = pieces = 0
    while True:
        ptr, nb = ctypes.c_void_p(), ctypes.c_uint64()
        _gpu_check(lib.salt_gpu_index_depth_text_next(aln._ix, ctypes.byref(ptr), ctypes.byref(nb)))
        if nb.value == 0:
            break
        total += nb.value
        pieces += 1
    return time.perf_counter() - t0, total, pieces


leg(8)                                                            # warm: buffers grown, code objects loaded
torch.cuda.synchronize()
free0 = torch.cuda.mem_get_info(0)[0]
t0 = time.perf_counter()
aln.depth_enable(True, 0)
torch.cuda.synchronize()
t_enable = time.perf_counter() - t0
free1, total_mem = torch.cuda.mem_get_info(0)
print("difference array: %d positions, %.1f MB, first enable %.1f ms; free memory %.1f GB before, %.1f GB after, of %.1f GB, beside %d workspaces"
      % (ref_len, (ref_len + 1) * 4 / 1e6, t_enable * 1e3, free0 / 1e9, free1 / 1e9, total_mem / 1e9, n_streams))
off, on = [], []
for _ in range(legs):
    aln.depth_enable(False)
    off.append(leg(steps))
    aln.depth_enable(True, 0)
    on.append(leg(steps))
aln.depth_enable(False)
fmt = lambda v: " ".join("%.3f" % x for x in v)
print("ms per step of %d reads, %d steps a leg, %d streams, legs alternating: off %s | on %s" % (n, steps, n_streams, fmt(off), fmt(on)))
print("Mreads/s: off %s | on %s" % (" ".join("%.1f" % (n / x / 1e3) for x in off), " ".join("%.1f" % (n / x / 1e3) for x in on)))
# the coverage the marked steps left: twice the reads' bases would be summed from a sample of the array, so it is taken from the marks
marked = legs * steps
probe = aln.depth_fetch(0, min(ref_len + 1, 1 << 26))
print("marked: %d steps = %d reads; the first %d words hold %d marks (+1 words %d); mean depth if every read mapped %.2f"
      % (marked, marked * n, probe.size, int(np.count_nonzero(probe)), int((probe.astype(np.int32) > 0).sum()), marked * n * L / ref_len))
del probe
for window in (0, 1000):
    for bgzf in (False, True):
        secs, nbytes, pieces = text(window, bgzf)
        print("finish %s, %s: %.2f s, %d bytes in %d pieces" % ("per base" if window == 0 else "windows of %d" % window, "BGZF blocks" if bgzf else "text", secs, nbytes, pieces))
print("free memory with the text buffers: %.1f GB" % (torch.cuda.mem_get_info(0)[0] / 1e9))
for a in alns[1:]:
    a.close()
aln.close()
