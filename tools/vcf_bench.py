#!/usr/bin/env python3
"""The `salt-idx --vcf` measurement of profiles/r25/vcf.md: the synthetic dbSNP-shaped VCF of tools/vcf_synth.py over a workload of
salt_amd/workload.py, ingested by the device parser (salt_gpu_vcf_*, the text's host-to-device copies included), by the host twin on one
thread (salt_vcf_snps) and, as the SNP file of the same sites, by the parent's reader (tools/snp_file_read, when it has been built).
One JSON line per run; the medians are taken by the reader of the log.

    python tools/vcf_bench.py --config grch38 --runs 6          (the first run of each is the warm-up)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import salt_amd                                                 # noqa: E402
from salt_amd import api                                        # noqa: E402
import vcf_synth                                                # noqa: E402


def say(**kw):
    print(json.dumps(kw), flush=True)


def device_run(run, contigs, text, chunk_bytes):
    g = salt_amd.gpu_lib()
    n = len(contigs)
    seq = (ctypes.c_void_p * n)(*[s.ctypes.data for _, s in contigs])
    lens = (ctypes.c_uint64 * n)(*[len(s) for _, s in contigs])
    keys = (ctypes.c_char_p * n)(*[nm.encode() for nm, _ in contigs])
    kc = (ctypes.c_int32 * n)(*range(n))

    class Opt(ctypes.Structure):
        _fields_ = [("pass_only", ctypes.c_int32), ("reserved", ctypes.c_int32), ("chunk_bytes", ctypes.c_uint64)]
    opt = Opt(0, 0, chunk_bytes)
    g.salt_gpu_vcf_open.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_void_p)]
    g.salt_gpu_vcf_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    g.salt_gpu_vcf_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    g.salt_gpu_vcf_fetch.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    g.salt_gpu_vcf_close.argtypes = [ctypes.c_void_p]
    h = ctypes.c_void_p()
    t0 = time.perf_counter()
    api._gpu_check(g.salt_gpu_vcf_open(0, n, seq, lens, n, keys, kc, ctypes.byref(opt), ctypes.byref(h)))
    t1 = time.perf_counter()
    api._gpu_check(g.salt_gpu_vcf_add(h, text.ctypes.data, len(text)))
    t2 = time.perf_counter()
    ct = api._VcfCounters()
    per = (ctypes.c_uint32 * n)()
    api._gpu_check(g.salt_gpu_vcf_finish(h, ctypes.byref(ct), per))
    t3 = time.perf_counter()
    for i in range(n):
        pos, al, rf = np.empty(per[i], np.uint32), np.empty(per[i], np.uint8), np.empty(per[i], np.uint8)
        api._gpu_check(g.salt_gpu_vcf_fetch(h, i, pos.ctypes.data, al.ctypes.data, rf.ctypes.data))
    t4 = time.perf_counter()
    g.salt_gpu_vcf_close(h)
    say(what="device", run=run, open_s=round(t1 - t0, 3), add_s=round(t2 - t1, 3), finish_s=round(t3 - t2, 3), fetch_s=round(t4 - t3, 3),
        ingest_s=round(t4 - t1, 3), total_s=round(t4 - t0, 3), lines=int(ct.lines), sites=int(ct.sites), lines_per_s=round(ct.lines / (t4 - t1)))
    return int(ct.lines), int(ct.sites)


def copy_run(run, text, chunk_bytes):
    """the text's bytes alone through one page-locked buffer to the device, chunk by chunk: what the copies cost without any parse"""
    import torch
    pin = torch.empty(chunk_bytes, dtype=torch.uint8).pin_memory()
    dev = torch.empty(chunk_bytes, dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(text)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for lo in range(0, len(text), chunk_bytes):
        c = min(chunk_bytes, len(text) - lo)
        pin[:c].copy_(src[lo:lo + c])
        dev[:c].copy_(pin[:c], non_blocking=True)
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    for lo in range(0, len(text), chunk_bytes):
        c = min(chunk_bytes, len(text) - lo)
        dev[:c].copy_(pin[:c], non_blocking=True)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    say(what="copy", run=run, staged_s=round(t1 - t0, 3), h2d_only_s=round(t2 - t1, 3), bytes=len(text))


def host_run(run, contigs, text):
    t0 = time.perf_counter()
    groups, ct = salt_amd.vcf_snps(contigs, memoryview(text))
    t1 = time.perf_counter()
    say(what="host_twin", run=run, total_s=round(t1 - t0, 3), lines=ct["lines"], sites=ct["sites"], lines_per_s=round(ct["lines"] / (t1 - t0)))
    return ct["lines"], ct["sites"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="grch38_mini")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--only", default="device,copy,host,snpfile")
    ap.add_argument("--chunk-bytes", type=int, default=16 << 20)
    a = ap.parse_args()
    import torch
    t0 = time.perf_counter()
    contigs, text, snp = vcf_synth.synth(a.config, "cuda" if torch.cuda.is_available() else "cpu")
    say(what="synth", config=a.config, seconds=round(time.perf_counter() - t0, 1), vcf_bytes=len(text), snp_file_bytes=len(snp), bases=sum(len(s) for _, s in contigs))
    only = a.only.split(",")
    seen = set()
    if "device" in only:
        for r in range(a.runs):
            seen.add(device_run(r, contigs, text, a.chunk_bytes))
    if "copy" in only:
        for r in range(a.runs):
            copy_run(r, text, a.chunk_bytes)
    if "host" in only:
        os.environ["SALT_IDX_VERBOSE"] = "1"
        for r in range(a.runs):
            seen.add(host_run(r, contigs, text))
    assert len(seen) <= 1, seen
    exe = os.path.join(ROOT, "tools", "snp_file_read")
    if "snpfile" in only and os.path.exists(exe):
        with tempfile.TemporaryDirectory() as d:
            snp.tofile(os.path.join(d, "snps.txt"))
            subprocess.run([exe, os.path.join(d, "snps.txt"), str(a.runs)], check=True)


if __name__ == "__main__":
    main()
