"""The Smith-Waterman shape sweep (tests/golden/ssw_vectors_shapes.txt.gz, oracle/ref_harness_ssw.c --shapes): loading, the
launches the GPU tests make of it, and the k_swtb band pass each vector needs.  Shared by tests/test_oracle_golden.py (CPU) and
tests/test_gpu_pe.py, which runs `python ssw_sweep.py OUT.npz` as a child process: the stripe variant is chosen once per process
(SALT_GPU_SW_LDS), so each leg gets a fresh one."""
import ctypes
import gzip
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = os.path.join(HERE, "golden", "ssw_vectors_shapes.txt.gz")

MAX_CIGAR_OPS = 64            # SALT_MAX_CIGAR_OPS
SW_BAND_W = 1100              # salt_kernels.h: ints per band row in k_swtb's global scratch
CLASS_EDGES = (104, 152, 256, 512)    # sw_seg_variant: 13 / 19 / 32 stripes of 8 in registers, rows in LDS beyond 256 bases
SALT_E_CAPACITY = -5


class Vec:
    __slots__ = ("aware", "ref", "codes", "want6", "cigar", "n_ops")

    def __init__(self, line):
        t = line.split()
        self.aware = int(t[1])
        self.ref = np.array([int(c, 16) for c in t[2]], dtype=np.uint8)
        self.codes = np.frombuffer(t[3].encode(), dtype=np.uint8) - 48
        self.want6 = [int(x) for x in t[4:10]]
        self.cigar = t[10]
        self.n_ops = len(re.findall(r"\d+[MID]", self.cigar))


def load(path=SHAPES):
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        return [Vec(line) for line in f]


def launches(vecs):
    """One launch per stripe variant: (class edge, vector indices in launch order).  Each launch opens with a run of reads of its
    longest length, SNP-aware and plain in turn (request 0 sets k_swf's packed length, so these run as pairs), then the other lengths
    (k_swf1), neighbours alternating between short and long windows, and closes with one more read of the packed length: with an odd
    number of cases that last request runs as a pair with itself."""
    out = []
    for k, edge in enumerate(CLASS_EDGES):
        lo = CLASS_EDGES[k - 1] if k else 0
        idx = [i for i, v in enumerate(vecs) if lo < len(v.codes) <= edge]
        if not idx:
            continue
        lref = max(len(vecs[i].codes) for i in idx)
        packed = [i for i in idx if len(vecs[i].codes) == lref]
        a0 = [i for i in packed if vecs[i].aware == 0]
        a1 = [i for i in packed if vecs[i].aware == 1]
        mixed = [x for pair in zip(a0, a1) for x in pair] + a0[len(a1):] + a1[len(a0):]
        rest = sorted((i for i in idx if len(vecs[i].codes) != lref), key=lambda i: len(vecs[i].ref))
        alt = []
        while rest:
            alt.append(rest.pop(0))
            if rest:
                alt.append(rest.pop())
        out.append((edge, mixed[:-1] + alt + mixed[-1:]))
    return out


def tb_geom(max_len):
    """k_swtb's LDS per group (salt_pe.hip tb_geom)."""
    read_b = (max_len + 15) & ~15
    ref_b = min((2 * max_len + 15) & ~15, 1024)
    dir_b = min((13 * max_len + 15) & ~15, 4096)
    return read_b, ref_b, 32, dir_b


def tb_pass(v, band, max_len):
    """The k_swtb band pass whose direction bytes the walk reads for vector v in a launch whose longest read is max_len, given the
    half-width `band` at which the doubling stopped (salt_pe.hip k_swtb): 'reg' (half-width <= 3, everything in LDS),
    'lds' (rows and directions in LDS), 'rows_lds', 'dir_lds' (the other one in global scratch), 'global', or 'over' (band beyond
    SW_BAND_W or the global direction bytes).  None for a vector without a traceback."""
    _, ref_b, row_w, dir_b = tb_geom(max_len)
    _, _, rb0, re0, qb0, qe0 = v.want6
    rfl, rdl = re0 - rb0 + 1, qe0 - qb0 + 1
    if rfl <= 0 or rdl <= 0 or band <= 0:
        return None
    width, width_d = 2 * band + 3, 2 * band + 1
    dir_lds = width_d * rdl <= dir_b
    gdir_cap = (max_len * (SW_BAND_W - 3) + 255) & ~255
    if width > SW_BAND_W or (not dir_lds and width_d * rdl > gdir_cap):
        return "over"
    if width - 1 <= 8 and dir_lds and rfl <= ref_b:
        return "reg"
    if width <= row_w:
        return "lds" if dir_lds else "rows_lds"
    return "dir_lds" if dir_lds else "global"


def launch_max_len(vecs, order):
    return max(len(vecs[i].codes) for i in order)


def run_launch(lib, vecs, order):
    """salt_gpu_diag_ssw over vecs[order] in that order: (rc, out6 [n, 6], n_cigar [n], CIGAR texts)."""
    n = len(order)
    aw = np.array([vecs[i].aware for i in order], dtype=np.uint8)
    rs = np.concatenate([vecs[i].ref for i in order])
    qs = np.concatenate([vecs[i].codes for i in order]).astype(np.uint8)
    ro = np.concatenate([[0], np.cumsum([len(vecs[i].ref) for i in order])]).astype(np.uint32)
    qo = np.concatenate([[0], np.cumsum([len(vecs[i].codes) for i in order])]).astype(np.uint32)
    out6 = np.zeros((n, 6), dtype=np.int32)
    cig = np.zeros((n, MAX_CIGAR_OPS), dtype=np.uint16)
    ncig = np.zeros(n, dtype=np.uint16)
    rc = lib.salt_gpu_diag_ssw(n, aw.ctypes.data, rs.ctypes.data, ro.ctypes.data, qs.ctypes.data, qo.ctypes.data,
                               out6.ctypes.data, cig.ctypes.data, ncig.ctypes.data)
    texts = ["".join("%d%s" % (int(x) >> 4, "MID"[int(x) & 3]) for x in cig[k, :int(ncig[k])]) or "-" for k in range(n)]
    return rc, out6, ncig, texts


def main(out_path):
    """Child process: every launch of the sweep, results in launch order to out_path (.npz)."""
    sys.path.insert(0, ROOT)
    try:
        import torch                              # torch's HIP context first, as in the test session (tests/conftest.py)
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    import salt_amd
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_diag_ssw.argtypes = [ctypes.c_uint32] + [ctypes.c_void_p] * 8
    vecs = load()
    res = {}
    for edge, order in launches(vecs):
        rc, out6, ncig, texts = run_launch(lib, vecs, order)
        res["order_%d" % edge] = np.array(order, dtype=np.int32)
        res["rc_%d" % edge] = np.array([rc], dtype=np.int32)
        res["err_%d" % edge] = np.array([(lib.salt_gpu_last_error() or b"").decode()])
        res["out6_%d" % edge] = out6
        res["ncig_%d" % edge] = ncig
        res["cigar_%d" % edge] = np.array(texts)
    np.savez(out_path, **res)
    print("ssw sweep: %d launches, %d vectors" % (len(CLASS_EDGES), len(vecs)))


if __name__ == "__main__":
    main(sys.argv[1])
