"""ctypes bindings over the product's two C-ABI libraries (include/salt_gpu.h, include/salt_host.h).

The names follow the reference (weiquan/salt, Align_src/):
    Index.reload(prefix)          alnse_index_reload            indexio.c:23-49
    AlnOpt                        aln_opt_t / opt_init defaults aln.h:63-89, aln.c:28-56
    GpuAligner.alnse_core1(...)   alnse_core1 over one batch    alnse.c:1316-1352
    sam_header / samse            aln_samhead / aln_samse       sam.c:56-182

There is no CPU fallback here: every compute entry point goes through libsalt_gpu.so and raises
SaltError when the library or a HIP device is missing.
"""
import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

MAX_HITS = 5
MAX_CIGAR_OPS = 64
CTR_NAMES = ["lkt", "occ_c", "occ_r", "sa_c", "sa_r", "verify", "verify_words", "lv", "reads", "bases", "loci",
             "t_load", "t_gather", "t_locate", "t_sort", "t_dedup", "t_verify", "t_scan", "t_gap", "t_tail", "heavy_reads", "x0", "x1", "x2", "x3",
             "lt_seeds", "lt_locate", "lt_sort", "lt_verify", "lt_out", "lt_samples", "max_heavy", "max_gapfin",
             "d_wlkt", "d_cocc_seed", "d_rocc_seed", "d_sa_seed", "d_text_seed", "d_sa_light", "d_verify_light", "d_out_light",
             "d_sa_heavy", "d_verify_heavy", "d_out_heavy", "d_ctx_rows", "d_ctx_rejected"]


class SaltError(RuntimeError):
    pass


HIT_DTYPE = np.dtype([("pos", "<u4"), ("n_diff", "u1"), ("is_gap", "u1"), ("strand", "<u2")])
RESULT_DTYPE = np.dtype([
    ("pos", "<u4"), ("strand", "u1"), ("n_diff", "u1"), ("is_gap", "u1"), ("mapq", "u1"),
    ("b0", "<i4"), ("b1", "<i4"), ("seq_start", "<u2"), ("seq_end", "<u2"),
    ("n_hits", "u1", (2,)), ("n_cigar", "u1"), ("skipped", "u1"),
    ("hits", HIT_DTYPE, (2, MAX_HITS)),
    ("hit_n_cigar", "u1", (MAX_HITS,)), ("pad", "u1", (3,)),
    ("cigar", "<u2", (MAX_CIGAR_OPS,)),
    ("hit_cigar", "<u2", (MAX_HITS, MAX_CIGAR_OPS)),
])
assert RESULT_DTYPE.itemsize == 880


class _HostIndex(ctypes.Structure):
    _fields_ = [
        ("c_primary", ctypes.c_uint32), ("c_L2", ctypes.c_uint32 * 5), ("c_seq_len", ctypes.c_uint32),
        ("c_bwt_size", ctypes.c_uint32), ("c_bwt", ctypes.c_void_p),
        ("c_sa_intv", ctypes.c_uint32), ("c_n_sa", ctypes.c_uint32), ("c_sa", ctypes.c_void_p),
        ("lkt_len", ctypes.c_uint32), ("lkt_n", ctypes.c_uint32), ("lkt", ctypes.c_void_p),
        ("r_text_len", ctypes.c_uint32), ("r_inv_sa0", ctypes.c_uint32), ("r_cum", ctypes.c_uint32 * 6),
        ("r_bwt_words", ctypes.c_uint32), ("r_bwt", ctypes.c_void_p),
        ("r_occ_words", ctypes.c_uint32), ("r_occ", ctypes.c_void_p),
        ("r_major_words", ctypes.c_uint32), ("r_major", ctypes.c_void_p),
        ("r_n_sa", ctypes.c_uint32), ("r_sa", ctypes.c_void_p),
        ("ref_len", ctypes.c_uint32), ("ref", ctypes.c_void_p),
        ("l_seed", ctypes.c_int32),
    ]


class _AlnOpt(ctypes.Structure):
    _fields_ = [("l_seed", ctypes.c_int32), ("l_overlap", ctypes.c_int32), ("max_seed", ctypes.c_uint32),
                ("max_locate", ctypes.c_uint32), ("max_hits", ctypes.c_int32), ("seed_only_ref", ctypes.c_int32),
                ("collect_counters", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class _PeOpt(ctypes.Structure):
    _fields_ = [("min_tlen", ctypes.c_uint32), ("max_tlen", ctypes.c_uint32)]


class _SamOpt(ctypes.Structure):
    _fields_ = [("print_xa_cigar", ctypes.c_int32), ("print_nm_md", ctypes.c_int32), ("rg_id", ctypes.c_char_p)]


_gpu = None
_host = None


def host_lib():
    global _host
    if _host is None:
        path = os.path.join(LIB_DIR, "libsalt_host.so")
        if not os.path.exists(path):
            raise SaltError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
        lib = ctypes.CDLL(path)
        lib.salt_index_load.restype = ctypes.c_void_p
        lib.salt_index_load.argtypes = [ctypes.c_char_p, ctypes.c_int]
        lib.salt_index_free.argtypes = [ctypes.c_void_p]
        lib.salt_index_host_view.restype = ctypes.POINTER(_HostIndex)
        lib.salt_index_host_view.argtypes = [ctypes.c_void_p]
        lib.salt_index_seed_len.argtypes = [ctypes.c_void_p]
        lib.salt_index_n_seqs.argtypes = [ctypes.c_void_p]
        lib.salt_host_last_error.restype = ctypes.c_char_p
        lib.salt_sam_header.argtypes = [ctypes.c_void_p, ctypes.POINTER(_SamOpt), ctypes.c_char_p, ctypes.c_size_t]
        lib.salt_index_pac.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        lib.salt_index_pac.restype = ctypes.c_void_p
        lib.salt_sam_pe.argtypes = [ctypes.c_void_p, ctypes.POINTER(_SamOpt), ctypes.POINTER(_PeOpt), ctypes.POINTER(ctypes.c_char_p),
                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_char_p),
                                    ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.salt_sam_se.argtypes = [ctypes.c_void_p, ctypes.POINTER(_SamOpt), ctypes.c_char_p, ctypes.c_void_p,
                                    ctypes.c_int32, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.salt_lkt_build.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        lib.salt_cigar_text.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
        lib.salt_index_seq.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                                       ctypes.POINTER(ctypes.c_char_p)]
        lib.salt_bam_header.restype = ctypes.c_int64
        lib.salt_bam_header.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        lib.salt_bam_from_sam.restype = ctypes.c_int64
        lib.salt_bam_from_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64)]
        _host = lib
    return _host


def gpu_lib():
    """The HIP library.  Missing library = hard error (never a silent fallback)."""
    global _gpu
    if _gpu is None:
        path = os.path.join(LIB_DIR, "libsalt_gpu.so")
        if not os.path.exists(path):
            raise SaltError("%s is missing: the HIP extension was not built" % path)
        lib = ctypes.CDLL(path)
        lib.salt_gpu_last_error.restype = ctypes.c_char_p
        lib.salt_gpu_result_size.restype = ctypes.c_uint32
        lib.salt_gpu_index_attach.argtypes = [ctypes.POINTER(_HostIndex), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        lib.salt_gpu_index_detach.argtypes = [ctypes.c_void_p]
        lib.salt_gpu_index_image.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.salt_gpu_index_attach_image.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        lib.salt_gpu_ws_create.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
        lib.salt_gpu_ws_destroy.argtypes = [ctypes.c_void_p]
        lib.salt_gpu_align_se.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlnOpt), ctypes.c_uint32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p]
        lib.salt_gpu_align_se_resident.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlnOpt), ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.salt_gpu_index_set_pac.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        lib.salt_gpu_align_pe.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlnOpt), ctypes.POINTER(_PeOpt), ctypes.c_uint32,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.salt_gpu_align_pe_resident.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlnOpt), ctypes.POINTER(_PeOpt), ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.salt_gpu_ws_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        lib.salt_gpu_ws_pe_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        lib.salt_gpu_index_image_compact.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.salt_gpu_index_attach_compact.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        lib.salt_gpu_index_image_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        lib.salt_gpu_ws_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.salt_gpu_ws_queue_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        lib.salt_gpu_ws_heavy_reads.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        lib.salt_gpu_ws_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)]
        lib.salt_gpu_diag_verify.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        lib.salt_gpu_diag_occ.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        lib.salt_gpu_diag_pack.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5
        assert lib.salt_gpu_result_size() == RESULT_DTYPE.itemsize
        _gpu = lib
    return _gpu


def _gpu_check(rc):
    if rc != 0:
        raise SaltError("salt_gpu error %d: %s" % (rc, gpu_lib().salt_gpu_last_error().decode()))


@dataclass
class AlnOpt:
    """aln_opt_t as the SE path reads it; defaults of opt_init()/aln_opt_init() (aln.c:28-56, aln.h:112-145)."""
    l_seed: int = 25
    l_overlap: int = -1
    max_seed: int = 50
    max_locate: int = 1000
    max_hits: int = 5
    seed_only_ref: int = 0
    print_xa_cigar: int = 0
    print_nm_md: int = 0
    rg_id: str = None
    collect_counters: int = 0
    paired: int = 0             # -p
    min_tlen: int = 250         # -a (aln.c:43)
    max_tlen: int = 550         # -b (aln.c:44)

    def _pe(self):
        return _PeOpt(self.min_tlen, self.max_tlen)

    def _c(self):
        ov = self.l_overlap if self.l_overlap > 0 else self.l_seed          # aln.c:223
        return _AlnOpt(self.l_seed, ov, self.max_seed, self.max_locate, self.max_hits, self.seed_only_ref,
                       self.collect_counters, 0)

    def _sam(self):
        return _SamOpt(self.print_xa_cigar, self.print_nm_md, self.rg_id.encode() if self.rg_id else None)

    @classmethod
    def from_argv(cls, argv, l_seed):
        """Parses salt's option letters (optstring aln.c:102); ignored flags stay ignored."""
        import getopt
        opts, rest = getopt.getopt(argv, "t:n:hpa:b:g:em:s:l:cdr:vM:O:E:X:")
        o = cls(l_seed=l_seed)
        for k, v in opts:
            if k == "-s":
                o.max_seed = int(v)
            elif k == "-m":
                o.max_locate = int(v)
            elif k == "-r":
                o.l_overlap = int(v)
            elif k == "-v":
                o.seed_only_ref = 1
            elif k == "-c":
                o.print_xa_cigar = 1
            elif k == "-d":
                o.print_nm_md = 1
            elif k == "-g":
                o.rg_id = v
            elif k == "-p":
                o.paired = 1
            elif k == "-a":
                o.min_tlen = int(v)
            elif k == "-b":
                o.max_tlen = int(v)
        return o, rest


class Index:
    """index_t: the arrays of the index files, on the host."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def reload(cls, prefix, rebuild_lkt=True):
        h = host_lib().salt_index_load(os.fsencode(prefix), 1 if rebuild_lkt else 0)
        if not h:
            raise SaltError(host_lib().salt_host_last_error().decode())
        return cls(h)

    @property
    def view(self):
        return host_lib().salt_index_host_view(self._h)

    @property
    def l_seed(self):
        return host_lib().salt_index_seed_len(self._h)

    @property
    def ref_len(self):
        """positions of the concatenated genome (the length of <P>.ref)"""
        return int(self.view.contents.ref_len)

    def destroy(self):
        if self._h:
            host_lib().salt_index_free(self._h)
            self._h = None

    def sam_header(self, opt):
        buf = ctypes.create_string_buffer(1 << 20)
        so = opt._sam()
        n = host_lib().salt_sam_header(self._h, ctypes.byref(so), buf, len(buf))
        if n < 0:
            raise SaltError("SAM header too large")
        return buf.raw[:n]

    def contigs(self):
        """[(offset in the concatenated genome, length, name)] of <P>.C.ann: what @SQ, RNAME and BAM's reference list come from."""
        lib = host_lib()
        out = []
        for i in range(lib.salt_index_n_seqs(self._h)):
            off, ln, nm = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_char_p()
            lib.salt_index_seq(self._h, i, ctypes.byref(off), ctypes.byref(ln), ctypes.byref(nm))
            out.append((off.value, ln.value, nm.value))
        return out

    def pac(self):
        n = ctypes.c_uint64()
        p = host_lib().salt_index_pac(self._h, ctypes.byref(n))
        return p, n.value

    def sampe(self, opt, names, seqs, quals, result_rows):
        """Both SAM records of a pair (bytes, with the reference's blank line after each)."""
        buf = ctypes.create_string_buffer(16384 + 16 * (len(seqs[0]) + len(seqs[1])))
        so, pe = opt._sam(), opt._pe()
        sq = [np.ascontiguousarray(x, dtype=np.uint8) for x in seqs]
        rows = np.ascontiguousarray(result_rows)
        nm = (ctypes.c_char_p * 2)(names[0], names[1])
        ql = (ctypes.c_char_p * 2)(quals[0], quals[1])
        sp = (ctypes.c_void_p * 2)(sq[0].ctypes.data, sq[1].ctypes.data)
        ls = (ctypes.c_int32 * 2)(len(sq[0]), len(sq[1]))
        n = host_lib().salt_sam_pe(self._h, ctypes.byref(so), ctypes.byref(pe), nm, sp, ls, ql, rows.ctypes.data, buf, len(buf))
        if n < 0:
            raise SaltError("SAM record too large")
        return buf.raw[:n]

    def samse(self, opt, name, seq, qual, result_row):
        """One SAM record (bytes, no newline) for a row of RESULT_DTYPE."""
        buf = ctypes.create_string_buffer(4096 + 8 * len(seq))
        so = opt._sam()
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        row = np.ascontiguousarray(result_row)
        n = host_lib().salt_sam_se(self._h, ctypes.byref(so), name, seq.ctypes.data, len(seq), qual,
                                   row.ctypes.data, buf, len(buf))
        if n < 0:
            raise SaltError("SAM record too large")
        return buf.raw[:n]


# ---- index builder (salt-idx; include/salt_host.h, include/salt_gpu.h "index construction on the device") ----
_BUILD_C = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32)
_BUILD_R = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p)
_LAST_ERR = ctypes.CFUNCTYPE(ctypes.c_char_p)


class _IdxBackend(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("build_c", _BUILD_C), ("build_r", _BUILD_R), ("last_error", _LAST_ERR)]


class _IdxContig(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("comment", ctypes.c_char_p), ("seq", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class _IdxSnps(ctypes.Structure):
    _fields_ = [("chr", ctypes.c_char_p), ("pos", ctypes.c_void_p), ("alleles", ctypes.c_void_p), ("ref", ctypes.c_void_p), ("n", ctypes.c_uint32)]


IDX_NO_LP = 1


def _idx_backend(gpu_device):
    """None -> the host suffix sorter; a device number -> the device builder of libsalt_gpu.so."""
    if gpu_device is None:
        return None
    g = gpu_lib()
    return _IdxBackend(int(gpu_device), ctypes.cast(g.salt_gpu_idx_build_c, _BUILD_C), ctypes.cast(g.salt_gpu_idx_build_r, _BUILD_R),
                       ctypes.cast(g.salt_gpu_idx_last_error, _LAST_ERR))


_VCF_OPEN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_void_p)
_VCF_ADD = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)
_VCF_FINISH = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
_VCF_FETCH = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
_VCF_CLOSE = ctypes.CFUNCTYPE(None, ctypes.c_void_p)
VCF_COUNTERS = ("lines", "kept", "sites", "unknown_contig", "out_of_range", "not_snv", "ref_mismatch", "filtered")


class _VcfDevice(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("open", _VCF_OPEN), ("add", _VCF_ADD), ("finish", _VCF_FINISH), ("fetch", _VCF_FETCH), ("close", _VCF_CLOSE),
                ("last_error", _LAST_ERR)]


class _VcfCounters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in VCF_COUNTERS + ("first_unknown_line",)]


class _VcfOpt(ctypes.Structure):
    _fields_ = [("pass_only", ctypes.c_int32), ("n_rename", ctypes.c_int32), ("rename_from", ctypes.POINTER(ctypes.c_char_p)),
                ("rename_to", ctypes.POINTER(ctypes.c_char_p)), ("chunk_bytes", ctypes.c_uint64), ("device", ctypes.POINTER(_VcfDevice)),
                ("rename_file", ctypes.c_char_p), ("snp_out", ctypes.c_char_p), ("counters", ctypes.POINTER(_VcfCounters)),
                ("unknown_name", ctypes.c_void_p), ("unknown_name_cap", ctypes.c_uint32)]


def _vcf_opt(gpu_device, pass_only, rename, chunk_bytes, keep):
    """salt_vcf_opt_t; `keep` collects what the struct points to.  gpu_device None: the host twin, else the device ingest of libsalt_gpu.so."""
    o = _VcfOpt()
    o.pass_only = 1 if pass_only else 0
    pairs = list(rename.items()) if isinstance(rename, dict) else list(rename or [])
    o.n_rename = len(pairs)
    if pairs:
        fr = (ctypes.c_char_p * len(pairs))(*[os.fsencode(a) for a, _ in pairs])
        to = (ctypes.c_char_p * len(pairs))(*[os.fsencode(b) for _, b in pairs])
        keep += [fr, to]
        o.rename_from, o.rename_to = fr, to
    o.chunk_bytes = int(chunk_bytes or 0)
    if gpu_device is not None:
        g = gpu_lib()
        d = _VcfDevice(int(gpu_device), ctypes.cast(g.salt_gpu_vcf_open, _VCF_OPEN), ctypes.cast(g.salt_gpu_vcf_add, _VCF_ADD),
                       ctypes.cast(g.salt_gpu_vcf_finish, _VCF_FINISH), ctypes.cast(g.salt_gpu_vcf_fetch, _VCF_FETCH),
                       ctypes.cast(g.salt_gpu_vcf_close, _VCF_CLOSE), ctypes.cast(g.salt_gpu_last_error, _LAST_ERR))
        keep.append(d)
        o.device = ctypes.pointer(d)
    return o


def vcf_snps(contigs, vcf_bytes, gpu_device=None, pass_only=False, rename=None, chunk_bytes=None):
    """SNP sites from the text of a VCF under the rule of DESIGN.md 2.2 (salt_vcf_snps): contigs as idx_build_mem takes them, vcf_bytes the plain
    text.  Returns (groups, counters): groups is what idx_build_mem takes -- one (name, positions, allele masks, reference codes) per contig
    in FASTA order, matched by NAME, empty for a contig without sites -- and counters a dict of the eight counts plus first_unknown_line.
    gpu_device None: the host twin; a device number: the device parser, cut into chunks of chunk_bytes (None: its default).  rename: VCF name
    -> FASTA name (dict or pairs).  SaltError on a malformed line names its 1-based line number."""
    lib = host_lib()
    keep = []
    cs = (_IdxContig * len(contigs))()
    for i, (name, seq) in enumerate(contigs):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        keep.append(seq)
        cs[i] = _IdxContig(name.encode(), None, seq.ctypes.data, len(seq))
    opt = _vcf_opt(gpu_device, pass_only, rename, chunk_bytes, keep)
    text = np.frombuffer(vcf_bytes, dtype=np.uint8)            # bytes, a memoryview or a uint8 array: not copied
    lib.salt_vcf_snps.restype = ctypes.c_void_p
    lib.salt_vcf_snps.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.salt_vcf_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.salt_vcf_group.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.salt_vcf_free.argtypes = [ctypes.c_void_p]
    lib.salt_idx_last_error.restype = ctypes.c_char_p
    h = lib.salt_vcf_snps(cs, len(contigs), text.ctypes.data if len(text) else None, len(text), ctypes.byref(opt))
    if not h:
        raise SaltError("VCF: %s" % lib.salt_idx_last_error().decode())
    try:
        ct = _VcfCounters()
        lib.salt_vcf_counters(h, ctypes.byref(ct))
        groups = []
        for i, (name, _) in enumerate(contigs):
            g = _IdxSnps()
            if lib.salt_vcf_group(h, i, ctypes.byref(g)) != 0:
                raise SaltError("VCF: %s" % lib.salt_idx_last_error().decode())
            n = g.n
            pos = np.ctypeslib.as_array(ctypes.cast(g.pos, ctypes.POINTER(ctypes.c_uint32)), (n,)).copy() if n else np.zeros(0, np.uint32)
            al = np.ctypeslib.as_array(ctypes.cast(g.alleles, ctypes.POINTER(ctypes.c_uint8)), (n,)).copy() if n else np.zeros(0, np.uint8)
            rf = np.ctypeslib.as_array(ctypes.cast(g.ref, ctypes.POINTER(ctypes.c_uint8)), (n,)).copy() if n else np.zeros(0, np.uint8)
            groups.append((name, pos, al, rf))
        return groups, {n: int(getattr(ct, n)) for n, _ in _VcfCounters._fields_}
    finally:
        lib.salt_vcf_free(h)


def idx_build(fasta, snps, prefix, l_seed, gpu_device=None, flags=0, vcf=False, vcf_opts=None):
    """salt-idx: FASTA + SNP file -> index files (index_main, Index_src/index1.c:46-185).  vcf=True: `snps` is a VCF (plain, BGZF or gzip;
    salt_idx_build_vcf) and vcf_opts a dict of pass_only, rename (dict or pairs), rename_file, snp_out, device (True: parse on gpu_device),
    chunk_bytes; the eight counters and first_unknown_line are returned as a dict."""
    lib = host_lib()
    be = _idx_backend(gpu_device)
    if vcf:
        vo = dict(vcf_opts or {})
        keep = []
        opt = _vcf_opt(gpu_device if vo.pop("device", False) else None, vo.pop("pass_only", False), vo.pop("rename", None), vo.pop("chunk_bytes", None), keep)
        ct = _VcfCounters()
        opt.counters = ctypes.pointer(ct)
        if vo.get("rename_file"):
            opt.rename_file = os.fsencode(vo.pop("rename_file"))
        if vo.get("snp_out"):
            opt.snp_out = os.fsencode(vo.pop("snp_out"))
        if any(v for v in vo.values()):
            raise SaltError("unknown vcf_opts: %s" % ", ".join(sorted(vo)))
        lib.salt_idx_build_vcf.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        lib.salt_idx_last_error.restype = ctypes.c_char_p
        if lib.salt_idx_build_vcf(os.fsencode(fasta), os.fsencode(snps), os.fsencode(prefix), int(l_seed), ctypes.byref(be) if be else None, int(flags),
                                  ctypes.byref(opt)) != 0:
            raise SaltError("index build failed: %s" % lib.salt_idx_last_error().decode())
        return {n: int(getattr(ct, n)) for n, _ in _VcfCounters._fields_}
    lib.salt_idx_build_ex.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.salt_idx_last_error.restype = ctypes.c_char_p
    if lib.salt_idx_build_ex(os.fsencode(fasta), os.fsencode(snps), os.fsencode(prefix), int(l_seed), ctypes.byref(be) if be else None, int(flags)) != 0:
        raise SaltError("index build failed: %s" % lib.salt_idx_last_error().decode())


def idx_build_mem(contigs, snp_groups, prefix, l_seed, gpu_device=None, flags=0):
    """The same from memory.  contigs: [(name, uint8 array of base LETTERS)]; snp_groups: [(chr name, uint32 0-based positions,
    uint8 allele masks, uint8 reference codes)] in contig order (group i belongs to contig i)."""
    lib = host_lib()
    be = _idx_backend(gpu_device)
    keep = []
    cs = (_IdxContig * len(contigs))()
    for i, (name, seq) in enumerate(contigs):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        keep.append(seq)
        cs[i] = _IdxContig(name.encode(), None, seq.ctypes.data, len(seq))
    gs = (_IdxSnps * max(len(snp_groups), 1))()
    for i, (name, pos, al, ref) in enumerate(snp_groups):
        pos, al, ref = np.ascontiguousarray(pos, dtype=np.uint32), np.ascontiguousarray(al, dtype=np.uint8), np.ascontiguousarray(ref, dtype=np.uint8)
        keep += [pos, al, ref]
        gs[i] = _IdxSnps(name.encode(), pos.ctypes.data, al.ctypes.data, ref.ctypes.data, len(pos))
    lib.salt_idx_build_mem.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.salt_idx_last_error.restype = ctypes.c_char_p
    rc = lib.salt_idx_build_mem(cs, len(contigs), gs, len(snp_groups), os.fsencode(prefix), int(l_seed), ctypes.byref(be) if be else None, int(flags))
    if rc != 0:
        raise SaltError("index build failed: %s" % lib.salt_idx_last_error().decode())


def suffix_array(text, bits, gpu_device=None):
    """Full suffix array (empty suffix first) of a uint8 symbol array: host SA-IS, or the device sorter."""
    text = np.ascontiguousarray(text, dtype=np.uint8)
    sa = np.zeros(len(text) + 1, dtype=np.uint32)
    if gpu_device is None:
        lib = host_lib()
        lib.salt_idx_suffix_array_cpu.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
        if lib.salt_idx_suffix_array_cpu(text.ctypes.data, len(text), bits, sa.ctypes.data) != 0:
            raise SaltError("host suffix sorter failed")
    else:
        g = gpu_lib()
        g.salt_gpu_suffix_array.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
        g.salt_gpu_idx_last_error.restype = ctypes.c_char_p
        if g.salt_gpu_suffix_array(int(gpu_device), text.ctypes.data, len(text), bits, sa.ctypes.data) != 0:
            raise SaltError("device suffix sorter: %s" % g.salt_gpu_idx_last_error().decode())
    return sa


BGZF_CUT = 32640        # text bytes per BGZF block (salt_amd/csrc/salt_bgzf_block.h)
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_deflate(data, device=0):
    """data -> BGZF blocks (blocked gzip, one block per BGZF_CUT bytes) by the device kernels behind `salt --bgzf`.
    No end-of-file block: append BGZF_EOF after the last piece of a stream."""
    g = gpu_lib()
    g.salt_gpu_bgzf_deflate.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    data = bytes(data)
    cap = len(data) + 31 * ((len(data) + BGZF_CUT - 1) // BGZF_CUT)
    out = ctypes.create_string_buffer(max(cap, 1))
    n = ctypes.c_uint64(0)
    _gpu_check(g.salt_gpu_bgzf_deflate(int(device), data, len(data), out, cap, ctypes.byref(n)))
    return out.raw[:n.value]


def bgzf_inflate(data, device=0):
    """Whole BGZF members (blocked gzip; an end-of-file block is one) -> their text, by the device kernel behind blocked-gzip FASTQ input.
    SaltError when a member is damaged: the message names the first such member and the reason."""
    g = gpu_lib()
    g.salt_gpu_bgzf_inflate.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    data = bytes(data)
    n = ctypes.c_uint64(0)
    rc = g.salt_gpu_bgzf_inflate(int(device), data, len(data), None, 0, ctypes.byref(n))       # the text's length (ISIZE fields): nothing runs yet
    if rc != -5:                                                                               # SALT_E_CAPACITY: there is text
        _gpu_check(rc)
        return b""
    out = ctypes.create_string_buffer(n.value)
    _gpu_check(g.salt_gpu_bgzf_inflate(int(device), data, len(data), out, n.value, ctypes.byref(n)))
    return out.raw[:n.value]


BAM_MAX_NAME = 254      # bytes of a BAM read name (l_read_name is one byte and counts the NUL)


def bam_header(index, header_text):
    """The uncompressed head of a BAM file (SAM spec 4.2): magic, header_text as given, the reference list of the index's contigs."""
    h = host_lib()
    header_text = bytes(header_text)
    cap = len(header_text) + 64 + sum(len(nm) + 16 for _, _, nm in index.contigs())
    out = ctypes.create_string_buffer(cap)
    n = h.salt_bam_header(index._h, header_text, len(header_text), out, cap)
    if n < 0:
        raise SaltError("BAM header: %s" % (h.salt_host_last_error().decode() if n == -1 else "buffer too small"))
    return out.raw[:n]


def bam_from_sam(index, sam):
    """This program's own SAM records (no header lines) -> the BAM records `salt --bam` holds for them, by the host encoder
    (salt_bam_from_sam): one per non-empty line.  It is also the model the device's record kernels are compared with."""
    h = host_lib()
    sam = bytes(sam)
    cap = 4 * len(sam) + 64
    out = ctypes.create_string_buffer(cap)
    n = h.salt_bam_from_sam(index._h, sam, len(sam), out, cap, None)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode() if n == -1 else "BAM records larger than their bound")
    return out.raw[:n]


def snp_sites(index):
    """The genome positions (0-based, concatenated coordinate) whose mixRef mask lists two or more bases, ascending: uint32 array
    (salt_snp_sites, the host twin of GpuAligner.snp_sites)."""
    h = host_lib()
    h.salt_snp_sites.restype = ctypes.c_int64
    h.salt_snp_sites.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    n = h.salt_snp_sites(index._h, None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    pos = np.zeros(n, dtype=np.uint32)
    h.salt_snp_sites(index._h, pos.ctypes.data, n)
    return pos


def snp_count_sam(index, sam, min_mapq=0, counts=None):
    """What this program's own SAM text shows at the SNP sites: (n_sites, 4) uint32 counts, A C G T (salt_snp_count_sam, the host twin of
    the device's counts).  counts: an array of an earlier call to add into."""
    h = host_lib()
    h.salt_snp_sites.restype = ctypes.c_int64
    h.salt_snp_sites.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_snp_count_sam.restype = ctypes.c_int64
    h.salt_snp_count_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    sam = bytes(sam)
    n_sites = h.salt_snp_sites(index._h, None, 0)
    if counts is None:
        counts = np.zeros((n_sites, 4), dtype=np.uint32)
    if counts.dtype != np.uint32 or counts.shape != (n_sites, 4) or not counts.flags.c_contiguous:
        raise SaltError("snp_count_sam: counts must be a contiguous (%d, 4) uint32 array" % n_sites)
    if h.salt_snp_count_sam(index._h, sam, len(sam), int(min_mapq), counts.ctypes.data, n_sites) < 0:
        raise SaltError(h.salt_host_last_error().decode())
    return counts


def depth_add_sam(index, sam, min_mapq=0, diff=None):
    """The coverage difference array of this program's own SAM text: uint32[ref_len + 1], +1 where an M run begins and -1 where it ends
    (salt_depth_add_sam, the host twin of the device's k_depth_mark).  diff: an array of an earlier call to add into.  Returns
    (diff, records that counted)."""
    h = host_lib()
    h.salt_depth_add_sam.restype = ctypes.c_int64
    h.salt_depth_add_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    sam = bytes(sam)
    if diff is None:
        diff = np.zeros(index.ref_len + 1, dtype=np.uint32)
    if diff.dtype != np.uint32 or diff.ndim != 1 or not diff.flags.c_contiguous:
        raise SaltError("depth_add_sam: diff must be a contiguous uint32 array of ref_len + 1 words")
    n = h.salt_depth_add_sam(index._h, sam, len(sam), int(min_mapq), diff.ctypes.data, diff.size)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    return diff, int(n)


def depth_text(index, diff, window=0):
    """The text of a difference array (salt_depth_text, the host twin of the device's text kernels): window 0 = per-base bedGraph, one
    line per run of equal depth inside a contig; window W = the mean depth of every window of W positions.  bytes."""
    h = host_lib()
    h.salt_depth_text.restype = ctypes.c_int64
    h.salt_depth_text.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    diff = np.ascontiguousarray(diff, dtype=np.uint32)
    n = h.salt_depth_text(index._h, diff.ctypes.data, diff.size, int(window), None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    if h.salt_depth_text(index._h, diff.ctypes.data, diff.size, int(window), out, n) != n:
        raise SaltError("depth_text: the size of the text changed between two calls")
    return out.raw[:n]


ERRPROF_SHAPE = (2, 512, 95, 4, 4)       # E[mate][cycle][q][ref][read]; q 94 = "none"


def errprof_add_sam(index, sam, min_mapq=0, tables=None):
    """The error profile of this program's own SAM text (salt_errprof_add_sam, the host twin of the device's k_errprof): base events by
    mate, cycle, quality, genome base and read base, the index's SNP sites and N left out.  tables: the (E, R) of an earlier call to add
    into.  Returns (E uint64 (2, 512, 95, 4, 4), R uint64 (2, 8), records that counted)."""
    h = host_lib()
    h.salt_errprof_add_sam.restype = ctypes.c_int64
    h.salt_errprof_add_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    sam = bytes(sam)
    E, R = tables if tables is not None else (np.zeros(ERRPROF_SHAPE, dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64))
    for a, shape in ((E, ERRPROF_SHAPE), (R, (2, 8))):
        if a.dtype != np.uint64 or a.shape != shape or not a.flags.c_contiguous:
            raise SaltError("errprof_add_sam: tables must be contiguous uint64 arrays of shapes (2, 512, 95, 4, 4) and (2, 8)")
    n = h.salt_errprof_add_sam(index._h, sam, len(sam), int(min_mapq), E.ctypes.data, E.size, R.ctypes.data)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    return E, R, int(n)


def errprof_text(E, R, min_mapq=0, full=False):
    """The bytes of `salt --error-profile`'s file for the tables (salt_errprof_text)."""
    h = host_lib()
    h.salt_errprof_text.restype = ctypes.c_int64
    h.salt_errprof_text.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64]
    E = np.ascontiguousarray(E, dtype=np.uint64)
    R = np.ascontiguousarray(R, dtype=np.uint64)
    if E.shape != ERRPROF_SHAPE or R.shape != (2, 8):
        raise SaltError("errprof_text: tables of shapes (2, 512, 95, 4, 4) and (2, 8)")
    n = h.salt_errprof_text(E.ctypes.data, R.ctypes.data, int(min_mapq), 1 if full else 0, None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    if h.salt_errprof_text(E.ctypes.data, R.ctypes.data, int(min_mapq), 1 if full else 0, out, n) != n:
        raise SaltError("errprof_text: the size of the text changed between two calls")
    return out.raw[:n]


# the run's summary (salt_gpu.h, SALT_STATS_*): name -> (offset in the fixed cells, shape)
STATS_TABLES = {"SN": (0, (2, 16)), "MQ": (32, (2, 256)), "RL": (544, (2, 513)), "GC": (1570, (2, 102)), "XA": (1774, (2, 8)), "IS": (1790, (4097,)),
                "OR": (5887, (4,)), "ID": (5891, (2, 65))}
STATS_CELLS = 6021
STATS_CT_LDS = 64                         # contigs whose CT rows k_stats_add sums in LDS (SALT_STATS_CT_LDS)
STATS_CHUNK = 2048                        # records a workgroup of k_stats_add owns (SALT_STATS_CHUNK)


def stats_split(cells):
    """The fixed cells of the summary as a dict of views, name -> array of the table's shape."""
    cells = np.asarray(cells)
    if cells.shape != (STATS_CELLS,):
        raise SaltError("stats_split: %d cells, the summary has %d" % (cells.size, STATS_CELLS))
    return {k: cells[o:o + int(np.prod(shape))].reshape(shape) for k, (o, shape) in STATS_TABLES.items()}


def _stats_arrays(index, tables, what):
    n = len(index.contigs())
    cells, ct = tables if tables is not None else (np.zeros(STATS_CELLS, dtype=np.uint64), np.zeros((n, 8), dtype=np.uint64))
    for a, shape in ((cells, (STATS_CELLS,)), (ct, (n, 8))):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint64 or a.shape != shape or not a.flags.c_contiguous:
            raise SaltError("%s: tables must be contiguous uint64 arrays of shapes (%d,) and (%d, 8)" % (what, STATS_CELLS, n))
    return cells, ct


def stats_add_sam(index, sam, min_mapq=0, tables=None):
    """The summary of this program's own SAM text (salt_stats_add_sam, the host twin of the device's k_stats_add).  tables: the (cells, ct)
    of an earlier call to add into.  Returns (cells uint64 (6021,), ct uint64 (contigs, 8), records that counted); stats_split names the
    tables inside cells."""
    h = host_lib()
    h.salt_stats_add_sam.restype = ctypes.c_int64
    h.salt_stats_add_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    sam = bytes(sam)
    cells, ct = _stats_arrays(index, tables, "stats_add_sam")
    n = h.salt_stats_add_sam(index._h, sam, len(sam), int(min_mapq), cells.ctypes.data, cells.size, ct.ctypes.data, ct.size)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    return cells, ct, int(n)


def stats_text(index, cells, ct, min_mapq=0):
    """The bytes of `salt --stats`'s file for the tables (salt_stats_text)."""
    h = host_lib()
    h.salt_stats_text.restype = ctypes.c_int64
    h.salt_stats_text.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    cells, ct = _stats_arrays(index, (np.ascontiguousarray(cells, dtype=np.uint64), np.ascontiguousarray(ct, dtype=np.uint64)), "stats_text")
    n = h.salt_stats_text(index._h, cells.ctypes.data, cells.size, ct.ctypes.data, ct.size, int(min_mapq), None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    if h.salt_stats_text(index._h, cells.ctypes.data, cells.size, ct.ctypes.data, ct.size, int(min_mapq), out, n) != n:
        raise SaltError("stats_text: the size of the text changed between two calls")
    return out.raw[:n]


GT_Q_NONE = 20                            # the quality of an event without a quality byte (SALT_GT_Q_NONE)


def _gt_host():
    h = host_lib()
    h.salt_snp_sites.restype = ctypes.c_int64
    h.salt_snp_sites.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_gt_add_sam.restype = ctypes.c_int64
    h.salt_gt_add_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_gt_text.restype = ctypes.c_int64
    h.salt_gt_text.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_gt_header.restype = ctypes.c_int64
    h.salt_gt_header.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_gt_table.restype = ctypes.c_void_p
    h.salt_gt_table.argtypes = []
    return h


def gt_table():
    """The penalty table of the genotype calls as the libraries hold it: (94, 3) uint32, per quality 0 .. 93 the penalties M, X, H in
    1 / 4096 Phred (SALT_GT_TABLE of include/salt_gt_table.h)."""
    h = _gt_host()
    return np.ctypeslib.as_array(ctypes.cast(h.salt_gt_table(), ctypes.POINTER(ctypes.c_uint32)), shape=(94, 3)).copy()


def gt_add_sam(index, sam, min_mapq=0, sums=None):
    """The genotype sums of this program's own SAM text (salt_gt_add_sam, the host twin of the device's k_gt_add): (n_sites, 4, 4) uint64,
    per site and base A C G T the words n, sm, sx, sh.  sums: the array of an earlier call to add into.  Returns (sums, records that counted)."""
    h = _gt_host()
    sam = bytes(sam)
    n_sites = h.salt_snp_sites(index._h, None, 0)
    if sums is None:
        sums = np.zeros((n_sites, 4, 4), dtype=np.uint64)
    if sums.dtype != np.uint64 or sums.shape != (n_sites, 4, 4) or not sums.flags.c_contiguous:
        raise SaltError("gt_add_sam: sums must be a contiguous (%d, 4, 4) uint64 array" % n_sites)
    n = h.salt_gt_add_sam(index._h, sam, len(sam), int(min_mapq), sums.ctypes.data, n_sites)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    return sums, int(n)


def gt_text(index, sums, first=0):
    """The VCF records of sites [first, first + len(sums)) for the sums given (salt_gt_text, the host twin of the device's call and text
    kernels; no header).  bytes."""
    h = _gt_host()
    sums = np.ascontiguousarray(sums, dtype=np.uint64)
    if sums.ndim != 3 or sums.shape[1:] != (4, 4):
        raise SaltError("gt_text: sums of shape (n, 4, 4)")
    n = h.salt_gt_text(index._h, sums.ctypes.data, int(first), sums.shape[0], None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    if h.salt_gt_text(index._h, sums.ctypes.data, int(first), sums.shape[0], out, n) != n:
        raise SaltError("gt_text: the size of the text changed between two calls")
    return out.raw[:n]


def gt_header(index, sample=None):
    """The header of `salt --genotype`'s file (salt_gt_header).  bytes."""
    h = _gt_host()
    name = None if sample is None else os.fsencode(sample)
    n = h.salt_gt_header(index._h, name, None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    h.salt_gt_header(index._h, name, out, n)
    return out.raw[:n]


DISC_ALT, DISC_DIFF = 0, 1              # the two arrays of the SNP candidates (SALT_DISC_ALT, SALT_DISC_DIFF)
DISC_FIELD_BITS = 21                    # alt: three fields of 21 bits a position
DISC_DEFAULTS = dict(min_mapq=20, min_baseq=20, min_alt=3, min_pct=20)


def _disc_host():
    h = host_lib()
    h.salt_disc_add_sam.restype = ctypes.c_int64
    h.salt_disc_add_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_disc_text.restype = ctypes.c_int64
    h.salt_disc_text.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return h


def disc_add_sam(index, sam, min_mapq=20, min_baseq=20, alt=None, diff=None):
    """The candidate arrays of this program's own SAM text (salt_disc_add_sam, the host twin of the device's k_disc_add): alt, uint64[ref_len]
    of three 21-bit fields a position, and diff, the tally's own uint32[ref_len + 1] difference array.  alt, diff: the arrays of an earlier
    call to add into.  Returns (alt, diff, records that counted)."""
    h = _disc_host()
    sam = bytes(sam)
    n_pos = int(index.ref_len)
    if alt is None:
        alt = np.zeros(n_pos, dtype=np.uint64)
    if diff is None:
        diff = np.zeros(n_pos + 1, dtype=np.uint32)
    if alt.dtype != np.uint64 or alt.shape != (n_pos,) or not alt.flags.c_contiguous or diff.dtype != np.uint32 or diff.shape != (n_pos + 1,) or not diff.flags.c_contiguous:
        raise SaltError("disc_add_sam: alt must be a contiguous (%d,) uint64 array and diff a contiguous (%d,) uint32 array" % (n_pos, n_pos + 1))
    n = h.salt_disc_add_sam(index._h, sam, len(sam), int(min_mapq), int(min_baseq), alt.ctypes.data, diff.ctypes.data, n_pos)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    return alt, diff, int(n)


def disc_text(index, alt, diff, min_alt=3, min_pct=20, all_sites=False, seen=False):
    """The candidate lines of the two arrays (salt_disc_text, the host twin of the device's flag and line kernels).  bytes; with seen=True
    (bytes, a uint8 per sequence of the index: it has a line)."""
    h = _disc_host()
    alt = np.ascontiguousarray(alt, dtype=np.uint64)
    diff = np.ascontiguousarray(diff, dtype=np.uint32)
    if alt.ndim != 1 or diff.shape != (alt.shape[0] + 1,):
        raise SaltError("disc_text: alt of shape (n,) and diff of shape (n + 1,)")
    n_seqs = host_lib().salt_index_n_seqs(index._h)
    marks = np.zeros(max(n_seqs, 1), dtype=np.uint8)
    args = (index._h, alt.ctypes.data, diff.ctypes.data, alt.shape[0], int(min_alt), int(min_pct), 1 if all_sites else 0)
    n = h.salt_disc_text(*args, None, 0, None)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    if h.salt_disc_text(*args, out, n, marks.ctypes.data) != n:
        raise SaltError("disc_text: the size of the text changed between two calls")
    return (out.raw[:n], marks[:n_seqs]) if seen else out.raw[:n]


INDEL_DEFAULTS = dict(min_mapq=20, min_alt=3, min_pct=20, log2_slots=24)
INDEL_STATS = ("tabled", "dropped", "long", "unanchored")      # the four counters (SALT_INDEL_TABLED ..)
INDEL_PROBE, INDEL_MAX_INS, INDEL_MAX_DEL, INDEL_MAX_SHIFT = 128, 12, 63, 4096


def _indel_host():
    h = host_lib()
    h.salt_indel_new.restype = ctypes.c_void_p
    h.salt_indel_free.argtypes = [ctypes.c_void_p]
    h.salt_indel_free.restype = None
    h.salt_indel_add_sam.restype = ctypes.c_int64
    h.salt_indel_add_sam.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_indel_entries.restype = ctypes.c_int64
    h.salt_indel_entries.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_indel_stats.restype = None
    h.salt_indel_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    h.salt_indel_text.restype = ctypes.c_int64
    h.salt_indel_text.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    h.salt_indel_header.restype = ctypes.c_int64
    h.salt_indel_header.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    return h


def indel_add_sam(index, sam, min_mapq=20):
    """The indel table of this program's own SAM text (salt_indel_add_sam, the host twin of the device's k_indel_add).  sam: bytes, or a
    list of texts that are added one after the other into one table.  Returns (entries, diff, stats, records that counted): entries a
    uint64 (n, 2) array of (key, value) pairs in key order, diff the tally's own uint32[ref_len + 1] difference array, stats the four
    counters INDEL_STATS."""
    h = _indel_host()
    n_pos = int(index.ref_len)
    diff = np.zeros(n_pos + 1, dtype=np.uint32)
    t = h.salt_indel_new()
    try:
        n_rec = 0
        for text in ([sam] if isinstance(sam, (bytes, bytearray, memoryview)) else sam):
            text = bytes(text)
            n = h.salt_indel_add_sam(index._h, t, text, len(text), int(min_mapq), diff.ctypes.data, n_pos)
            if n < 0:
                raise SaltError(h.salt_host_last_error().decode())
            n_rec += int(n)
        n = h.salt_indel_entries(t, None, 0)
        entries = np.zeros((max(n, 0), 2), dtype=np.uint64)
        if n < 0 or h.salt_indel_entries(t, entries.ctypes.data, n) != n:
            raise SaltError("indel_add_sam: the entries changed between two calls")
        stats = np.zeros(4, dtype=np.uint64)
        h.salt_indel_stats(t, stats.ctypes.data)
    finally:
        h.salt_indel_free(t)
    return entries, diff, stats, n_rec


def indel_text(index, entries, diff, min_alt=3, min_pct=20):
    """The VCF records of (key, value) pairs in key order and a difference array (salt_indel_text, the host twin of the device's text kernels)."""
    h = _indel_host()
    entries = np.ascontiguousarray(entries, dtype=np.uint64).reshape(-1, 2)
    diff = np.ascontiguousarray(diff, dtype=np.uint32)
    if diff.ndim != 1 or diff.shape[0] < 1:
        raise SaltError("indel_text: diff of shape (ref_len + 1,)")
    args = (index._h, entries.ctypes.data, entries.shape[0], diff.ctypes.data, diff.shape[0] - 1, int(min_alt), int(min_pct))
    n = h.salt_indel_text(*args, None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    if h.salt_indel_text(*args, out, n) != n:
        raise SaltError("indel_text: the size of the text changed between two calls")
    return out.raw[:n]


def indel_header(index, min_mapq=20, min_alt=3, min_pct=20, dropped=0):
    """The header of the `--indels` file (salt_indel_header)."""
    h = _indel_host()
    args = (index._h, int(min_mapq), int(min_alt), int(min_pct), int(dropped))
    n = h.salt_indel_header(*args, None, 0)
    if n < 0:
        raise SaltError(h.salt_host_last_error().decode())
    out = ctypes.create_string_buffer(max(n, 1))
    if h.salt_indel_header(*args, out, n) != n:
        raise SaltError("indel_header: the size of the text changed between two calls")
    return out.raw[:n]


TRIM_COUNTERS = ("reads", "bases_in", "bases_out", "reads_qual", "bases_qual", "reads_adapter", "bases_adapter", "reads_floored")


class _TrimOpt(ctypes.Structure):
    _fields_ = [("adapter", ctypes.c_char_p), ("adapter_len", ctypes.c_uint32), ("adapter2", ctypes.c_char_p), ("adapter2_len", ctypes.c_uint32),
                ("front", ctypes.c_uint32), ("tail", ctypes.c_uint32), ("qual", ctypes.c_uint32), ("min_overlap", ctypes.c_uint32),
                ("error_pct", ctypes.c_uint32)]


def _trim_opt(adapter, adapter2, qual, front, tail, min_overlap, error_pct):
    """salt_trim_opt_t; min_overlap and error_pct belong to the adapter and are left out without one"""
    a = adapter.encode() if isinstance(adapter, str) else adapter
    a2 = adapter2.encode() if isinstance(adapter2, str) else adapter2
    for v in (qual, front, tail, min_overlap, error_pct):
        if not 0 <= int(v) < 2 ** 32:
            raise SaltError("trim: a number outside 0 .. 2^32 - 1")
    return _TrimOpt(a or None, len(a) if a else 0, a2 or None, len(a2) if a2 else 0, int(front), int(tail), int(qual),
                    int(min_overlap) if a else 0, int(error_pct) if a else 0)


def _host_trim():
    lib = host_lib()
    lib.salt_trim_span.argtypes = [ctypes.POINTER(_TrimOpt), ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                   ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p]
    lib.salt_trim_fastq.restype = ctypes.c_int64
    lib.salt_trim_fastq.argtypes = [ctypes.POINTER(_TrimOpt), ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def trim_span(seq, qual, mate=0, adapter=None, adapter2=None, qual_min=0, front=0, tail=0, min_overlap=5, error_pct=10, counts=None):
    """The host twin of k_fq_trim on one read (salt_trim_span): -> (beg, end).  qual_min is set_trim's `qual` (qual here is the read's
    quality string).  counts: a (2, 8) uint64 array the read's counters are added to."""
    lib, o = _host_trim(), _trim_opt(adapter, adapter2, qual_min, front, tail, min_overlap, error_pct)
    seq, qual = bytes(seq), bytes(qual)
    if len(seq) != len(qual):
        raise SaltError("trim: sequence and quality lengths differ")
    if counts is not None and (counts.dtype != np.uint64 or counts.shape != (2, 8) or not counts.flags.c_contiguous):
        raise SaltError("trim: counts is a C-contiguous (2, 8) uint64 array")
    b, e = ctypes.c_uint32(), ctypes.c_uint32()
    if lib.salt_trim_span(ctypes.byref(o), int(mate), seq, qual, len(seq), ctypes.byref(b), ctypes.byref(e), counts.ctypes.data if counts is not None else None) != 0:
        raise SaltError(lib.salt_host_last_error().decode())
    return b.value, e.value


def trim_fastq(fastq, mate=0, adapter=None, adapter2=None, qual=0, front=0, tail=0, min_overlap=5, error_pct=10, counts=None):
    """A block of 4-line FASTQ trimmed on the host (salt_trim_fastq): the reads `salt --trim-*` aligns, as FASTQ."""
    lib, o = _host_trim(), _trim_opt(adapter, adapter2, qual, front, tail, min_overlap, error_pct)
    fastq = bytes(fastq)
    if counts is not None and (counts.dtype != np.uint64 or counts.shape != (2, 8) or not counts.flags.c_contiguous):
        raise SaltError("trim: counts is a C-contiguous (2, 8) uint64 array")
    out = ctypes.create_string_buffer(len(fastq) + 1)
    n = lib.salt_trim_fastq(ctypes.byref(o), int(mate), fastq, len(fastq), out, len(fastq), counts.ctypes.data if counts is not None else None)
    if n < 0:
        raise SaltError(lib.salt_host_last_error().decode())
    return out.raw[:n]


TRIM_PAIR_COUNTERS = ("pairs", "overlapping", "trimmed", "reads1", "bases1", "reads2", "bases2", "skipped_long")


class _TrimPairOpt(ctypes.Structure):
    _fields_ = [("min_overlap", ctypes.c_uint32), ("error_pct", ctypes.c_uint32)]


def _trim_pair_opt(min_overlap, error_pct):
    """salt_trim_pair_opt_t of a rule that is on (all zero would switch it off, so a min_overlap of 0 is refused here)"""
    for v in (min_overlap, error_pct):
        if not 0 <= int(v) < 2 ** 32:
            raise SaltError("trim pair: a number outside 0 .. 2^32 - 1")
    if int(min_overlap) == 0:
        raise SaltError("trim pair: min_overlap outside 1 .. 512")
    return _TrimPairOpt(int(min_overlap), int(error_pct))


def _pair_args(pair, min_overlap, error_pct, adapter, adapter2, qual, front, tail, a_min_overlap, a_error_pct, counts, pair_counts):
    lib = _host_trim()
    o = _trim_opt(adapter, adapter2, qual, front, tail, a_min_overlap, a_error_pct)
    po = _trim_pair_opt(min_overlap, error_pct) if pair else _TrimPairOpt(0, 0)
    if counts is not None and (counts.dtype != np.uint64 or counts.shape != (2, 8) or not counts.flags.c_contiguous):
        raise SaltError("trim: counts is a C-contiguous (2, 8) uint64 array")
    if pair_counts is not None and (pair_counts.dtype != np.uint64 or pair_counts.shape != (8,) or not pair_counts.flags.c_contiguous):
        raise SaltError("trim pair: pair_counts is a C-contiguous (8,) uint64 array")
    return lib, o, po, counts.ctypes.data if counts is not None else None, pair_counts.ctypes.data if pair_counts is not None else None


def trim_pair_span(seq1, qual1, seq2, qual2, pair=True, min_overlap=20, error_pct=10, adapter=None, adapter2=None, qual_min=0, front=0, tail=0,
                   adapter_min_overlap=5, adapter_error_pct=10, counts=None, pair_counts=None):
    """The host twin of k_fq_trim_pair on one pair (salt_trim_pair_span): -> (b1, e1, b2, e2).  min_overlap and error_pct are the pair
    rule's (pair=False: the rule off); the adapter step's are adapter_min_overlap and adapter_error_pct.  counts: a (2, 8) uint64 array,
    pair_counts: an (8,) one, to which the pair's counters are added."""
    lib, o, po, c, pc = _pair_args(pair, min_overlap, error_pct, adapter, adapter2, qual_min, front, tail, adapter_min_overlap, adapter_error_pct, counts, pair_counts)
    seq1, qual1, seq2, qual2 = bytes(seq1), bytes(qual1), bytes(seq2), bytes(qual2)
    if len(seq1) != len(qual1) or len(seq2) != len(qual2):
        raise SaltError("trim pair: sequence and quality lengths differ")
    span = (ctypes.c_uint32 * 4)()
    lib.salt_trim_pair_span.argtypes = [ctypes.POINTER(_TrimOpt), ctypes.POINTER(_TrimPairOpt), ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p,
                                        ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    if lib.salt_trim_pair_span(ctypes.byref(o), ctypes.byref(po), seq1, qual1, len(seq1), seq2, qual2, len(seq2), span, c, pc) != 0:
        raise SaltError(lib.salt_host_last_error().decode())
    return tuple(span)


def trim_fastq_pair(fastq1, fastq2, pair=True, min_overlap=20, error_pct=10, adapter=None, adapter2=None, qual=0, front=0, tail=0,
                    adapter_min_overlap=5, adapter_error_pct=10, counts=None, pair_counts=None):
    """Two blocks of 4-line FASTQ trimmed on the host as pairs (salt_trim_fastq_pair): -> (block1, block2), the reads
    `salt --trim-pair-overlap` aligns, as FASTQ."""
    lib, o, po, c, pc = _pair_args(pair, min_overlap, error_pct, adapter, adapter2, qual, front, tail, adapter_min_overlap, adapter_error_pct, counts, pair_counts)
    fastq1, fastq2 = bytes(fastq1), bytes(fastq2)
    out1, out2 = ctypes.create_string_buffer(len(fastq1) + 1), ctypes.create_string_buffer(len(fastq2) + 1)
    w1, w2 = ctypes.c_uint64(), ctypes.c_uint64()
    lib.salt_trim_fastq_pair.argtypes = [ctypes.POINTER(_TrimOpt), ctypes.POINTER(_TrimPairOpt), ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64,
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_uint64,
                                         ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.c_void_p]
    if lib.salt_trim_fastq_pair(ctypes.byref(o), ctypes.byref(po), fastq1, len(fastq1), fastq2, len(fastq2), out1, len(fastq1), ctypes.byref(w1),
                                out2, len(fastq2), ctypes.byref(w2), c, pc) != 0:
        raise SaltError(lib.salt_host_last_error().decode())
    return out1.raw[:w1.value], out2.raw[:w2.value]


class _IndelTextOpt(ctypes.Structure):
    _fields_ = [("min_alt", ctypes.c_uint32), ("min_pct", ctypes.c_uint32), ("tile_positions", ctypes.c_uint32), ("bgzf", ctypes.c_int32)]


class _DiscTextOpt(ctypes.Structure):
    _fields_ = [("min_alt", ctypes.c_uint32), ("min_pct", ctypes.c_uint32), ("all_sites", ctypes.c_int32), ("tile_positions", ctypes.c_uint32), ("bgzf", ctypes.c_int32)]


class _GtTextOpt(ctypes.Structure):
    _fields_ = [("tile_sites", ctypes.c_uint32), ("bgzf", ctypes.c_int32)]


class _DepthTextOpt(ctypes.Structure):
    _fields_ = [("window", ctypes.c_uint32), ("tile_positions", ctypes.c_uint32), ("bgzf", ctypes.c_int32)]


class _TextOpt(ctypes.Structure):
    _fields_ = [("print_xa_cigar", ctypes.c_int32), ("print_nm_md", ctypes.c_int32), ("rg_id", ctypes.c_char_p)]


KERNELS = ("k_pack", "k_seed", "k_light", "k_heavy", "k_gap", "k_gapfin", "k_cigar", "k_pair", "k_sw", "k_pe_final")

PACK_FILL = 0x5A5A5A5A      # what diag_pack's buffers hold where k_pack wrote nothing


def pack_geom(max_read_len):
    """PackGeom::make (salt_kernels.h): the word counts and strides of k_pack's records for reads of up to max_read_len bases."""
    m = max(1, int(max_read_len))
    nw8, nw16, nw32 = (m + 7) // 8, (m + 15) // 16, (m + 31) // 32
    return {"nw8": nw8, "nw16": nw16, "nw32": nw32, "pm_stride": (2 * nw8 + 1 + 3) & ~3, "tb_stride": (2 * nw16 + 2 * nw32 + 1 + 3) & ~3}


def diag_pack(n_reads, max_read_len, d_seqs, d_offs, byte_offset=0, stream=0):
    """k_pack alone (salt_gpu_diag_pack) on torch tensors of one GPU: the reads' uint8 codes start byte_offset bytes into d_seqs, d_offs
    n_reads + 1 int32 offsets from there -> (pack_geom(max_read_len), pm (n_reads, pm_stride), tb (n_reads, tb_stride)) as int64 numpy
    arrays of the uint32 words; words the kernel did not write hold PACK_FILL."""
    import torch
    lib = gpu_lib()
    g = pack_geom(max_read_len)
    dev = d_seqs.device
    fill = PACK_FILL - (1 << 32) if PACK_FILL >= 1 << 31 else PACK_FILL
    pm = torch.full((max(n_reads, 1), g["pm_stride"]), fill, dtype=torch.int32, device=dev)
    tb = torch.full((max(n_reads, 1), g["tb_stride"]), fill, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _gpu_check(lib.salt_gpu_diag_pack(dev.index or 0, n_reads, max_read_len, d_seqs.data_ptr() + byte_offset, d_offs.data_ptr(), pm.data_ptr(), tb.data_ptr(), stream))
    torch.cuda.synchronize(dev)
    u = lambda t: t[:n_reads].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    return g, u(pm), u(tb)


class GpuAligner:
    """Device copy of the index + one batch workspace on one GPU."""

    def __init__(self, index=None, device=0, max_reads=100000, max_bases=None, image=None, compact=None):
        """index: a host Index to re-pack and upload; or image=(device_ptr, bytes): an already packed full
        device image that stays owned by the caller; or compact=(device_ptr, bytes): the compact part of an image
        (e.g. received by an RCCL broadcast), from which this device builds its own full image."""
        lib = gpu_lib()
        self._ix = ctypes.c_void_p()
        if compact is not None:
            _gpu_check(lib.salt_gpu_index_attach_compact(compact[0], compact[1], device, ctypes.byref(self._ix)))
        elif image is not None:
            _gpu_check(lib.salt_gpu_index_attach_image(image[0], image[1], device, ctypes.byref(self._ix)))
        else:
            _gpu_check(lib.salt_gpu_index_attach(index.view, device, ctypes.byref(self._ix)))
        self._ws = ctypes.c_void_p()
        self.max_reads = max_reads
        self.max_bases = max_bases if max_bases is not None else max_reads * 160
        try:
            _gpu_check(lib.salt_gpu_ws_create(self._ix, max_reads, self.max_bases, ctypes.byref(self._ws)))
        except SaltError:
            lib.salt_gpu_index_detach(self._ix)
            raise
        self.device = device

    def image(self):
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _gpu_check(gpu_lib().salt_gpu_index_image(self._ix, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def pe_counts(self):
        """Counters of the last paired batch: [0] rescue requests, [2] CIGAR items, [4] overflowed rescues."""
        out = (ctypes.c_uint32 * 8)()
        _gpu_check(gpu_lib().salt_gpu_ws_pe_counts(self._ws, out))
        return list(out)

    def image_compact(self):
        """(device pointer, bytes) of the part of the image a multi-GPU driver broadcasts (everything but the W-mer table)."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _gpu_check(gpu_lib().salt_gpu_index_image_compact(self._ix, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def image_copy(self, dst_ptr, dst_bytes):
        _gpu_check(gpu_lib().salt_gpu_index_image_copy(self._ix, dst_ptr, dst_bytes))

    def timing(self, enable=True):
        _gpu_check(gpu_lib().salt_gpu_ws_timing(self._ws, 1 if enable else 0))

    def kernel_ms(self):
        """({kernel: ms summed since the last read}, calls)."""
        ms = (ctypes.c_double * len(KERNELS))()
        n = ctypes.c_uint32()
        _gpu_check(gpu_lib().salt_gpu_ws_kernel_ms(self._ws, ms, ctypes.byref(n)))
        return dict(zip(KERNELS, list(ms))), n.value

    def queue_counts(self):
        out = (ctypes.c_uint32 * 8)()
        _gpu_check(gpu_lib().salt_gpu_ws_queue_counts(self._ws, out))
        return list(out)

    def heavy_reads(self):
        """Indices (in the last batch) of the reads k_light queued for k_heavy."""
        n = ctypes.c_uint32()
        ids = np.zeros(self.max_reads, dtype=np.uint32)
        _gpu_check(gpu_lib().salt_gpu_ws_heavy_reads(self._ws, ids.ctypes.data, len(ids), ctypes.byref(n)))
        return ids[:n.value]

    def alnse_core1(self, opt, seqs, offs):
        """seqs: uint8 codes 0..4 concatenated; offs: uint32 n+1 offsets.  Returns RESULT_DTYPE[n]."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        n = len(offs) - 1
        res = np.zeros(n, dtype=RESULT_DTYPE)
        co = opt._c()
        done = 0
        while done < n:                                   # batches of the workspace size (N_SEQS, aln.h:27)
            m = min(self.max_reads, n - done)
            while m > 1 and int(offs[done + m]) - int(offs[done]) > self.max_bases:
                m //= 2
            o = (offs[done:done + m + 1] - offs[done]).astype(np.uint32)
            s = seqs[int(offs[done]):int(offs[done + m])]
            self._quals_for(int(offs[done]), int(offs[done + m]))
            _gpu_check(gpu_lib().salt_gpu_align_se(self._ws, ctypes.byref(co), m, s.ctypes.data, o.ctypes.data,
                                                   res[done:].ctypes.data))
            done += m
        self._quals = None
        return res

    def alnpe_core1(self, opt, index, seqs, offs):
        """Paired end: mates interleaved (pair i = reads 2i, 2i+1).  Returns RESULT_DTYPE[2 * n_pairs]."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint32)
        n = len(offs) - 1
        if n % 2:
            raise SaltError("paired end needs an even number of reads")
        lib = gpu_lib()
        if not getattr(self, "_pac_set", False):
            pac, l_pac = index.pac()
            _gpu_check(lib.salt_gpu_index_set_pac(self._ix, pac, l_pac))
            self._pac_set = True
        res = np.zeros(n, dtype=RESULT_DTYPE)
        co, pe = opt._c(), opt._pe()
        done = 0
        cap = self.max_reads & ~1
        while done < n:
            m = min(cap, n - done)
            while m > 2 and int(offs[done + m]) - int(offs[done]) > self.max_bases:
                m = (m // 2) & ~1
            o = (offs[done:done + m + 1] - offs[done]).astype(np.uint32)
            s = seqs[int(offs[done]):int(offs[done + m])]
            self._quals_for(int(offs[done]), int(offs[done + m]))
            _gpu_check(lib.salt_gpu_align_pe(self._ws, ctypes.byref(co), ctypes.byref(pe), m // 2, s.ctypes.data,
                                             o.ctypes.data, res[done:].ctypes.data))
            done += m
        self._quals = None
        return res

    def r_ctx(self):
        """(device pointer or None, bytes) of the R rows' context table of this aligner's index."""
        lib = gpu_lib()
        lib.salt_gpu_index_r_ctx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _gpu_check(lib.salt_gpu_index_r_ctx(self._ix, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def diag_occ(self, mode, queries):
        """The rank primitives asked directly (salt_gpu_diag_occ): mode "C" or "R", queries (n, 3) uint32 rows (x, y, c) -> (n, 12) uint32."""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, 3)
        out = np.zeros((len(q), 12), dtype=np.uint32)
        _gpu_check(gpu_lib().salt_gpu_diag_occ(self._ix, {"C": 0, "R": 1}[mode], len(q), q.ctypes.data, out.ctypes.data))
        return out

    def epoch(self):
        """The epoch the workspace's next alignment call runs at."""
        lib = gpu_lib()
        lib.salt_gpu_ws_epoch.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        e = ctypes.c_uint32()
        _gpu_check(lib.salt_gpu_ws_epoch(self._ws, ctypes.byref(e)))
        return e.value

    def set_pac(self, index):
        """Uploads the 2-bit genome the singleton rescue aligns against (once per device index; forks made afterwards share it)."""
        if not getattr(self, "_pac_set", False):
            pac, l_pac = index.pac()
            _gpu_check(gpu_lib().salt_gpu_index_set_pac(self._ix, pac, l_pac))
            self._pac_set = True

    def set_contigs(self, index):
        """The contig table the text entry points print RNAME / POS from (once per device index)."""
        cs = index.contigs()
        offs = (ctypes.c_int64 * len(cs))(*[c[0] for c in cs])
        names = (ctypes.c_char_p * len(cs))(*[c[2] for c in cs])
        lib = gpu_lib()
        lib.salt_gpu_index_set_contigs.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_index_set_contigs(self._ix, len(cs), offs, names))
        self._ix_state()["n_contigs"] = len(cs)

    def _ix_state(self):
        """what Python remembers of the device index, shared with the forks"""
        if not hasattr(self, "_ix_shared"):
            self._ix_shared = {}
        return self._ix_shared

    def set_sam_bgzf(self, on=True):
        """The text entry points return BGZF blocks (deflated on the device) instead of the bytes themselves."""
        gpu_lib().salt_gpu_ws_set_sam_bgzf.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _gpu_check(gpu_lib().salt_gpu_ws_set_sam_bgzf(self._ws, 1 if on else 0))

    def set_sam_bam(self, on=True):
        """The text entry points write BAM records (k_bam_len / k_bam_write) instead of SAM lines."""
        gpu_lib().salt_gpu_ws_set_sam_bam.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _gpu_check(gpu_lib().salt_gpu_ws_set_sam_bam(self._ws, 1 if on else 0))

    def set_polish(self, mode):
        """The text entry points return the records `polish` makes of the block's SAM lines instead of the lines themselves, straight from
        the result rows: mode 0 off, 1 (or "lv") Landau-Vishkin re-scoring, 2 (or "sw") Smith-Waterman.  Needs set_pac and set_contigs
        first; excludes set_sam_bam."""
        mode = {"off": 0, "lv": 1, "sw": 2}.get(mode, mode)
        gpu_lib().salt_gpu_ws_set_polish.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _gpu_check(gpu_lib().salt_gpu_ws_set_polish(self._ws, int(mode)))

    def set_trim(self, adapter=None, adapter2=None, qual=0, front=0, tail=0, min_overlap=5, error_pct=10):
        """The text entry points trim every read on the device (k_fq_trim) in front of the aligner: fixed clips, the 3' quality rule of
        `bwa aln -q`, a 3' adapter by Hamming overlap (adapter2: mate 2's own), never below one base.  Without arguments: off."""
        o = _trim_opt(adapter, adapter2, qual, front, tail, min_overlap, error_pct)
        gpu_lib().salt_gpu_ws_set_trim.argtypes = [ctypes.c_void_p, ctypes.POINTER(_TrimOpt)]
        _gpu_check(gpu_lib().salt_gpu_ws_set_trim(self._ws, ctypes.byref(o)))

    def trim_counts(self, reset=False):
        """(2, 8) uint64: per mate TRIM_COUNTERS, summed over this workspace's calls."""
        out = np.zeros((2, 8), dtype=np.uint64)
        gpu_lib().salt_gpu_ws_trim_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        _gpu_check(gpu_lib().salt_gpu_ws_trim_counts(self._ws, out.ctypes.data, 1 if reset else 0))
        return out

    def trim_uncount(self):
        """Takes back what this aligner's last text call (or trim_spans) added to trim_counts."""
        gpu_lib().salt_gpu_ws_trim_uncount.argtypes = [ctypes.c_void_p]
        _gpu_check(gpu_lib().salt_gpu_ws_trim_uncount(self._ws))

    def trim_spans(self, fastq, mate=0):
        """The parser and k_fq_trim alone on one block of 4-line FASTQ: (records, 2) uint32, the span (beg, end) of every record."""
        fastq = bytes(fastq)
        out = np.zeros((fastq.count(b"\n") // 4 + 1, 2), dtype=np.uint32)
        gpu_lib().salt_gpu_trim_spans.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
        _gpu_check(gpu_lib().salt_gpu_trim_spans(self._ws, fastq, len(fastq), int(mate), out.ctypes.data))
        return out[:-1]

    def set_trim_pair(self, min_overlap=20, error_pct=10):
        """align_pe_text finds each pair's adapters from the mates' overlap (step 2p of the trimming rule, k_fq_trim_pair) and cuts both
        mates at the insert's end.  Without arguments: on with the defaults; set_trim_pair(None): off."""
        o = _TrimPairOpt(0, 0) if min_overlap is None else _trim_pair_opt(min_overlap, error_pct)
        gpu_lib().salt_gpu_ws_set_trim_pair.argtypes = [ctypes.c_void_p, ctypes.POINTER(_TrimPairOpt)]
        _gpu_check(gpu_lib().salt_gpu_ws_set_trim_pair(self._ws, ctypes.byref(o)))

    def trim_pair_counts(self, reset=False):
        """(8,) uint64: TRIM_PAIR_COUNTERS, summed over this workspace's calls."""
        out = np.zeros(8, dtype=np.uint64)
        gpu_lib().salt_gpu_ws_trim_pair_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        _gpu_check(gpu_lib().salt_gpu_ws_trim_pair_counts(self._ws, out.ctypes.data, 1 if reset else 0))
        return out

    def trim_pair_spans(self, fastq1, fastq2):
        """The parser and k_fq_trim_pair alone on two blocks of 4-line FASTQ: (pairs, 4) uint32, (b1, e1, b2, e2) of every pair."""
        fastq1, fastq2 = bytes(fastq1), bytes(fastq2)
        out = np.zeros((max(fastq1.count(b"\n"), fastq2.count(b"\n")) // 4 + 1, 4), dtype=np.uint32)
        gpu_lib().salt_gpu_trim_pair_spans.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p]
        _gpu_check(gpu_lib().salt_gpu_trim_pair_spans(self._ws, fastq1, len(fastq1), fastq2, len(fastq2), out.ctypes.data))
        return out[:-1]

    def align_se_text(self, opt, fastq):
        """One block of whole 4-line FASTQ records -> (the block's SAM lines, or what set_sam_bam / set_sam_bgzf make of them; reads)."""
        lib = gpu_lib()
        lib.salt_gpu_align_se_text.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlnOpt), ctypes.POINTER(_TextOpt), ctypes.c_char_p, ctypes.c_uint64,
                                               ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        fastq = bytes(fastq)
        co, to = opt._c(), _TextOpt(opt.print_xa_cigar, opt.print_nm_md, opt.rg_id.encode() if opt.rg_id else None)
        out, n, reads = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
        _gpu_check(lib.salt_gpu_align_se_text(self._ws, ctypes.byref(co), ctypes.byref(to), fastq, len(fastq), ctypes.byref(out), ctypes.byref(n), ctypes.byref(reads)))
        return ctypes.string_at(out.value, n.value) if n.value else b"", reads.value

    def align_pe_text(self, opt, index, fastq1, fastq2):
        """Two blocks with the mates of the same pairs -> (both records of every pair in order; pairs)."""
        lib = gpu_lib()
        lib.salt_gpu_align_pe_text.argtypes = [ctypes.c_void_p, ctypes.POINTER(_AlnOpt), ctypes.POINTER(_PeOpt), ctypes.POINTER(_TextOpt), ctypes.c_char_p,
                                               ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                               ctypes.POINTER(ctypes.c_uint32)]
        self.set_pac(index)
        fastq1, fastq2 = bytes(fastq1), bytes(fastq2)
        co, pe, to = opt._c(), opt._pe(), _TextOpt(opt.print_xa_cigar, opt.print_nm_md, opt.rg_id.encode() if opt.rg_id else None)
        out, n, pairs = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
        _gpu_check(lib.salt_gpu_align_pe_text(self._ws, ctypes.byref(co), ctypes.byref(pe), ctypes.byref(to), fastq1, len(fastq1), fastq2, len(fastq2),
                                              ctypes.byref(out), ctypes.byref(n), ctypes.byref(pairs)))
        return ctypes.string_at(out.value, n.value) if n.value else b"", pairs.value

    def _text_rows(self, opt, paired, fastq1, fastq2, rows):
        lib = gpu_lib()
        lib.salt_gpu_diag_text_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(_TextOpt), ctypes.POINTER(_PeOpt), ctypes.c_char_p, ctypes.c_uint64,
                                                ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p),
                                                ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        rows = np.ascontiguousarray(rows, dtype=RESULT_DTYPE)
        fastq1, fastq2 = bytes(fastq1), bytes(fastq2)
        pe, to = opt._pe(), _TextOpt(opt.print_xa_cigar, opt.print_nm_md, opt.rg_id.encode() if opt.rg_id else None)
        out, n, recs = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32()
        _gpu_check(lib.salt_gpu_diag_text_rows(self._ws, ctypes.byref(to), ctypes.byref(pe) if paired else None, fastq1, len(fastq1), fastq2, len(fastq2),
                                               rows.ctypes.data if len(rows) else None, len(rows), ctypes.byref(out), ctypes.byref(n), ctypes.byref(recs)))
        return ctypes.string_at(out.value, n.value) if n.value else b"", recs.value

    def text_from_rows(self, opt, fastq, rows):
        """The text stage alone (salt_gpu_diag_text_rows): one FASTQ block and one RESULT_DTYPE row per record of it -> (what align_se_text
        would return had the aligner produced these rows; records).  The library refuses rows that lie outside the genome or the reads."""
        return self._text_rows(opt, False, fastq, b"", rows)

    def text_from_rows_pe(self, opt, index, fastq1, fastq2, rows):
        """The same for two blocks of mates: rows[2p], rows[2p + 1] are the mates of pair p -> (what align_pe_text would return; records,
        both mates counted)."""
        self.set_pac(index)
        return self._text_rows(opt, True, fastq1, fastq2, rows)

    def align_pe_resident(self, opt, index, n_pairs, max_read_len, d_seqs, d_offs, d_results, stream=0):
        lib = gpu_lib()
        self.set_pac(index)
        co, pe = opt._c(), opt._pe()
        _gpu_check(lib.salt_gpu_align_pe_resident(self._ws, ctypes.byref(co), ctypes.byref(pe), n_pairs, max_read_len, d_seqs, d_offs,
                                                  d_results, stream))

    def align_resident(self, opt, n_reads, max_read_len, d_seqs, d_offs, d_results, stream=0):
        co = opt._c()
        _gpu_check(gpu_lib().salt_gpu_align_se_resident(self._ws, ctypes.byref(co), n_reads, max_read_len, d_seqs, d_offs,
                                                        d_results, stream))

    def snp_enable(self, on=True, min_mapq=0):
        """Count, from now on, what every align call on this aligner's device index (its forks included) shows at the index's SNP sites;
        records below min_mapq do not count.  The first enable builds the site table and zeroes the counts; on=False stops and keeps both."""
        lib = gpu_lib()
        lib.salt_gpu_index_snp_enable.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
        _gpu_check(lib.salt_gpu_index_snp_enable(self._ix, 1 if on else 0, int(min_mapq)))

    def snp_sites(self):
        """The sites' genome positions from the device's table, ascending: uint32 array."""
        lib = gpu_lib()
        lib.salt_gpu_index_snp_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.c_uint64]
        n = ctypes.c_uint32()
        _gpu_check(lib.salt_gpu_index_snp_sites(self._ix, ctypes.byref(n), None, 0))
        pos = np.zeros(n.value, dtype=np.uint32)
        _gpu_check(lib.salt_gpu_index_snp_sites(self._ix, ctypes.byref(n), pos.ctypes.data, pos.size))
        return pos

    def snp_counts(self, reset=False):
        """(n_sites, 4) uint32: the adds of all align calls since the first enable or the last reset, A C G T.  Synchronises the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_snp_sites.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.c_uint64]
        lib.salt_gpu_index_snp_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
        n = ctypes.c_uint32()
        _gpu_check(lib.salt_gpu_index_snp_sites(self._ix, ctypes.byref(n), None, 0))
        counts = np.zeros((n.value, 4), dtype=np.uint32)
        _gpu_check(lib.salt_gpu_index_snp_counts(self._ix, counts.ctypes.data, counts.size, 1 if reset else 0))
        return counts

    def depth_enable(self, on=True, min_mapq=0):
        """Mark, from now on, the M runs of every align call on this aligner's device index (its forks included) in the index's coverage
        difference array; records below min_mapq do not count.  The first enable allocates and zeroes the array (4 bytes a genome
        position); on=False stops and keeps it."""
        lib = gpu_lib()
        lib.salt_gpu_index_depth_enable.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
        _gpu_check(lib.salt_gpu_index_depth_enable(self._ix, 1 if on else 0, int(min_mapq)))

    def depth_reset(self):
        lib = gpu_lib()
        lib.salt_gpu_index_depth_reset.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_index_depth_reset(self._ix))

    def depth_fetch(self, first, n):
        """diff[first .. first + n) of the device's difference array (ref_len + 1 words in all): uint32 array.  Synchronises the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_depth_fetch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        out = np.zeros(max(int(n), 0), dtype=np.uint32)
        _gpu_check(lib.salt_gpu_index_depth_fetch(self._ix, int(first), int(n), out.ctypes.data))
        return out

    def depth_add(self, first, words):
        """diff[first .. first + len(words)) += words, on the device: how the arrays of several GPUs are summed."""
        lib = gpu_lib()
        lib.salt_gpu_index_depth_add.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        words = np.ascontiguousarray(words, dtype=np.uint32)
        _gpu_check(lib.salt_gpu_index_depth_add(self._ix, int(first), words.size, words.ctypes.data))

    def depth_uncount(self):
        """Takes back what this aligner's last align call marked."""
        lib = gpu_lib()
        lib.salt_gpu_ws_depth_uncount.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_ws_depth_uncount(self._ws))

    def depth_text(self, window=0, tile_positions=0, bgzf=False, pieces=False):
        """The text of the difference array as it stands, made on the device: per-base bedGraph (window 0) or window means; with bgzf
        whole BGZF blocks (no end-of-file block).  pieces=True: the list of pieces as they left the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_depth_text_begin.argtypes = [ctypes.c_void_p, ctypes.POINTER(_DepthTextOpt)]
        lib.salt_gpu_index_depth_text_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        opt = _DepthTextOpt(int(window), int(tile_positions), 1 if bgzf else 0)
        _gpu_check(lib.salt_gpu_index_depth_text_begin(self._ix, ctypes.byref(opt)))
        out = []
        while True:
            p, n = ctypes.c_void_p(), ctypes.c_uint64()
            _gpu_check(lib.salt_gpu_index_depth_text_next(self._ix, ctypes.byref(p), ctypes.byref(n)))
            if n.value == 0:
                break
            out.append(ctypes.string_at(p.value, n.value))
        return out if pieces else b"".join(out)

    def gt_enable(self, on=True, min_mapq=0):
        """Add, from now on, the base and quality events of every align call on this aligner's device index (its forks included) to the
        index's genotype sums; records below min_mapq do not count.  The first enable builds the site table if snp_enable has not, and
        zeroes the sums (128 bytes a site); on=False stops and keeps them."""
        lib = gpu_lib()
        lib.salt_gpu_index_gt_enable.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
        _gpu_check(lib.salt_gpu_index_gt_enable(self._ix, 1 if on else 0, int(min_mapq)))

    def gt_reset(self):
        lib = gpu_lib()
        lib.salt_gpu_index_gt_reset.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_index_gt_reset(self._ix))

    def gt_fetch(self, first=0, n=None):
        """The sums of sites [first, first + n) (n None: all behind first): (n, 4, 4) uint64, per site and base A C G T the words n, sm, sx,
        sh.  Synchronises the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_gt_fetch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        if n is None:
            n = max(len(self.snp_sites()) - int(first), 0)
        out = np.zeros((max(int(n), 0), 4, 4), dtype=np.uint64)
        _gpu_check(lib.salt_gpu_index_gt_fetch(self._ix, int(first), int(n), out.ctypes.data))
        return out

    def gt_add(self, first, sums):
        """sums[first .. first + len(sums)) += sums, on the device: how the tables of several GPUs are summed."""
        lib = gpu_lib()
        lib.salt_gpu_index_gt_add.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        sums = np.ascontiguousarray(sums, dtype=np.uint64)
        if sums.ndim != 3 or sums.shape[1:] != (4, 4):
            raise SaltError("gt_add: sums of shape (n, 4, 4)")
        _gpu_check(lib.salt_gpu_index_gt_add(self._ix, int(first), sums.shape[0], sums.ctypes.data))

    def gt_uncount(self):
        """Takes back what this aligner's last align call added to the genotype sums."""
        lib = gpu_lib()
        lib.salt_gpu_ws_gt_uncount.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_ws_gt_uncount(self._ws))

    def gt_text(self, tile_sites=0, bgzf=False, pieces=False):
        """The VCF records of the sums as they stand, called and printed on the device (no header); with bgzf whole BGZF blocks (no
        end-of-file block).  pieces=True: the list of pieces as they left the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_gt_text_begin.argtypes = [ctypes.c_void_p, ctypes.POINTER(_GtTextOpt)]
        lib.salt_gpu_index_gt_text_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        opt = _GtTextOpt(int(tile_sites), 1 if bgzf else 0)
        _gpu_check(lib.salt_gpu_index_gt_text_begin(self._ix, ctypes.byref(opt)))
        out = []
        while True:
            p, n = ctypes.c_void_p(), ctypes.c_uint64()
            _gpu_check(lib.salt_gpu_index_gt_text_next(self._ix, ctypes.byref(p), ctypes.byref(n)))
            if n.value == 0:
                break
            out.append(ctypes.string_at(p.value, n.value))
        return out if pieces else b"".join(out)

    def disc_enable(self, on=True, min_mapq=20, min_baseq=20):
        """Add, from now on, every align call on this aligner's device index (its forks included) to the index's SNP candidate arrays: a
        base the mixRef does not have at its position, with a quality of at least min_baseq or none; records below min_mapq do not count.
        The first enable allocates and zeroes both arrays (12 bytes a genome position); on=False stops and keeps them."""
        lib = gpu_lib()
        lib.salt_gpu_index_disc_enable.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        _gpu_check(lib.salt_gpu_index_disc_enable(self._ix, 1 if on else 0, int(min_mapq), int(min_baseq)))

    def disc_reset(self):
        lib = gpu_lib()
        lib.salt_gpu_index_disc_reset.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_index_disc_reset(self._ix))

    def disc_fetch(self, which, first, n):
        """Words [first, first + n) of alt (which = DISC_ALT: uint64, ref_len words) or of diff (DISC_DIFF: uint32, ref_len + 1 words).
        Synchronises the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_disc_fetch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        out = np.zeros(max(int(n), 0), dtype=np.uint32 if which == DISC_DIFF else np.uint64)
        _gpu_check(lib.salt_gpu_index_disc_fetch(self._ix, int(which), int(first), int(n), out.ctypes.data))
        return out

    def disc_add(self, which, first, words):
        """array[first .. first + len(words)) += words, on the device: how the arrays of several GPUs are summed."""
        lib = gpu_lib()
        lib.salt_gpu_index_disc_add.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        words = np.ascontiguousarray(words, dtype=np.uint32 if which == DISC_DIFF else np.uint64)
        if words.ndim != 1:
            raise SaltError("disc_add: words of shape (n,)")
        _gpu_check(lib.salt_gpu_index_disc_add(self._ix, int(which), int(first), words.shape[0], words.ctypes.data))

    def disc_uncount(self):
        """Takes back what this aligner's last align call added to the SNP candidate arrays."""
        lib = gpu_lib()
        lib.salt_gpu_ws_disc_uncount.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_ws_disc_uncount(self._ws))

    def disc_text(self, min_alt=3, min_pct=20, all_sites=False, tile_positions=0, bgzf=False, pieces=False, seen=0):
        """The candidate lines of the arrays as they stand, flagged, compacted and printed on the device; with bgzf whole BGZF blocks (no
        end-of-file block).  pieces=True: the list of pieces as they left the device.  seen=N, the contigs' number: (that, a uint8 per contig: it has a line)."""
        lib = gpu_lib()
        lib.salt_gpu_index_disc_text_begin.argtypes = [ctypes.c_void_p, ctypes.POINTER(_DiscTextOpt)]
        lib.salt_gpu_index_disc_text_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        lib.salt_gpu_index_disc_text_seen.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        opt = _DiscTextOpt(int(min_alt), int(min_pct), 1 if all_sites else 0, int(tile_positions), 1 if bgzf else 0)
        _gpu_check(lib.salt_gpu_index_disc_text_begin(self._ix, ctypes.byref(opt)))
        out = []
        while True:
            p, n = ctypes.c_void_p(), ctypes.c_uint64()
            _gpu_check(lib.salt_gpu_index_disc_text_next(self._ix, ctypes.byref(p), ctypes.byref(n)))
            if n.value == 0:
                break
            out.append(ctypes.string_at(p.value, n.value))
        text = out if pieces else b"".join(out)
        if not seen:
            return text
        marks = np.zeros(int(seen), dtype=np.uint8)
        _gpu_check(lib.salt_gpu_index_disc_text_seen(self._ix, marks.ctypes.data, marks.shape[0]))
        return text, marks

    def errprof_enable(self, on=True, min_mapq=0):
        """Add, from now on, the base events of every align call on this aligner's device index (its forks included) to the index's error
        profile; records below min_mapq do not count.  The first enable allocates and zeroes the tables (12.45 MB); on=False stops and
        keeps them."""
        lib = gpu_lib()
        lib.salt_gpu_index_errprof_enable.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
        _gpu_check(lib.salt_gpu_index_errprof_enable(self._ix, 1 if on else 0, int(min_mapq)))

    def errprof_table(self, reset=False):
        """(E uint64 (2, 512, 95, 4, 4) indexed [mate][cycle][q][ref][read], R uint64 (2, 8)): the adds of all align calls since the
        first enable or the last reset.  Synchronises the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_errprof_fetch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int]
        E = np.zeros(ERRPROF_SHAPE, dtype=np.uint64)
        R = np.zeros((2, 8), dtype=np.uint64)
        _gpu_check(lib.salt_gpu_index_errprof_fetch(self._ix, E.ctypes.data, E.size, R.ctypes.data, 1 if reset else 0))
        return E, R

    def errprof_uncount(self):
        """Takes back what this aligner's last align call added to the error profile."""
        lib = gpu_lib()
        lib.salt_gpu_ws_errprof_uncount.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_ws_errprof_uncount(self._ws))

    def stats_enable(self, on=True, min_mapq=0):
        """Add, from now on, every align call on this aligner's device index (its forks included) to the index's summary tables (mapping
        counts, histograms, per-contig counts; salt_gpu.h); records below min_mapq are mapped but not counted.  The first enable
        allocates and zeroes the tables and needs set_contigs; on=False stops and keeps them."""
        lib = gpu_lib()
        lib.salt_gpu_index_stats_enable.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32]
        _gpu_check(lib.salt_gpu_index_stats_enable(self._ix, 1 if on else 0, int(min_mapq)))

    def stats_tables(self, reset=False):
        """(cells uint64 (6021,), ct uint64 (contigs, 8)): the adds of all align calls since the first enable or the last reset;
        stats_split names the tables inside cells.  Synchronises the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_stats_fetch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int]
        cells = np.zeros(STATS_CELLS, dtype=np.uint64)
        ct = np.zeros((self._ix_state().get("n_contigs", 0), 8), dtype=np.uint64)
        _gpu_check(lib.salt_gpu_index_stats_fetch(self._ix, cells.ctypes.data, cells.size, ct.ctypes.data if ct.size else None, ct.size, 1 if reset else 0))
        return cells, ct

    def stats_uncount(self):
        """Takes back what this aligner's last align call added to the summary tables."""
        lib = gpu_lib()
        lib.salt_gpu_ws_stats_uncount.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_ws_stats_uncount(self._ws))

    def indel_enable(self, on=True, min_mapq=20, log2_slots=0):
        """Add, from now on, the insertions and deletions of every align call on this aligner's device index (its forks included) to the
        index's table of allele keys, left-normalised; records below min_mapq do not count.  The first enable allocates and zeroes the
        table (2^log2_slots slots of 16 bytes; 0: the default, 2^24), the counters and the difference array and needs set_contigs;
        on=False stops and keeps them."""
        lib = gpu_lib()
        lib.salt_gpu_index_indel_enable.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        _gpu_check(lib.salt_gpu_index_indel_enable(self._ix, 1 if on else 0, int(min_mapq), int(log2_slots)))

    def indel_reset(self):
        lib = gpu_lib()
        lib.salt_gpu_index_indel_reset.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_index_indel_reset(self._ix))

    def indel_stats(self):
        """The four counters INDEL_STATS, uint64 (4,).  Synchronises the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_indel_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        out = np.zeros(4, dtype=np.uint64)
        _gpu_check(lib.salt_gpu_index_indel_stats(self._ix, out.ctypes.data))
        return out

    def indel_fetch(self):
        """The slots with a non-zero value as a uint64 (n, 2) array of (key, value) pairs in key order."""
        lib = gpu_lib()
        lib.salt_gpu_index_indel_fetch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        n = ctypes.c_uint64()
        _gpu_check(lib.salt_gpu_index_indel_fetch(self._ix, 0, None, ctypes.byref(n)))
        out = np.zeros((n.value, 2), dtype=np.uint64)
        if n.value:
            m = ctypes.c_uint64()
            _gpu_check(lib.salt_gpu_index_indel_fetch(self._ix, n.value, out.ctypes.data, ctypes.byref(m)))
            if m.value != n.value:
                raise SaltError("indel_fetch: the table changed between two calls")
        return out

    def indel_add(self, entries):
        """Inserts (key, value) pairs with the kernels' insert routine: how the tables of several GPUs are summed."""
        lib = gpu_lib()
        lib.salt_gpu_index_indel_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        entries = np.ascontiguousarray(entries, dtype=np.uint64).reshape(-1, 2)
        _gpu_check(lib.salt_gpu_index_indel_add(self._ix, entries.ctypes.data, entries.shape[0]))

    def indel_fetch_diff(self, first, n):
        """Words [first, first + n) of the tally's own difference array (uint32, ref_len + 1 words)."""
        lib = gpu_lib()
        lib.salt_gpu_index_indel_fetch_diff.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        out = np.zeros(max(int(n), 0), dtype=np.uint32)
        _gpu_check(lib.salt_gpu_index_indel_fetch_diff(self._ix, int(first), int(n), out.ctypes.data))
        return out

    def indel_add_diff(self, first, words):
        lib = gpu_lib()
        lib.salt_gpu_index_indel_add_diff.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
        words = np.ascontiguousarray(words, dtype=np.uint32)
        if words.ndim != 1:
            raise SaltError("indel_add_diff: words of shape (n,)")
        _gpu_check(lib.salt_gpu_index_indel_add_diff(self._ix, int(first), words.shape[0], words.ctypes.data))

    def indel_uncount(self):
        """Takes back what this aligner's last align call added to the indel table, its counters and its difference array."""
        lib = gpu_lib()
        lib.salt_gpu_ws_indel_uncount.argtypes = [ctypes.c_void_p]
        _gpu_check(lib.salt_gpu_ws_indel_uncount(self._ws))

    def indel_text(self, min_alt=3, min_pct=20, tile_positions=0, bgzf=False, pieces=False):
        """The VCF records of the table and the difference array as they stand, sorted, called and printed on the device (no header); with
        bgzf whole BGZF blocks (no end-of-file block).  pieces=True: the list of pieces as they left the device."""
        lib = gpu_lib()
        lib.salt_gpu_index_indel_text_begin.argtypes = [ctypes.c_void_p, ctypes.POINTER(_IndelTextOpt)]
        lib.salt_gpu_index_indel_text_next.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)]
        opt = _IndelTextOpt(int(min_alt), int(min_pct), int(tile_positions), 1 if bgzf else 0)
        _gpu_check(lib.salt_gpu_index_indel_text_begin(self._ix, ctypes.byref(opt)))
        out = []
        while True:
            p, n = ctypes.c_void_p(), ctypes.c_uint64()
            _gpu_check(lib.salt_gpu_index_indel_text_next(self._ix, ctypes.byref(p), ctypes.byref(n)))
            if n.value == 0:
                break
            out.append(ctypes.string_at(p.value, n.value))
        return out if pieces else b"".join(out)

    def set_quals(self, quals, on_device=False):
        """Quality bytes (Phred + 33, FASTQ order) parallel to the bases of the NEXT alnse_core1 / alnpe_core1 (a uint8 array or bytes) or,
        with on_device, of the next align_resident / align_pe_resident (a device pointer).  That call consumes them; None: none."""
        lib = gpu_lib()
        lib.salt_gpu_ws_set_quals.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        self._quals = None
        if quals is None or on_device:
            _gpu_check(lib.salt_gpu_ws_set_quals(self._ws, quals, 1 if on_device else 0))
        else:
            _gpu_check(lib.salt_gpu_ws_set_quals(self._ws, None, 0))
            self._quals = np.ascontiguousarray(np.frombuffer(quals, dtype=np.uint8) if isinstance(quals, (bytes, bytearray)) else quals, dtype=np.uint8)

    def _quals_for(self, lo, hi):
        """hands the pending host qualities of bases [lo, hi) to the batch that is about to be aligned"""
        q = getattr(self, "_quals", None)
        if q is None:
            return
        if len(q) < hi:
            raise SaltError("set_quals: %d quality bytes for %d bases" % (len(q), hi))
        self._qslice = np.ascontiguousarray(q[lo:hi])
        _gpu_check(gpu_lib().salt_gpu_ws_set_quals(self._ws, self._qslice.ctypes.data, 0))

    def counters(self):
        out = (ctypes.c_uint64 * len(CTR_NAMES))()
        _gpu_check(gpu_lib().salt_gpu_ws_counters(self._ws, out))
        return dict(zip(CTR_NAMES, [int(x) for x in out]))

    def fork(self, max_reads=None, max_bases=None):
        """Another workspace on the SAME device index (one per host thread / stream, as `salt` runs several per GPU).
        Close the forks before the aligner they came from."""
        other = GpuAligner.__new__(GpuAligner)
        other._ix, other._owns_ix = self._ix, False
        other._ix_shared = self._ix_state()
        other._ws = ctypes.c_void_p()
        other.max_reads = max_reads or self.max_reads
        other.max_bases = max_bases or self.max_bases
        other.device = self.device
        other._pac_set = getattr(self, "_pac_set", False)      # the 2-bit genome belongs to the device index, not to the workspace
        _gpu_check(gpu_lib().salt_gpu_ws_create(self._ix, other.max_reads, other.max_bases, ctypes.byref(other._ws)))
        return other

    def close(self):
        lib = gpu_lib()
        if self._ws:
            lib.salt_gpu_ws_destroy(self._ws)
            self._ws = None
        if self._ix and getattr(self, "_owns_ix", True):
            lib.salt_gpu_index_detach(self._ix)
        self._ix = None


class _PolishOpt(ctypes.Structure):
    _fields_ = [("paired", ctypes.c_int32), ("use_sw", ctypes.c_int32)]


POLISH_STATS = ("records", "hits_parsed", "unique_hits", "clipped_windows", "cigar_items", "proper_pairs", "output_bytes", "reserved")


class Polisher:
    """`polish` for a caller that holds SAM text: record lines in, polished record lines out, one device call per block
    (salt_gpu_polish_text).  Takes the 2-bit genome and the contig table from the Index."""

    def __init__(self, index, device=0):
        lib = gpu_lib()
        lib.salt_gpu_polish_open.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
        lib.salt_gpu_polish_close.argtypes = [ctypes.c_void_p]
        lib.salt_gpu_polish_set_contigs.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
        lib.salt_gpu_polish_text.argtypes = [ctypes.c_void_p, ctypes.POINTER(_PolishOpt), ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p),
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)]
        lib.salt_gpu_polish_text_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        self._h = ctypes.c_void_p()
        self.device = device
        self.stopped, self.n_records = False, 0
        pac, l_pac = index.pac()
        _gpu_check(lib.salt_gpu_polish_open(device, pac, l_pac, ctypes.byref(self._h)))
        cs = index.contigs()
        offs = (ctypes.c_int64 * len(cs))(*[c[0] for c in cs])
        names = (ctypes.c_char_p * len(cs))(*[c[2] for c in cs])
        try:
            _gpu_check(lib.salt_gpu_polish_set_contigs(self._h, len(cs), offs, names))
        except SaltError:
            self.close()
            raise

    def polish_text(self, sam, paired=False, sw=False):
        """One block of whole SAM record lines (no header) -> the polished records, in input order.  `stopped` says whether an empty
        line ended the block early; `n_records` how many records were polished."""
        sam = bytes(sam)
        self.stopped, self.n_records = False, 0                   # of this call, also when it raises
        opt = _PolishOpt(1 if paired else 0, 1 if sw else 0)
        out, n, recs, stopped = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_int()
        _gpu_check(gpu_lib().salt_gpu_polish_text(self._h, ctypes.byref(opt), sam, len(sam), ctypes.byref(out), ctypes.byref(n), ctypes.byref(recs), ctypes.byref(stopped)))
        self.stopped, self.n_records = bool(stopped.value), recs.value
        return ctypes.string_at(out.value, n.value) if n.value else b""

    def stats(self):
        """The eight counts of the last polish_text call, in the order of POLISH_STATS."""
        out = (ctypes.c_uint64 * 8)()
        _gpu_check(gpu_lib().salt_gpu_polish_text_stats(self._h, out))
        return [int(x) for x in out]

    def close(self):
        if getattr(self, "_h", None):
            gpu_lib().salt_gpu_polish_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


_NT4 = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _NT4[ord(_c)] = _i
    _NT4[ord(_c.lower())] = _i


def read_fastq(path):
    """4-line FASTQ (optionally .gz) -> names, seqs (codes), offs, quals.  A name ends at the first white-space
    byte of C's isspace() behind the '@', as kseq and the device parser end it (so it is empty when the header
    begins with one), and loses a trailing /digit when longer than 2 like trim_readno (query.c:139-143)."""
    import gzip
    op = gzip.open if path.endswith(".gz") else open
    names, quals, chunks, offs = [], [], [], [0]
    with op(path, "rb") as f:
        while True:
            h = f.readline()
            if not h:
                break
            if not h.startswith(b"@"):
                continue
            s = f.readline().rstrip(b"\r\n")
            f.readline()
            q = f.readline().rstrip(b"\r\n")
            nm = h[1:]
            for k, c in enumerate(nm):                    # up to the first white space of isspace(): the name may be empty
                if c in b" \t\n\v\f\r":
                    nm = nm[:k]
                    break
            if len(nm) > 2 and nm[-2:-1] == b"/" and nm[-1:].isdigit():
                nm = nm[:-2]
            names.append(nm)
            quals.append(q)
            chunks.append(_NT4[np.frombuffer(s, dtype=np.uint8)])
            offs.append(offs[-1] + len(s))
    seqs = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
    return names, seqs, np.array(offs, dtype=np.uint32), quals


def interleave_pairs(r1, r2):
    """Two read_fastq() results -> one with mates interleaved as query_read_multiPairedSeqs (query.c:252-268)."""
    n1, s1, o1, q1 = r1
    n2, s2, o2, q2 = r2
    if len(n1) != len(n2):
        raise SaltError("mate files differ in length")
    names, quals, chunks, offs = [], [], [], [0]
    for i in range(len(n1)):
        for nm, sq, of, ql in ((n1, s1, o1, q1), (n2, s2, o2, q2)):
            names.append(nm[i]); quals.append(ql[i]); chunks.append(sq[of[i]:of[i + 1]])
            offs.append(offs[-1] + int(of[i + 1] - of[i]))
    seqs = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.uint8)
    return names, seqs, np.array(offs, dtype=np.uint32), quals


def sam_text_pe(index, opt, names, seqs, offs, quals, results, header=True):
    """The SAM stream `salt -p` prints (without @PG)."""
    out = [index.sam_header(opt)] if header else []
    for i in range(0, len(names), 2):
        out.append(index.sampe(opt, names[i:i + 2], [seqs[offs[i]:offs[i + 1]], seqs[offs[i + 1]:offs[i + 2]]],
                               quals[i:i + 2], results[i:i + 2]))
    return b"".join(out)


def sam_text(index, opt, names, seqs, offs, quals, results, header=True):
    """The SAM stream `salt` prints (without @PG): header, then one line per read in input order."""
    out = []
    if header:
        out.append(index.sam_header(opt))
    for i in range(len(names)):
        rec = index.samse(opt, names[i], seqs[offs[i]:offs[i + 1]], quals[i], results[i:i + 1])
        out.append(rec + b"\n")
    return b"".join(out)
