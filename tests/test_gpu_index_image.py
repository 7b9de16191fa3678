"""The device index image, word by word, against the plain model of tests/index_image_model.py -- and the rank primitives that read
it, asked directly.

Every alignment kernel reads the index through the image salt_gpu_index_attach builds (salt_device.h): COcc, ROcc, c_sa, r_pos, lkt, ref,
text, wlkt and c_ctx, with r_ctx beside it.  Here each of them is compared over its whole defined length, no tolerance, with arrays the
model computed from the index files alone (a sorted suffix array, BWT = T[SA - 1], Occ = a cumulative count; tests/
test_index_image_model.py pins the model on the CPU): on the lambda index (-k 19; the W-mer table and the context records again at
W = 13 and 14 and with an index built with -k 21, where side A of the records starts elsewhere), the four tests/golden/index_cases and
the generated edge cases whose lengths sit on the block and word boundaries.  W = 15 and 16 (32 and 128 GiB) are not attached: the
table's width is a run-time argument of the one kernel k_build_wlkt, no code is specific to them.

The W-mer table (512 MB at W = 12, 8.6 GB at 14) never comes to the host whole: the entries that are not ((1,0,1,0),(0,0,0,0)) are
found on the device, their index set must be the model's set of non-empty W-mers, and only they are brought over and compared.

salt_gpu_diag_occ asks c_occ, c_occ2, c_occ2_addr + c_occ2_eval and c_sym (r_occ, r_occ2, r_occ2_addr + r_occ2_eval, r_bwt2nt) the
same questions: every row, symbol and pair distance on the small indexes, random pairs and the rows around the '$' row, the 65 536
boundaries and both ends on lambda.  All must give the model's cumulative counts, and so agree with each other."""
import ctypes
import os

import numpy as np
import pytest

import index_image_model as M
from conftest import GOLDEN, LAMBDA

pytestmark = pytest.mark.gpu

NONE = M.NONE
SMALL = ["all_snp_contigs", "dense", "gap_short", "two_contigs"] + sorted(M.EDGE_CASES)
DELTAS = (0, 1, 2, 62, 63, 64, 65, 127, 128, 129)

# ImageHeader of salt_device.h
HEADER = np.dtype([("magic", "<u8"), ("bytes", "<u8"), ("c_primary", "<u4"), ("c_L2", "<u4", (5,)), ("c_seq_len", "<u4"), ("c_sa_intv", "<u4"),
                   ("lkt_len", "<u4"), ("lkt_n", "<u4"), ("r_text_len", "<u4"), ("r_inv_sa0", "<u4"), ("r_cum", "<u4", (6,)), ("ref_len", "<u4"),
                   ("r_lkt_len", "<u4"), ("off_c_occ", "<u8"), ("off_c_sa", "<u8"), ("off_lkt", "<u8"), ("off_r_occ", "<u8"), ("off_r_pos", "<u8"),
                   ("off_wlkt", "<u8"), ("off_ref", "<u8"), ("off_text", "<u8"), ("n_c_blocks", "<u8"), ("n_r_blocks", "<u8"), ("off_ctx", "<u8"),
                   ("ctx_k", "<u4"), ("pad0", "<u4"), ("reserved", "<u8", (5,))])
assert HEADER.itemsize == 232


class Attached:
    """One index on the device at W-mer width w: the host index, the aligner, the model, a copy of the image in a torch tensor."""

    def __init__(self, prefix, w, model=None):
        import salt_amd
        import torch
        self.model = model or M.Model(prefix)
        self.idx = salt_amd.Index.reload(prefix)
        old = os.environ.get("SALT_GPU_LKT_LEN")
        os.environ["SALT_GPU_LKT_LEN"] = str(w)
        try:
            self.aln = salt_amd.GpuAligner(self.idx, device=0, max_reads=16)
        finally:
            if old is None:
                del os.environ["SALT_GPU_LKT_LEN"]
            else:
                os.environ["SALT_GPU_LKT_LEN"] = old
        _, n = self.aln.image()
        self.image = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        self.aln.image_copy(self.image.data_ptr(), n)
        self.hdr = self.image[:HEADER.itemsize].cpu().numpy().view(HEADER)[0]
        self.w = w

    def words(self, off, n_words):
        """n_words 32-bit words of the image from byte `off`, as an int32 tensor on the device."""
        import torch
        return self.image[int(off):int(off) + 4 * int(n_words)].view(torch.int32)

    def close(self):
        import torch
        self.image = None
        self.aln.close()
        self.idx.destroy()
        torch.cuda.empty_cache()      # the image copies go back to the device: later tests size their tables by the memory that is free


def first_diff(name, got_dev, want):
    """got_dev: int32 tensor on the device; want: uint32 array.  Fails with the array's name, the first differing index, both values."""
    import torch
    want = np.ascontiguousarray(want, dtype="<u4").reshape(-1)
    assert got_dev.numel() == want.size, "%s: %d words on the device, %d in the model" % (name, got_dev.numel(), want.size)
    w = torch.from_numpy(want.view(np.int32)).to(got_dev.device)
    ne = got_dev != w
    if bool(ne.any()):
        i = int(ne.nonzero()[0, 0])
        pytest.fail("%s: first difference at word %d: device 0x%08x, model 0x%08x (%d words differ)"
                    % (name, i, int(got_dev[i]) & 0xFFFFFFFF, int(want[i]), int(ne.sum())))


def check_header(a):
    m, h = a.model, a.hdr
    assert h["bytes"] == a.image.numel()
    assert (h["c_primary"], h["c_seq_len"], h["c_sa_intv"], h["lkt_len"], h["lkt_n"]) == (m.c_primary, m.c_seq_len, 8, 12, (1 << 24) + 1)
    assert list(h["c_L2"]) == list(m.c_L2) and list(h["r_cum"]) == list(m.r_cum)
    assert (h["r_text_len"], h["r_inv_sa0"], h["ref_len"], h["r_lkt_len"], h["ctx_k"]) == (m.r_text_len, m.r_inv_sa0, m.ref_len, a.w, m.l_seed)
    assert (h["n_c_blocks"], h["n_r_blocks"]) == (m.c_seq_len // 64 + 1, m.r_text_len // 128 + 1)
    assert h["off_ctx"] != 0, "no context table on a device with room for it"


def check_wlkt(a):
    """The table's non-empty entries are the model's, in place and in full; every other entry is the empty pattern."""
    import torch
    m, h = a.model, a.hdr
    n = 1 << (2 * a.w)
    t = a.words(h["off_wlkt"], 8 * n).view(n, 8)
    empty = torch.tensor([1, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=t.device)
    where = (t != empty).any(dim=1).nonzero().squeeze(1)
    x, rows = m.wlkt(a.w)
    got_x = where.cpu().numpy()
    if not np.array_equal(got_x, x):
        only = np.setxor1d(got_x, x)
        pytest.fail("wlkt (W = %d): %d non-empty entries on the device, %d in the model; first W-mer in one set only: %d (%s)"
                    % (a.w, len(got_x), len(x), only[0], "device" if only[0] in got_x else "model"))
    got = t[where].cpu().numpy().view("<u4")
    if not np.array_equal(got, rows):
        i = int(np.nonzero((got != rows).any(axis=1))[0][0])
        pytest.fail("wlkt (W = %d): entry of W-mer %d: device %s, model %s" % (a.w, x[i], got[i].tolist(), rows[i].tolist()))


def check_c_ctx(a):
    m, h = a.model, a.hdr
    first_diff("c_ctx", a.words(h["off_ctx"], 4 * (m.c_seq_len + 1)), m.c_ctx())


def check_r_ctx(a):
    """r_ctx lies outside the image: the model's records go up into a tensor and are compared 4 096 rows at a time on the device."""
    import salt_amd
    import torch
    m = a.model
    p, n = a.aln.r_ctx()
    assert p and n == 16 * (m.r_text_len + 1), "r_ctx absent or of the wrong size on a small index: %r, %d bytes" % (p, n)
    want = m.r_ctx()
    dev = torch.from_numpy(want.view(np.int32)).to("cuda:0")
    lib = salt_amd.gpu_lib()
    lib.salt_gpu_buffer_equal.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int)]
    for lo in range(0, len(want), 4096):
        hi = min(lo + 4096, len(want))
        eq = ctypes.c_int(-1)
        assert lib.salt_gpu_buffer_equal(0, p + 16 * lo, dev.data_ptr() + 16 * lo, 16 * (hi - lo), ctypes.byref(eq)) == 0
        if eq.value != 1:
            pytest.fail("r_ctx: rows %d..%d differ from the model's, which are (first 8)\n%s" % (lo, hi - 1, want[lo:lo + 8]))


def check_all(a):
    m, h = a.model, a.hdr
    check_header(a)
    first_diff("COcc", a.words(h["off_c_occ"], 8 * int(h["n_c_blocks"])), m.c_occ_words())
    first_diff("ROcc", a.words(h["off_r_occ"], 16 * int(h["n_r_blocks"])), m.r_occ_words())
    first_diff("c_sa", a.words(h["off_c_sa"], m.c_seq_len + 1), m.c_sa)
    first_diff("r_pos", a.words(h["off_r_pos"], m.r_text_len + 1), m.r_pos())
    first_diff("lkt", a.words(h["off_lkt"], (1 << 24) + 1), m.lkt())
    first_diff("ref", a.words(h["off_ref"], (m.ref_len + 7) // 8 + 4), m.ref_image_words())
    first_diff("text", a.words(h["off_text"], m.c_seq_len // 16 + 4), m.text_words())
    check_c_ctx(a)
    check_wlkt(a)
    check_r_ctx(a)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """name -> Attached (W = 12) of the four index cases and the edge cases, attached on first use, detached with the module."""
    prefixes = {c: os.path.join(GOLDEN, "index_cases", c, "idx") for c in SMALL[:4]}
    prefixes.update(M.edge_cases(tmp_path_factory.mktemp("edge")))
    made = {}

    def get(name):
        if name not in made:
            made[name] = Attached(prefixes[name], 12)
        return made[name]
    yield get
    for a in made.values():
        a.close()


@pytest.fixture(scope="module")
def lam():
    a = Attached(os.path.join(LAMBDA, "idx"), 12)
    yield a
    a.close()


@pytest.mark.parametrize("name", SMALL)
def test_gpu_image_equals_the_model_on_the_small_indexes(small, name):
    """An attach that fails here is a finding: these indexes are valid, the error bits of k_pack_c_occ / k_pack_r_occ are for arrays
    that are truly short."""
    check_all(small(name))


def test_gpu_image_equals_the_model_on_lambda(lam):
    check_all(lam)


@pytest.mark.parametrize("w", [13, 14])
def test_gpu_wlkt_and_ctx_equal_the_model_on_lambda_at_wider_tables(lam, w):
    a = Attached(os.path.join(LAMBDA, "idx"), w, model=lam.model)
    try:
        check_header(a)
        check_wlkt(a)
        check_c_ctx(a)
    finally:
        a.close()


def test_gpu_image_equals_the_model_on_lambda_built_with_k21(tmp_path):
    """Seed length 21: another R text, and side A of every context record starts at 42."""
    import salt_amd
    prefix = str(tmp_path / "k21")
    salt_amd.idx_build(os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix, 21, flags=salt_amd.IDX_NO_LP)
    a = Attached(prefix, 12)
    try:
        assert a.model.l_seed == 21
        check_all(a)
    finally:
        a.close()


# ---- the rank primitives ----
def expect_c(m, q):
    """The 10 defined words of salt_gpu_diag_occ's answer to C queries q (n, 3), from the model's cumulative counts."""
    k, l, c = (q[:, i].astype(np.int64) for i in range(3))
    ok, ol = m.c_occ(k, c), m.c_occ(l, c)
    ks, ls = (k == m.c_seq_len) | (k == NONE), (l == m.c_seq_len) | (l == NONE)
    bk, bl = (k - (k >= m.c_primary)) >> 6, (l - (l >= m.c_primary)) >> 6
    blocks = (~ks).astype(np.int64) + (~ls & (ks | (bl != bk)))          # distinct blocks among the ends that have one
    return np.stack([ok, ol, ok, ol, ok, ol, blocks, blocks, blocks, m.c_row_sym(k)], axis=1)


def expect_r(m, q):
    a, b, c = (q[:, i].astype(np.int64) for i in range(3))
    oa, ob = m.r_occ(a, c), m.r_occ(b, c)
    blocks = 1 + (((a - (a > m.r_inv_sa0)) >> 7) != ((b - (b > m.r_inv_sa0)) >> 7))
    sym = np.where(a > m.r_text_len, 5, m.r_row_sym(np.minimum(a, m.r_text_len)))
    return np.stack([oa, ob, oa, ob, oa, ob, blocks, blocks, blocks, sym], axis=1)


WORDS = ("occ(x)", "occ(y)", "occ2.x", "occ2.y", "addr+eval.x", "addr+eval.y", "occ2 blocks", "eval blocks", "addr blocks", "symbol of row x")


def ask(a, mode, q):
    m = a.model
    q = np.ascontiguousarray(q, dtype=np.uint32)
    got = a.aln.diag_occ(mode, q)
    want = (expect_c if mode == "C" else expect_r)(m, q)
    assert not got[:, 10:].any()
    bad = np.nonzero(got[:, :10].astype(np.int64) != want)
    if len(bad[0]):
        i, j = int(bad[0][0]), int(bad[1][0])
        pytest.fail("%s query %s (c_primary %d, c_seq_len %d, r_inv_sa0 %d, r_text_len %d): %s = %d, model %d; whole answer %s, model %s (%d queries differ)"
                    % (mode, q[i].tolist(), m.c_primary, m.c_seq_len, m.r_inv_sa0, m.r_text_len, WORDS[j], got[i, j], want[i, j],
                       got[i, :10].tolist(), want[i].tolist(), len(set(bad[0].tolist()))))


def pairs(xs, hi, specials):
    """(x, y) for every x of xs: y = x + d for d in DELTAS where that stays inside [0, hi], y = hi, and y = each special."""
    xs = np.asarray(xs, dtype=np.int64)
    out = [np.stack([xs, xs + d], axis=1)[xs + d <= hi] for d in DELTAS]
    out += [np.stack([xs, np.full(len(xs), y, dtype=np.int64)], axis=1) for y in [hi] + list(specials)]
    return np.concatenate(out)


def with_symbols(xy, n_sym):
    return np.concatenate([np.concatenate([xy, np.full((len(xy), 1), c, dtype=np.int64)], axis=1) for c in range(n_sym)])


@pytest.mark.parametrize("name", SMALL)
def test_gpu_rank_primitives_answer_every_query_as_the_model_on_the_small_indexes(small, name):
    """Exhaustive: every row, every symbol, every pair distance of DELTAS, the whole-text end from every row; for the C index also the
    empty end 0xFFFFFFFF at either side."""
    a = small(name)
    m = a.model
    rows = np.arange(m.c_seq_len + 1)
    xy = np.concatenate([pairs(rows, m.c_seq_len, [NONE]), np.stack([np.full(len(rows), NONE), rows], axis=1), [[NONE, NONE]]])
    ask(a, "C", with_symbols(xy, 4))
    xy = pairs(np.arange(m.r_text_len + 2), m.r_text_len + 1, [])
    for c in range(5):
        ask(a, "R", np.concatenate([xy, np.full((len(xy), 1), c, dtype=np.int64)], axis=1))


def test_gpu_rank_primitives_answer_as_the_model_on_lambda(lam):
    """200 000 random pairs, and every row within 130 of the '$' row, of a multiple of 65 536 and of either end, with every pair
    distance and symbol."""
    m = lam.model
    rng = np.random.default_rng(12)
    for mode, hi, special_row, n_sym, specials in (("C", m.c_seq_len, m.c_primary, 4, [NONE]), ("R", m.r_text_len + 1, m.r_inv_sa0, 5, [])):
        x = rng.integers(0, hi + 1, 200000)
        y = np.where(rng.random(200000) < 0.5, rng.integers(0, hi + 1, 200000), np.minimum(x + rng.integers(0, 300, 200000), hi))
        if mode == "C":
            x[:2000], y[2000:4000] = NONE, NONE
        ask(lam, mode, np.stack([x, y, rng.integers(0, n_sym, 200000)], axis=1))
        near = np.concatenate([np.arange(c - 130, c + 131) for c in [special_row, 0, hi] + list(range(65536, hi, 65536))])
        near = np.unique(near[(near >= 0) & (near <= hi)])
        ask(lam, mode, with_symbols(pairs(near, hi, specials), n_sym))


def test_gpu_rank_entry_rejects_queries_outside_its_range(lam):
    import salt_amd
    m = lam.model
    for mode, q in (("C", [m.c_seq_len + 1, 0, 0]), ("C", [0, 0xFFFFFFFE, 0]), ("C", [0, 0, 4]),
                    ("R", [m.r_text_len + 2, 0, 0]), ("R", [0, NONE, 0]), ("R", [0, 0, 5])):
        with pytest.raises(salt_amd.SaltError, match="query 1"):
            lam.aln.diag_occ(mode, [[0, 0, 0], q])
