"""The plain model of the device index image (tests/index_image_model.py) against facts it did not compute itself: the index files'
own suffix-array samples, interleaved counts and explicit Occ values, the R text, the allele masks.  tests/test_gpu_index_image.py
compares the device image with this model element by element; here the model is pinned, on the lambda index, the four
tests/golden/index_cases and the generated edge cases, without a GPU."""
import ctypes
import os

import numpy as np
import pytest

import index_image_model as M
from conftest import GOLDEN, LAMBDA

COMMITTED = {"lambda": os.path.join(LAMBDA, "idx")}
COMMITTED.update({c: os.path.join(GOLDEN, "index_cases", c, "idx") for c in ("all_snp_contigs", "dense", "gap_short", "two_contigs")})
_models = {}


def model(prefix):
    if prefix not in _models:
        _models[prefix] = M.Model(prefix)
    return _models[prefix]


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    return M.edge_cases(tmp_path_factory.mktemp("edge"))


@pytest.fixture(scope="module")
def prefixes(edge, tmp_path_factory):
    """lambda as committed (written by the reference's indexer); the four index cases as this project's builder writes them from the
    case's genome.fa and snps.txt, each asserted to differ from the committed, reference-written files the model reads in nothing
    but the ONE word of .R.backward.sa that the reference reads past its array (tests/test_index_builder.py holds the same for
    every file); the edge cases."""
    import salt_amd
    lib = salt_amd.host_lib()
    lib.salt_idx_build.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
    out = {"lambda": COMMITTED["lambda"]}
    for name, committed in COMMITTED.items():
        if name == "lambda":
            continue
        d = os.path.dirname(committed)
        prefix = str(tmp_path_factory.mktemp(name) / "idx")
        assert lib.salt_idx_build(os.path.join(d, "genome.fa").encode(), os.path.join(d, "snps.txt").encode(), prefix.encode(), 19) == 0
        for sfx in (".R.seedLen", ".C.pac", ".C.ann", ".C.bwt", ".C.sa", ".R.backward.bwt", ".R.backward.occ"):
            assert open(prefix + sfx, "rb").read() == open(committed + sfx, "rb").read(), (name, sfx)
        got, want = np.fromfile(prefix + ".R.backward.sa", dtype="<u4"), np.fromfile(committed + ".R.backward.sa", dtype="<u4")
        assert len(got) == len(want) and int((got != want).sum()) <= 1, name
        a, b = M.Model(prefix), M.Model(committed)
        assert a.ref_len == b.ref_len and np.array_equal(a.mask, b.mask), name
        out[name] = prefix
    out.update(edge)
    return out


ALL = sorted(COMMITTED) + sorted(M.EDGE_CASES)


@pytest.mark.parametrize("name", ALL)
def test_c_suffix_array_and_bwt_agree_with_the_files(prefixes, name):
    """The sorted-suffix SA equals the file's samples SA[8], SA[16], ...; the row with SA == 0 is the file's primary; the BWT T[SA - 1]
    gives the file's L2 and, 128 symbols at a time, the file's interleaved counts and packed symbols."""
    m = model(prefixes[name])
    n = m.c_seq_len
    assert m.c_sa_intv == 8 and len(m.c_sa_file) == n // 8
    assert np.array_equal(m.SA[8::8], m.c_sa_file)
    assert m.primary == m.c_primary
    assert [int((m.B < c).sum()) for c in range(1, 5)] == list(m.c_L2[1:])
    body = np.fromfile(prefixes[name] + ".C.bwt", dtype="<u4")[5:]
    nb = (n + 127) // 128 + 1                                            # one block of counts past the last symbol block
    assert len(body) == (n + 15) // 16 + nb * 4
    sym = np.zeros((n + 15) // 16 * 16, dtype=np.uint64)
    sym[:n] = m.B
    words = (sym << (30 - 2 * (np.arange(len(sym)) & 15)).astype(np.uint64)).reshape(-1, 16).sum(axis=1).astype("<u4")
    at = 0
    for b in range(nb):                                                  # 4 counts, then the (up to 8) words of the block's symbols
        assert list(body[at:at + 4]) == [int(m.c_cum[c, min(128 * b, n)]) for c in range(4)], (name, "counts in front of symbol", 128 * b)
        nw = min(8, max(0, len(words) - 8 * b))
        assert np.array_equal(body[at + 4:at + 4 + nw], words[8 * b:8 * b + nw]), (name, "symbols of file block", b)
        at += 4 + nw
    assert at == len(body)


@pytest.mark.parametrize("name", ALL)
def test_r_explicit_occ_values_equal_the_cumulative_counts(prefixes, name):
    """What k_pack_r_occ reads is what the model computes: the file's explicit Occ value of every symbol at every 256 symbols
    (16-bit minor + 32-bit major) and its major values at every 65 536 equal the plain cumulative counts of the stored BWT."""
    m = model(prefixes[name])
    e = np.arange(m.r_text_len // 256 + 1)
    assert len(m.r_minor) >= (len(e) + 1) // 2 * 5 and len(m.r_major) >= (m.r_text_len // 65536 + 1) * 5
    for c in range(5):
        mv = m.r_minor[e // 2 * 5 + c]
        mv = np.where(e & 1, mv & 0xFFFF, mv >> 16)
        major = m.r_major[e // 256 * 5 + c]
        assert np.array_equal(major, m.r_occ_cum[c, 65536 * (e // 256)]), (name, c)
        assert np.array_equal(major.astype(np.int64) + mv, m.r_occ_cum[c, 256 * e]), (name, c)
    assert list(m.r_cum[1:]) == [int((m.RB <= c).sum()) for c in range(5)]
    assert len(m.r_sa) == m.r_text_len - int(m.r_cum[4]) + 1


@pytest.mark.parametrize("name", ALL)
def test_r_text_and_r_pos_are_consistent_with_the_allele_masks(prefixes, name):
    """The R text, recovered by inverting the stored BWT with the model's own Occ, is '#' segment '#' segment ... '#' (and equals
    idx.R.pac where that file exists), and r_pos is consistent with it and with the allele masks:

    (a) every row: within a segment r_pos grows by one per base -- r_pos[row] - d is one value v for the '#' in front of a segment
        (d = -1) and for each of its bases (d = 0, 1, ...) -- and the '$' row stands one behind the last '#'.
    (b) every segment but the first: the table entry of the segment BEFORE it places it on the genome.  Rbwt_gen_sa (rbwt.c:424-475)
        gives the '#' in front of segment s the window end of the record of segment s + 1, less the length of s and one: so segment
        s + 1 ends at v(s) + len(s) + 1 -- the SNP's position + k - 1 -- or at the last base of the SNP's contig (.C.ann) where that
        comes first, and every base of it is allowed by the mixRef mask there (a reference N has an empty mask and a random draw of its
        own in the R text: nothing to compare).  (For segments of one record this makes
        r_pos the suffix's position less two -- which the aligner, like the reference, meets as the 2D100M alignments of SURVEY.md
        Appendix B -- and for the last segment of a record it is the next record's end that counts.  A statement about "the mask at
        r_pos + i" holds for no row; this one holds for every entry the reference defines.)

    (c) the last segment, which no table entry behind it places: the reference reads the window end for it one past its array
        (sharp2Ri_array[n], rbwt.c:377,461); this project's builder puts 0 there, so in every index it wrote -- the
        index cases as built here and the edge cases -- the '#' in front of the last segment holds 0 - (len + 1), and with (a) that
        fixes r_pos of all its rows.

    The class none of this places on the genome: the rows of the last segment in an index the REFERENCE wrote, which here is lambda
    alone (that word is whatever lay behind the reference's array; (a) still holds for those rows).  The test prints the share of
    that class and asserts it below 1 % of the rows on every index: 0.004 % on lambda, none elsewhere."""
    m = model(prefixes[name])
    text, row_of = m.r_text()
    n = m.r_text_len
    assert text[0] == 4 and text[-1] == 4 and (text <= 4).all()
    assert name != "lambda" or os.path.exists(prefixes[name] + ".R.pac"), "the lambda fixture lost idx.R.pac"
    if os.path.exists(prefixes[name] + ".R.pac"):
        pac = np.fromfile(prefixes[name] + ".R.pac", dtype=np.uint8)
        i = np.arange(n)
        assert np.array_equal((pac[i >> 1] >> ((~i & 1) << 2)) & 15, text)
    rp = m.r_pos().astype(np.int64)[row_of]                                # by text position; [n]: the '$' row
    sharp = np.nonzero(text == 4)[0]
    seg = np.cumsum(text == 4) - 1                                         # the '#' in front, per text position
    d = np.arange(n) - sharp[seg] - 1
    v = (rp[sharp] + 1) & 0xFFFFFFFF
    assert np.array_equal(rp[:n], (v[seg] + d) & 0xFFFFFFFF), name        # (a)
    assert rp[n] == (rp[sharp[-1]] + 1) & 0xFFFFFFFF
    length = np.diff(sharp) - 1                                            # length[s]: the segment behind '#' s
    n_seg = len(length)
    lines = open(prefixes[name] + ".C.ann").read().split("\n")
    contigs = [tuple(int(x) for x in ln.split()[:2]) for ln in lines[2::2] if ln.strip()]      # (offset, length) of every contig
    for s in range(n_seg - 1):                                             # (b): '#' s places segment s + 1
        end = (int(v[s]) + int(length[s]) + 1) & 0xFFFFFFFF
        snp = end - (m.l_seed - 1)
        last = [o + ln - 1 for o, ln in contigs if o <= snp < o + ln]
        assert len(last) == 1, (name, "segment", s + 1, "no contig holds position", snp)
        end = min(end, last[0])
        start = end - int(length[s + 1]) + 1
        bases = text[sharp[s + 1] + 1:sharp[s + 2]].astype(np.int64)
        assert 0 <= start and end < m.ref_len, (name, "segment", s + 1, start, end)
        mk = m.mask[start:end + 1]
        ok = ((mk >> bases) & 1).astype(bool) | (mk == 0)      # a reference N: an empty mask, and a random draw of its own in the R text
        assert ok.all(), (name, "segment", s + 1, "at", start)
    if name == "lambda":
        share = (int(length[-1]) + 1) / (n + 1)
    else:                                                                  # (c)
        assert int(v[n_seg - 1]) == (-(int(length[-1]) + 1)) & 0xFFFFFFFF, (name, int(v[n_seg - 1]), int(length[-1]))
        share = 0.0
    print("%s: %d R rows, %d segments; rows whose position nothing states: %.4f %%" % (name, n + 1, n_seg, 100 * share))
    assert share < 0.01


@pytest.mark.parametrize("name", ALL)
def test_wlkt_c_interval_at_w12_counts_the_padded_suffixes(prefixes, name):
    """For all 4^12 W-mers: the C interval of the model's W = 12 table has l - k + 1 = the number of suffixes (the empty one included)
    that start with the W-mer once padded with A to 12 bases -- counted over text positions, not along the suffix array -- and the
    12-mer table starts each interval."""
    m = model(prefixes[name])
    x, rows = m.wlkt(12)
    width = np.zeros(1 << 24, dtype=np.int64)
    width[x] = rows[:, 1].astype(np.int64) - rows[:, 0].astype(np.int64) + 1
    n = m.c_seq_len
    t = np.concatenate([m.T, np.zeros(12, np.uint8)]).astype(np.int64)
    count = np.zeros(1 << 24, dtype=np.int64)
    keys = sum(t[j:j + n + 1] << (2 * (11 - j)) for j in range(12))
    np.add.at(count, keys, 1)
    assert np.array_equal(width, count)
    lkt = m.lkt().astype(np.int64)
    assert lkt[0] == 0 and lkt[-1] == n + 1 and np.array_equal(np.diff(lkt), count)
    c_rows = rows[width[x] > 0]
    assert np.array_equal(c_rows[:, 0], lkt[x[width[x] > 0]])


def test_edge_cases_have_what_they_are_listed_for(edge):
    """Each generated case still has the properties its table entry names (and the repeats and special sites every case has), and
    together the cases have all of EDGE_WANTED."""
    found_all = set()
    for name, (seed, length, listed) in M.EDGE_CASES.items():
        m = model(edge[name])
        found = M.edge_properties(m)
        print("%s: c_seq_len %d, c_primary %d, r_text_len %d, r_inv_sa0 %d, k %d: %s" % (name, m.c_seq_len, m.c_primary, m.r_text_len, m.r_inv_sa0, m.l_seed, sorted(found)))
        assert m.c_seq_len == length and m.ref_len == length
        assert set(listed) | set(M.EDGE_COMMON) <= found, (name, sorted((set(listed) | set(M.EDGE_COMMON)) - found))
        found_all |= found
    assert set(M.EDGE_WANTED) <= found_all, sorted(set(M.EDGE_WANTED) - found_all)
