"""The pair rule on the device (k_fq_trim_pair, salt_trim.hip) against the host twin (salt_amd.trim_pair_span /
trim_fastq_pair, which test_trim_pair_host.py holds against the plain Python statement of the rule): the kernel alone through
GpuAligner.trim_pair_spans on the edge-case set, 20 000 ragged pairs and blocks of one and of three pairs, both counter arrays; then the
contract -- a paired-end text call with set_trim_pair returns the block the same call returns without it on the twin's trimmed files, in
every output mode, for the tallies too -- and with the rule off a call is what it is on a workspace that never set it."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from bgzf_check import strip_pg
import trim_check as tc
import trim_pair_check as pc
from conftest import LAMBDA, ROOT

pytestmark = pytest.mark.gpu

PE_ARGS = ["-d", "-p", "-c", "-a", "350", "-b", "650"]
TRIM = dict(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2, qual=20)


@pytest.fixture(scope="module")
def lambda_index():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield ix
    ix.destroy()


def _aligner(ix):
    import salt_amd
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=40960)
    aln.set_contigs(ix)
    aln.set_pac(ix)
    return aln


@pytest.fixture(scope="module")
def aligner(lambda_index):
    aln = _aligner(lambda_index)
    yield aln
    aln.close()


def _set(aln, o, po):
    aln.set_trim(**o)
    aln.set_trim_pair(po["min_overlap"], po["error_pct"]) if po else aln.set_trim_pair(None)


def _off(aln):
    aln.set_trim()
    aln.set_trim_pair(None)


def twin_spans(o, po, pairs, counts=None, pair_counts=None):
    import salt_amd
    kw = dict(adapter=o["adapter"], adapter2=o["adapter2"], qual_min=o["qual"], front=o["front"], tail=o["tail"], adapter_min_overlap=o["min_overlap"],
              adapter_error_pct=o["error_pct"])
    kw.update(dict(pair=True, min_overlap=po["min_overlap"], error_pct=po["error_pct"]) if po else dict(pair=False))
    return np.array([salt_amd.trim_pair_span(r1[0], r1[1], r2[0], r2[1], counts=counts, pair_counts=pair_counts, **kw) for r1, r2 in pairs], dtype=np.uint32).reshape(-1, 4)


def same_spans(got, want, pairs, what):
    bad = np.argwhere((got != want).any(axis=1)).reshape(-1)
    assert got.shape == want.shape and not len(bad), (what, len(bad), [(int(i), pairs[i][0][0], pairs[i][1][0], got[i].tolist(), want[i].tolist()) for i in bad[:3]])


def test_spans_and_both_counter_arrays_equal_the_twin_on_the_edge_case_set(aligner):
    counts, pairs_c = np.zeros((2, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    aligner.trim_counts(reset=True); aligner.trim_pair_counts(reset=True)
    n = 0
    try:
        for cr, (o, po, pairs) in enumerate(pc.group(pc.edge_cases())):
            _set(aligner, o, po)
            fq1, fq2 = pc.fastq_of_pairs(pairs, cr=cr % 2 == 1)            # every other group with CR LF line ends
            same_spans(aligner.trim_pair_spans(fq1, fq2), twin_spans(o, po, pairs, counts, pairs_c), pairs, (o, po))
            n += len(pairs)
    finally:
        _off(aligner)
    assert n > 800 and pairs_c[7] == 8 and pairs_c[2] > 100
    assert (aligner.trim_counts() == counts).all(), (aligner.trim_counts(), counts)
    assert (aligner.trim_pair_counts() == pairs_c).all(), (aligner.trim_pair_counts(), pairs_c)


def test_spans_and_counters_equal_the_twin_on_20000_ragged_pairs(aligner):
    """Lengths 1 to 300 in one block, more pairs than the grid has waves: waves take several pairs and run out of them at different times."""
    o, po, pairs = pc.random_pairs(20000, seed=9)
    fq1, fq2 = pc.fastq_of_pairs(pairs)
    counts, pairs_c = np.zeros((2, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    want = twin_spans(o, po, pairs, counts, pairs_c)
    _set(aligner, o, po)
    try:
        aligner.trim_counts(reset=True); aligner.trim_pair_counts(reset=True)
        same_spans(aligner.trim_pair_spans(fq1, fq2), want, pairs, "ragged")
        assert (aligner.trim_counts(reset=True) == counts).all() and (aligner.trim_pair_counts(reset=True) == pairs_c).all()
        assert pairs_c[0] == 20000 and pairs_c[2] > 2000 and not aligner.trim_pair_counts().any()
    finally:
        _off(aligner)


def test_blocks_of_one_pair_and_of_three(aligner):
    o, po, pairs = pc.random_pairs(200, seed=12)
    _set(aligner, o, po)
    try:
        for pick in ([pairs[0]], pairs[5:8], [p for p in pairs if len(p[0][0]) > 150][:1], pairs[100:103]):
            fq1, fq2 = pc.fastq_of_pairs(pick)
            pairs_c = np.zeros(8, dtype=np.uint64)
            aligner.trim_pair_counts(reset=True)
            same_spans(aligner.trim_pair_spans(fq1, fq2), twin_spans(o, po, pick, None, pairs_c), pick, len(pick))
            assert (aligner.trim_pair_counts() == pairs_c).all() and pairs_c[0] == len(pick)
    finally:
        _off(aligner)


def _opt(ix):
    import salt_amd
    return salt_amd.AlnOpt.from_argv(PE_ARGS, ix.l_seed)[0]


@pytest.fixture(scope="module")
def built():
    """the constructed pairs and the twin's trimmed copies, under the pair rule alone ("pair") and with the other steps ("both")"""
    import salt_amd
    fq1, fq2 = pc.constructed_pairs(600, seed=4)
    out = dict(fq1=fq1, fq2=fq2)
    for tag, kw in (("pair", {}), ("both", TRIM)):
        counts, pairs = np.zeros((2, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        out[tag] = salt_amd.trim_fastq_pair(fq1, fq2, counts=counts, pair_counts=pairs, **kw) + (counts, pairs)
    assert out["pair"][3][2] > 150 and len(out["pair"][0]) < len(fq1) - 5000
    return out


def _call(aln, ix, built, tag=None):
    return aln.align_pe_text(_opt(ix), ix, built[tag][0] if tag else built["fq1"], built[tag][1] if tag else built["fq2"])


MODES = {"sam": lambda a, on: None, "bam": lambda a, on: a.set_sam_bam(on), "bgzf": lambda a, on: a.set_sam_bgzf(on), "polish": lambda a, on: a.set_polish(1 if on else 0)}


@pytest.mark.parametrize("tag", ["pair", "both"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_call_with_the_pair_rule_returns_the_block_of_the_pretrimmed_files(mode, tag, aligner, lambda_index, built):
    MODES[mode](aligner, True)
    try:
        want = _call(aligner, lambda_index, built, tag)
        if tag == "both":
            aligner.set_trim(**TRIM)
        aligner.set_trim_pair()
        aligner.trim_counts(reset=True); aligner.trim_pair_counts(reset=True)
        got = _call(aligner, lambda_index, built)
        counts, pairs = aligner.trim_counts(), aligner.trim_pair_counts()
    finally:
        _off(aligner)
        MODES[mode](aligner, False)
    if mode == "bgzf":
        got, want = (gzip.decompress(got[0]), got[1]), (gzip.decompress(want[0]), want[1])
    assert got[1] == want[1] == 600
    if got[0] != want[0]:
        g, w = got[0].split(b"\n"), want[0].split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        raise AssertionError((len(g), len(w), len(bad), [(g[i][:300], w[i][:300]) for i in bad[:2]]))
    assert len(got[0]) > 50000
    assert (counts == built[tag][2]).all() and (pairs == built[tag][3]).all(), (counts, pairs)


def test_the_tallies_see_the_trimmed_mates(aligner, lambda_index, built):
    import salt_amd
    ref_len = sum(c[1] for c in lambda_index.contigs())

    def tables(tag):
        aligner.errprof_enable(True, 0); aligner.stats_enable(True, 0); aligner.disc_enable(True, 20, 20)
        aligner.errprof_table(reset=True); aligner.stats_tables(reset=True); aligner.disc_reset()
        try:
            _call(aligner, lambda_index, built, tag)
            E, R = aligner.errprof_table()
            cells, ct = aligner.stats_tables()
            alt, diff = aligner.disc_fetch(salt_amd.DISC_ALT, 0, ref_len), aligner.disc_fetch(salt_amd.DISC_DIFF, 0, ref_len + 1)
        finally:
            aligner.errprof_enable(False); aligner.stats_enable(False); aligner.disc_enable(False)
        return E, R, cells, ct, alt, diff

    want = tables("both")
    aligner.set_trim(**TRIM); aligner.set_trim_pair()
    try:
        got = tables(None)
    finally:
        _off(aligner)
    for name, g, w in zip(("errprof E", "errprof R", "stats cells", "stats contigs", "discover alt", "discover diff"), got, want):
        assert np.array_equal(g, w), (name, int((g != w).sum()))
    assert want[0].any() and want[2].any()


def test_the_longest_trimmed_read_reaches_the_aligner_not_the_longest_raw_one(aligner, lambda_index):
    """ctl[3]: a pair of two 300-base mates over an insert of 100 is aligned as two reads of 100 -- the aligner's geometry comes from the
    trimmed length, and the block equals the pre-trimmed one's."""
    import random
    import salt_amd
    rng = random.Random(3)
    genome = "".join(l.strip() for l in open(os.path.join(LAMBDA, "genome.fa")).read().split(">")[1].split("\n")[1:]).upper()
    m1, m2 = pc.mates_of(rng, genome[2000:2100], 300, 300)
    fq1, fq2 = pc.fastq_of_pairs([((m1.encode(), b"I" * 300), (m2.encode(), b"I" * 300))])
    t1, t2 = salt_amd.trim_fastq_pair(fq1, fq2)
    assert t1.split(b"\n")[1] == genome[2000:2100].encode() and len(t2.split(b"\n")[1]) == 100
    want = aligner.align_pe_text(_opt(lambda_index), lambda_index, t1, t2)
    aligner.set_trim_pair()
    try:
        got = aligner.align_pe_text(_opt(lambda_index), lambda_index, fq1, fq2)
        assert got == want and got[1] == 1 and b"\t" + genome[2000:2100].encode() + b"\t" in got[0]
    finally:
        _off(aligner)


def test_one_workspace_on_off_and_on_again(aligner, lambda_index, built):
    plain = _call(aligner, lambda_index, built)
    want = _call(aligner, lambda_index, built, "pair")
    assert plain != want
    try:
        aligner.set_trim_pair()
        assert _call(aligner, lambda_index, built) == want
        aligner.set_trim_pair(None)
        assert _call(aligner, lambda_index, built) == plain
        aligner.set_trim_pair(20, 10)
        assert _call(aligner, lambda_index, built) == want
        # the single-end entry point ignores the rule
        se = aligner.align_se_text(salt_amd_opt_se(lambda_index), built["fq1"])
        aligner.set_trim_pair(None)
        assert aligner.align_se_text(salt_amd_opt_se(lambda_index), built["fq1"]) == se
    finally:
        _off(aligner)


def salt_amd_opt_se(ix):
    import salt_amd
    return salt_amd.AlnOpt.from_argv(["-d", "-c"], ix.l_seed)[0]


def test_uncount_takes_back_the_pair_counters_of_the_last_call_and_only_those(aligner, lambda_index, built):
    try:
        aligner.set_trim_pair()
        aligner.trim_counts(reset=True); aligner.trim_pair_counts(reset=True)
        _call(aligner, lambda_index, built)
        _call(aligner, lambda_index, built)
        assert (aligner.trim_pair_counts() == 2 * built["pair"][3]).all() and (aligner.trim_counts() == 2 * built["pair"][2]).all()
        aligner.trim_uncount()
        assert (aligner.trim_pair_counts() == built["pair"][3]).all() and (aligner.trim_counts() == built["pair"][2]).all()
        aligner.trim_uncount()                                       # nothing left to take back
        assert (aligner.trim_pair_counts(reset=True) == built["pair"][3]).all()
    finally:
        _off(aligner)
        aligner.trim_counts(reset=True)


def test_with_the_rule_off_a_call_is_that_of_a_workspace_that_never_set_it(aligner, lambda_index, built):
    import salt_amd
    fresh = _aligner(lambda_index)
    try:
        fresh.set_trim(**TRIM)
        want = _call(fresh, lambda_index, built)
        want_counts = fresh.trim_counts()
    finally:
        fresh.close()
    try:
        aligner.set_trim_pair()
        _call(aligner, lambda_index, built)
        aligner.set_trim_pair(None)
        aligner.set_trim(**TRIM)
        aligner.trim_counts(reset=True); aligner.trim_pair_counts(reset=True)
        assert _call(aligner, lambda_index, built) == want
        assert (aligner.trim_counts() == want_counts).all() and not aligner.trim_pair_counts().any()
        t1, t2 = salt_amd.trim_fastq(built["fq1"], 0, **TRIM), salt_amd.trim_fastq(built["fq2"], 1, **TRIM)
        aligner.set_trim()
        assert aligner.align_pe_text(_opt(lambda_index), lambda_index, t1, t2) == want
    finally:
        _off(aligner)


def test_options_out_of_range_are_refused_by_name_and_change_nothing(aligner, built):
    import salt_amd
    for args, word in (((0, 10), "min_overlap"), ((513, 10), "min_overlap"), ((20, 51), "error_pct")):
        with pytest.raises(salt_amd.SaltError, match=word):
            aligner.set_trim_pair(*args)
    fq1 = b"\n".join(built["fq1"].split(b"\n")[:4]) + b"\n"
    fq2 = b"\n".join(built["fq2"].split(b"\n")[:4]) + b"\n"
    assert (aligner.trim_pair_spans(fq1, fq2) == [[0, 100, 0, 100]]).all() and not aligner.trim_pair_counts(reset=True).any()      # still off
    with pytest.raises(salt_amd.SaltError, match="different numbers of reads"):
        aligner.trim_pair_spans(fq1 + fq1, fq2)


def test_the_rows_entry_refuses_a_workspace_with_the_pair_rule(aligner, lambda_index, built):
    import salt_amd
    rec = b"\n".join(built["fq1"].split(b"\n")[:4]) + b"\n"
    rows = np.zeros(1, dtype=salt_amd.RESULT_DTYPE)
    rows["pos"] = 0xFFFFFFFF
    aligner.set_trim_pair()
    try:
        with pytest.raises(salt_amd.SaltError, match="salt_gpu_ws_set_trim_pair is on"):
            aligner.text_from_rows(salt_amd_opt_se(lambda_index), rec, rows)
    finally:
        _off(aligner)
    assert aligner.text_from_rows(salt_amd_opt_se(lambda_index), rec, rows)[1] == 1


# ---- the driver ----
SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
TRIM_ARGS = ["--trim-adapter", tc.ADAPTER, "--trim-adapter2", tc.ADAPTER2, "--trim-qual", "20"]


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("trimpairidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), p], check=True, stderr=subprocess.DEVNULL)
    return p


def salt(prefix, args, files, env=None):
    p = subprocess.run([SALT] + args + [prefix] + files, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120)
    if p.returncode in (134, 139, -6, -11) or b"illegal memory access" in p.stderr or b"HSA_STATUS_ERROR" in p.stderr:
        pytest.exit("salt died or the device faulted (status %s): %s" % (p.returncode, p.stderr[-600:].decode("latin-1")), returncode=3)
    assert p.returncode == 0, (args, p.stderr[-600:])
    return p


def counters(stderr):
    """the two [salt] trim: lines -> (who trimmed, (2, 8) array, (8,) array)"""
    lines = [l for l in stderr.decode().split("\n") if l.startswith("[salt] trim: ")]
    first = [l for l in lines if "reads_floored" in l]
    second = [l for l in lines if l.startswith("[salt] trim: pairs: ")]
    assert len(first) == 1 and len(second) == 1, stderr[-800:]
    who = first[0][len("[salt] trim: "):].split(":")[0]
    c = np.zeros((2, 8), dtype=np.uint64)
    for m, part in enumerate(first[0].split("mate ")[1:]):
        got = dict(re.findall(r"(\w+) (\d+)", part.split(":", 1)[1]))
        c[m] = [int(got[k]) for k in tc.COUNTERS]
    m = re.fullmatch(r"\[salt\] trim: pairs: pairs (\d+) overlapping (\d+) trimmed (\d+) mate 1: reads (\d+) bases (\d+) mate 2: reads (\d+) bases (\d+) skipped_long (\d+)", second[0])
    assert m, second[0]
    return who, c, np.array([int(x) for x in m.groups()], dtype=np.uint64)


@pytest.fixture(scope="module")
def files(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("trimpairfiles")
    out = {}
    for k, text in (("1", built["fq1"]), ("2", built["fq2"]), ("1_t", built["both"][0]), ("2_t", built["both"][1])):
        out[k] = str(d / (k + ".fq"))
        open(out[k], "wb").write(text)
    return out


def test_the_binary_prints_the_run_on_the_pretrimmed_files_and_the_device_trims(built, files, prefix):
    args = PE_ARGS + ["-t", "8"]
    env = {"SALT_CHUNK_BYTES": "65536"}
    want = salt(prefix, args, [files["1_t"], files["2_t"]], env)
    got = salt(prefix, args + TRIM_ARGS + ["--trim-pair-overlap"], [files["1"], files["2"]], env)
    assert strip_pg(got.stdout) == strip_pg(want.stdout) and len(got.stdout) > 50000
    assert b"text path" in got.stderr and b"[salt] trim:" not in want.stderr
    who, c, p = counters(got.stderr)
    assert who == "device" and (c == built["both"][2]).all() and (p == built["both"][3]).all(), (who, c, p)


def test_a_file_that_crosses_the_hand_over_is_pair_trimmed_on_both_sides_of_it(prefix, tmp_path):
    """A multi-line record in the middle of the mates' file: the device trims the blocks in front of it, the host parser the rest; every pair
    is counted once."""
    import salt_amd
    fq1, fq2 = pc.constructed_pairs(1800, seed=6)                  # the head of a file that the driver looks at is 256 KiB: the record lies behind it
    counts, pairs = np.zeros((2, 8), dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    t1, t2 = salt_amd.trim_fastq_pair(fq1, fq2, counts=counts, pair_counts=pairs, **TRIM)
    recs = fq2.split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        # eight lines, so that the file still holds a multiple of four: the scan of the lines lets the device start, its parser refuses the chunk
        out += [r[0], r[1][:40], r[1][40:70], r[1][70:], r[2], r[3][:15], r[3][15:50], r[3][50:]] if i == 1500 else r
    paths = {}
    for name, text in (("1", fq1), ("2", b"\n".join(out) + b"\n"), ("1_t", t1), ("2_t", t2)):
        paths[name] = str(tmp_path / (name + ".fq"))
        open(paths[name], "wb").write(text)
    env = {"SALT_CHUNK_BYTES": "65536"}
    want = salt(prefix, PE_ARGS + ["-t", "8"], [paths["1_t"], paths["2_t"]], env)
    got = salt(prefix, PE_ARGS + ["-t", "8"] + TRIM_ARGS + ["--trim-pair-overlap"], [paths["1"], paths["2"]], env)
    assert b"the host parser takes over" in got.stderr
    assert strip_pg(got.stdout) == strip_pg(want.stdout)
    who, c, p = counters(got.stderr)
    assert who.startswith("device, and host") and (c == counts).all() and (p == pairs).all() and p[0] == 1800, (who, c, p)
