"""Trimming on the device (k_fq_trim, salt_trim.hip) against the host twin (salt_amd.trim_span / trim_fastq, which
test_trim_host.py holds against the plain Python statement of the rule): the kernel alone through GpuAligner.trim_spans on the edge-case set
and a ragged random block, its counters, the capacity rule on the trimmed length; then the contract -- a text call with set_trim returns the
block the same call returns without it on the twin's trimmed FASTQ, in every output mode, for the tallies too, and back to the plain block
with set_trim off."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from bgzf_check import strip_pg
import trim_check as tc
from conftest import LAMBDA, ROOT

pytestmark = pytest.mark.gpu

SE_ARGS = ["-d", "-c"]
PE_ARGS = ["-d", "-p", "-c", "-a", "350", "-b", "650"]
TRIM = tc.opts(adapter=tc.ADAPTER, adapter2=tc.ADAPTER2, qual=20)


@pytest.fixture(scope="module")
def lambda_index():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield ix
    ix.destroy()


@pytest.fixture(scope="module")
def aligner(lambda_index):
    import salt_amd
    aln = salt_amd.GpuAligner(lambda_index, device=0, max_reads=20480)
    aln.set_contigs(lambda_index)
    aln.set_pac(lambda_index)
    yield aln
    aln.close()


def twin_spans(o, mate, reads, counts=None):
    import salt_amd
    return np.array([salt_amd.trim_span(s, q, mate=mate, adapter=o["adapter"], adapter2=o["adapter2"], qual_min=o["qual"], front=o["front"], tail=o["tail"],
                                        min_overlap=o["min_overlap"], error_pct=o["error_pct"], counts=counts) for s, q in reads], dtype=np.uint32).reshape(-1, 2)


def same_spans(got, want, reads, what):
    bad = np.argwhere((got != want).any(axis=1)).reshape(-1)
    assert got.shape == want.shape and not len(bad), (what, len(bad), [(int(i), reads[i], got[i].tolist(), want[i].tolist()) for i in bad[:3]])


def test_spans_equal_the_twin_on_the_edge_case_set_for_both_mates(aligner):
    counts = np.zeros((2, 8), dtype=np.uint64)
    aligner.trim_counts(reset=True)
    n = 0
    try:
        for o, _, reads in tc.group(tc.edge_cases()):
            aligner.set_trim(**o)
            block = tc.fastq_of(reads)
            for mate in (0, 1):
                same_spans(aligner.trim_spans(block, mate), twin_spans(o, mate, reads, counts), reads, (o, mate))
                n += len(reads)
    finally:
        aligner.set_trim()
    assert n > 6000
    assert (aligner.trim_counts() == counts).all(), (aligner.trim_counts(), counts)


@pytest.fixture(scope="module")
def ragged():
    return tc.random_block(20000, seed=7)


def test_spans_and_counters_equal_the_twin_on_20000_ragged_records(aligner, ragged):
    """Lengths 1 to 512 in one block: records start in every lane of a block's four waves, waves run out of records at different times."""
    o, reads = ragged
    block = tc.fastq_of(reads)
    aligner.set_trim(**o)
    try:
        for mate in (0, 1):
            counts = np.zeros((2, 8), dtype=np.uint64)
            aligner.trim_counts(reset=True)
            same_spans(aligner.trim_spans(block, mate), twin_spans(o, mate, reads, counts), reads, mate)
            got = aligner.trim_counts(reset=True)
            assert (got == counts).all(), (mate, got, counts)
            assert counts[mate][0] == 20000 and counts[mate][7] > 100 and not aligner.trim_counts().any()
    finally:
        aligner.set_trim()


def test_a_block_of_one_record_and_a_block_whose_every_read_floors(aligner):
    ad = tc.ADAPTER
    one = [(b"ACGTTGCATT" + ad.encode()[:20], b"I" * 25 + b"#" * 5)]
    floors = [((ad + "ACGT" * k)[:33 + k].encode(), b"I" * (33 + k)) for k in range(300)] + [(b"ACGT" * 25, b"#" * 100)] * 40 + [(b"A", b"I")]
    o = tc.opts(adapter=ad, qual=20)
    aligner.set_trim(**o)
    try:
        for reads in (one, floors):
            got = aligner.trim_spans(tc.fastq_of(reads))
            same_spans(got, twin_spans(o, 0, reads), reads, len(reads))
        assert (got == [0, 1]).all()
    finally:
        aligner.set_trim()


def _opt(ix, paired):
    import salt_amd
    return salt_amd.AlnOpt.from_argv(PE_ARGS if paired else SE_ARGS, ix.l_seed)[0]


def test_the_length_limit_applies_to_the_trimmed_read(aligner, lambda_index):
    import salt_amd
    rec = open(os.path.join(LAMBDA, "reads_se.fq"), "rb").read().split(b"\n")[:4]
    genome = b"".join(open(os.path.join(LAMBDA, "genome.fa"), "rb").read().split(b">")[1].split(b"\n")[1:])          # the first contig
    long_read = genome[1000:1500] + tc.ADAPTER.encode() + b"ACGT" * 17                           # 500 + 33 + 68 = 601 bases, 500 behind the adapter
    block = b"\n".join(rec) + b"\n@long\n" + long_read + b"\n+\n" + b"I" * len(long_read) + b"\n"
    o = tc.opts(adapter=tc.ADAPTER)
    opt = _opt(lambda_index, False)
    plain = aligner.align_se_text(opt, salt_amd.trim_fastq(block, **o))
    aligner.set_trim(**o)
    try:
        assert aligner.align_se_text(opt, block) == plain and plain[1] == 2
        assert b"\t" + long_read[:500] + b"\t" in plain[0]
        # the adapter damaged: nothing to trim, 601 bases reach the aligner's limit
        spoilt = block.replace(tc.ADAPTER.encode(), tc.ADAPTER.encode()[:8] + b"N" * 25)
        with pytest.raises(salt_amd.SaltError, match=r"read longer than SALT_MAX_READ_LEN \(512\)"):
            aligner.align_se_text(opt, spoilt)
        assert aligner.align_se_text(opt, block) == plain                                         # the workspace stays usable
    finally:
        aligner.set_trim()


@pytest.fixture(scope="module")
def built():
    """the constructed reads and the twin's trimmed copies: (se, se_trimmed, pe1, pe2, pe1_trimmed, pe2_trimmed, twin counters)"""
    import salt_amd
    se = tc.constructed("reads_se.fq", tc.ADAPTER, 1)
    pe1, pe2 = tc.constructed("reads_pe_1.fq", tc.ADAPTER, 2), tc.constructed("reads_pe_2.fq", tc.ADAPTER2, 3)
    c_se, c_pe = np.zeros((2, 8), dtype=np.uint64), np.zeros((2, 8), dtype=np.uint64)
    out = dict(se=se, pe1=pe1, pe2=pe2, se_t=salt_amd.trim_fastq(se, 0, counts=c_se, **TRIM), pe1_t=salt_amd.trim_fastq(pe1, 0, counts=c_pe, **TRIM),
               pe2_t=salt_amd.trim_fastq(pe2, 1, counts=c_pe, **TRIM), c_se=c_se, c_pe=c_pe)
    assert c_se[0][5] > 500 and c_se[0][3] > 500 and c_pe[1][5] > 250 and len(out["se_t"]) < len(se) - 50000
    return out


def _call(aln, ix, paired, b, trimmed):
    if paired:
        return aln.align_pe_text(_opt(ix, True), ix, b["pe1_t" if trimmed else "pe1"], b["pe2_t" if trimmed else "pe2"])
    return aln.align_se_text(_opt(ix, False), b["se_t" if trimmed else "se"])


MODES = {"sam": lambda a, on: None, "bam": lambda a, on: a.set_sam_bam(on), "bgzf": lambda a, on: a.set_sam_bgzf(on), "polish": lambda a, on: a.set_polish(1 if on else 0)}


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_a_trimming_call_returns_the_block_of_the_pretrimmed_text(mode, paired, aligner, lambda_index, built):
    MODES[mode](aligner, True)
    try:
        want = _call(aligner, lambda_index, paired, built, True)
        aligner.set_trim(**TRIM)
        aligner.trim_counts(reset=True)
        got = _call(aligner, lambda_index, paired, built, False)
        counts = aligner.trim_counts()
    finally:
        aligner.set_trim()
        MODES[mode](aligner, False)
    if mode == "bgzf":
        got, want = (gzip.decompress(got[0]), got[1]), (gzip.decompress(want[0]), want[1])              # (blocks without the end-of-file block: that one is the caller's)
    assert got[1] == want[1] == (1000 if paired else 2000)
    if got[0] != want[0]:
        g, w = got[0].split(b"\n"), want[0].split(b"\n")
        bad = [i for i in range(min(len(g), len(w))) if g[i] != w[i]]
        raise AssertionError((len(g), len(w), len(bad), [(g[i][:300], w[i][:300]) for i in bad[:2]]))
    assert len(got[0]) > 100000
    assert (counts == built["c_pe" if paired else "c_se"]).all()


def test_the_single_end_block_is_the_oracles_sam_of_the_trimmed_reads(aligner, lambda_index, built, oracle_cli, tmp_path):
    fq = tmp_path / "trimmed.fq"
    fq.write_bytes(built["se_t"])
    want = subprocess.run([oracle_cli, "-d", "-c", os.path.join(LAMBDA, "idx"), str(fq)], check=True, capture_output=True).stdout
    want = b"".join(l for l in want.splitlines(keepends=True) if not l.startswith(b"@"))
    aligner.set_trim(**TRIM)
    try:
        got, n = _call(aligner, lambda_index, False, built, False)
    finally:
        aligner.set_trim()
    assert n == 2000 and got == want


@pytest.mark.parametrize("paired", [False, True], ids=["se", "pe"])
def test_the_tallies_see_the_trimmed_read(paired, aligner, lambda_index, built):
    """Error profile (cycles and qualities from the raw block through the moved offsets), summary tables (read lengths, clipped bases) and
    SNP candidates (base qualities) after a trimmed call equal those after the plain call on the pre-trimmed text."""
    import salt_amd
    ref_len = sum(c[1] for c in lambda_index.contigs())

    def tables(trimmed):
        aligner.errprof_enable(True, 0); aligner.stats_enable(True, 0); aligner.disc_enable(True, 20, 20)
        aligner.errprof_table(reset=True); aligner.stats_tables(reset=True); aligner.disc_reset()
        try:
            _call(aligner, lambda_index, paired, built, trimmed)
            E, R = aligner.errprof_table()
            cells, ct = aligner.stats_tables()
            alt, diff = aligner.disc_fetch(salt_amd.DISC_ALT, 0, ref_len), aligner.disc_fetch(salt_amd.DISC_DIFF, 0, ref_len + 1)
        finally:
            aligner.errprof_enable(False); aligner.stats_enable(False); aligner.disc_enable(False)
        return E, R, cells, ct, alt, diff

    want = tables(True)
    aligner.set_trim(**TRIM)
    try:
        got = tables(False)
    finally:
        aligner.set_trim()
    for name, g, w in zip(("errprof E", "errprof R", "stats cells", "stats contigs", "discover alt", "discover diff"), got, want):
        assert np.array_equal(g, w), (name, int((g != w).sum()))
    assert want[0].any() and want[2].any() and want[4].any()


def test_one_workspace_on_off_and_on_again(aligner, lambda_index, built):
    plain = _call(aligner, lambda_index, False, built, False)
    want = _call(aligner, lambda_index, False, built, True)
    assert plain != want
    aligner.set_trim(**TRIM)
    try:
        assert _call(aligner, lambda_index, False, built, False) == want
        aligner.set_trim()
        assert _call(aligner, lambda_index, False, built, False) == plain
        assert _call(aligner, lambda_index, True, built, False) == _call(aligner, lambda_index, True, built, False)
        aligner.set_trim(**TRIM)
        assert _call(aligner, lambda_index, False, built, False) == want
    finally:
        aligner.set_trim()


def test_uncount_takes_back_the_last_call_and_only_that(aligner, lambda_index, built):
    """What the driver does with a block it aligned and then drops at a hand-over: the call's counters leave, earlier calls' stay."""
    aligner.set_trim(**TRIM)
    try:
        aligner.trim_counts(reset=True)
        _call(aligner, lambda_index, True, built, False)
        _call(aligner, lambda_index, False, built, False)
        assert (aligner.trim_counts() == built["c_se"] + built["c_pe"]).all()
        aligner.trim_uncount()
        assert (aligner.trim_counts() == built["c_pe"]).all()
        aligner.trim_uncount()                                       # nothing left to take back
        assert (aligner.trim_counts(reset=True) == built["c_pe"]).all()
    finally:
        aligner.set_trim()


def test_options_out_of_range_are_refused_by_name_and_change_nothing(aligner, built, lambda_index):
    import salt_amd
    for kw, word in ((dict(adapter="ACGN"), "adapter holds a letter"), (dict(adapter2="ACGT"), "adapter2 without adapter"), (dict(adapter="ACGT", min_overlap=65), "min_overlap"),
                     (dict(adapter="ACGT", error_pct=51), "error_pct"), (dict(qual=94), "qual"), (dict(front=512), "front"), (dict(tail=512), "tail")):
        with pytest.raises(salt_amd.SaltError, match=word):
            aligner.set_trim(**kw)
    rec = b"\n".join(built["se"].split(b"\n")[:8]) + b"\n"
    assert (aligner.trim_spans(rec) == [[0, 100], [0, 100]]).all()                      # still off


def test_the_rows_entry_refuses_a_trimming_workspace(aligner, lambda_index, built):
    import salt_amd
    rec = b"\n".join(built["se"].split(b"\n")[:4]) + b"\n"
    rows = np.zeros(1, dtype=salt_amd.RESULT_DTYPE)
    rows["pos"] = 0xFFFFFFFF
    aligner.set_trim(**TRIM)
    try:
        with pytest.raises(salt_amd.SaltError, match="salt_gpu_ws_set_trim is on"):
            aligner.text_from_rows(_opt(lambda_index, False), rec, rows)
    finally:
        aligner.set_trim()
    assert aligner.text_from_rows(_opt(lambda_index, False), rec, rows)[1] == 1


# ---- the driver ----
SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")
TRIM_ARGS = ["--trim-adapter", tc.ADAPTER, "--trim-adapter2", tc.ADAPTER2, "--trim-qual", "20"]


@pytest.fixture(scope="module")
def prefix(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("trimidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), p], check=True, stderr=subprocess.DEVNULL)
    return p


def salt(prefix, args, files, env=None):
    p = subprocess.run([SALT] + args + [prefix] + files, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120)
    if p.returncode in (134, 139, -6, -11) or b"illegal memory access" in p.stderr or b"HSA_STATUS_ERROR" in p.stderr:
        pytest.exit("salt died or the device faulted (status %s): %s" % (p.returncode, p.stderr[-600:].decode("latin-1")), returncode=3)
    assert p.returncode == 0, (args, p.stderr[-600:])
    return p


def counters(stderr):
    """the [salt] trim: line -> (who trimmed, (2, 8) array in trim_check.COUNTERS' order)"""
    lines = [l for l in stderr.decode().split("\n") if l.startswith("[salt] trim: ") and "mate 1" in l]
    assert len(lines) == 1, stderr[-800:]
    who = lines[0][len("[salt] trim: "):].split(":")[0]
    c = np.zeros((2, 8), dtype=np.uint64)
    for m, part in enumerate(lines[0].split("mate ")[1:]):
        got = dict(re.findall(r"(\w+) (\d+)", part.split(":", 1)[1]))
        c[m] = [int(got[k]) for k in tc.COUNTERS]
    return who, c


@pytest.fixture(scope="module")
def files(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("trimfiles")
    out = {}
    for k in ("se", "se_t", "pe1", "pe1_t", "pe2", "pe2_t"):
        out[k] = str(d / (k + ".fq"))
        open(out[k], "wb").write(built[k])
    return out


@pytest.mark.parametrize("case", ["se_default", "pe_default"])
def test_the_binary_prints_the_run_on_the_pretrimmed_reads_and_the_device_trims(case, built, files, prefix):
    args = (SE_ARGS if case == "se_default" else PE_ARGS) + ["-t", "8"]
    names = ["se"] if case == "se_default" else ["pe1", "pe2"]
    env = {"SALT_CHUNK_BYTES": "65536"}
    want = salt(prefix, args, [files[n + "_t"] for n in names], env)
    got = salt(prefix, args + TRIM_ARGS, [files[n] for n in names], env)
    assert strip_pg(got.stdout) == strip_pg(want.stdout) and len(got.stdout) > 100000
    assert b"text path" in got.stderr and b"[salt] trim:" not in want.stderr
    who, c = counters(got.stderr)
    assert who == "device" and (c == built["c_se" if case == "se_default" else "c_pe"]).all(), (who, c)


def test_a_file_that_crosses_the_hand_over_is_trimmed_on_both_sides_of_it(built, files, prefix, tmp_path):
    """A multi-line record in the middle: the device trims the blocks in front of it, the host parser the rest; every read is counted once."""
    recs = built["se"].split(b"\n")
    recs = [recs[i:i + 4] for i in range(0, len(recs) - 3, 4)]
    out = []
    for i, r in enumerate(recs):
        out += [r[0], r[1][:40], r[1][40:], r[2], r[3][:15], r[3][15:]] if i == 1500 else r
    fq = tmp_path / "mid_multiline.fq"
    fq.write_bytes(b"\n".join(out) + b"\n")
    env = {"SALT_CHUNK_BYTES": "65536"}
    want = salt(prefix, SE_ARGS + ["-t", "8"], [files["se_t"]], env)
    got = salt(prefix, SE_ARGS + ["-t", "8"] + TRIM_ARGS, [str(fq)], env)
    assert b"the host parser takes over" in got.stderr
    assert strip_pg(got.stdout) == strip_pg(want.stdout)
    who, c = counters(got.stderr)
    assert who.startswith("device, and host") and (c == built["c_se"]).all(), (who, c)
