"""`salt --polish` without a GPU.  The record-to-hits rule of the fused route (pl_row_hits of salt_amd/csrc/salt_polish_text.h, the source
k_pl_rows of salt_polish.hip compiles) takes a record's hits straight from its result row; the route it replaces formats the row as a SAM
line (aln_samse / alnpe_sam with sam_add_xa) and parses the line back (pl_parse + pl_hits).  tools/polish_fuse_model.cc runs both on the
host under AddressSanitizer + UBSan and fails on any difference in the (strand, offset, pos, contig name) lists: on the oracle's rows for
the fixtures -- many alternative hits, ragged lengths with N, pairs -- with the lines the product's host formatter makes of them, and on
hand-made rows for what the fixtures do not reach.  Then the command line: the option's refusals come before any device call."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import LAMBDA, ROOT
from salt_amd.api import RESULT_DTYPE

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")
ANN = os.path.join(LAMBDA, "idx.C.ann")
SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("fusemodel")
    exe = str(d / "polish_fuse_model.san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tools", "polish_fuse_model.cc")], check=True)
    return exe


@pytest.fixture(scope="module")
def index(oracle_lib):
    import salt_amd
    idx = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield idx
    idx.destroy()


def run_model(exe, tmp_path, rows, lines, paired):
    (tmp_path / "rows.bin").write_bytes(np.ascontiguousarray(rows).tobytes())
    (tmp_path / "lines.sam").write_bytes(b"".join(l + b"\n" for l in lines))
    p = subprocess.run([exe] + (["-p"] if paired else []) + [ANN, str(tmp_path / "rows.bin"), str(tmp_path / "lines.sam")], capture_output=True, env=SAN_ENV, timeout=300)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode in (0, 1), (p.returncode, p.stderr[-500:])
    out = p.stdout.decode("latin-1").split("\n")[:-1]
    summary = dict(zip(out[-1].split(" ")[0::2], map(int, out[-1].split(" ")[1::2])))
    return p.returncode, out[:-1], summary


def se_lines(index, opt, names, seqs, offs, quals, rows):
    return [index.samse(opt, names[i], seqs[offs[i]:offs[i + 1]], quals[i], rows[i:i + 1]) for i in range(len(names))]


def pe_lines(index, opt, names, seqs, offs, quals, rows):
    out = []
    for i in range(0, len(names), 2):
        two = index.sampe(opt, names[i:i + 2], [seqs[offs[i]:offs[i + 1]], seqs[offs[i + 1]:offs[i + 2]]], quals[i:i + 2], rows[i:i + 2])
        recs = [l for l in two.split(b"\n") if l]                # without the driver's blank line behind every record
        assert len(recs) == 2
        out += recs
    return out


def oracle_rows(argv, files, l_seed):
    import salt_amd
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_py
    prefix = os.path.join(LAMBDA, "idx")
    ora = oracle_py.Oracle(prefix)
    opt, _ = salt_amd.AlnOpt.from_argv(argv, l_seed)
    oo = ora.opt(l_overlap=opt.l_overlap, max_seed=opt.max_seed, max_locate=opt.max_locate, seed_only_ref=opt.seed_only_ref)
    if len(files) == 1:
        reads = salt_amd.read_fastq(os.path.join(LAMBDA, files[0]))
        rows = ora.align(oo, reads[1], reads[2], n_threads=8)
    else:
        reads = salt_amd.interleave_pairs(*[salt_amd.read_fastq(os.path.join(LAMBDA, f)) for f in files])
        rows = ora.align_pe(oo, reads[1], reads[2], min_tlen=opt.min_tlen, max_tlen=opt.max_tlen, n_threads=8)
    ora.close()
    return opt, reads, product_rows(rows)


def product_rows(ora):
    """the oracle's rows in the product's layout (salt_result_t): the fields a SAM line is made of; the CIGAR from its text"""
    import re
    rows = np.zeros(len(ora), dtype=RESULT_DTYPE)
    for f in ("pos", "n_diff", "is_gap", "mapq", "b0", "b1", "seq_start", "seq_end", "n_hits", "hits"):
        rows[f] = ora[f]
    rows["strand"] = ora["strand"] & 0xFF
    for i, text in enumerate(ora["cigar"]):
        ops = [(int(n) << 4) | b"MID".index(c) for n, c in re.findall(rb"(\d+)([MID])", text)]
        assert bool(ops) == (ora["pos"][i] != 0xFFFFFFFF) and len(ops) <= 64
        rows["n_cigar"][i] = len(ops)
        rows["cigar"][i, :len(ops)] = ops
    return rows


FIXTURES = {
    "se_r1_m500": (["-r", "1", "-m", "500"], ["reads_se.fq"]),
    "ragged": ([], ["reads_ragged.fq"]),
    "pe": (["-p", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"]),
}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_the_hits_of_a_row_are_the_hits_of_its_sam_line_on_the_fixtures(name, model, index, tmp_path):
    argv, files = FIXTURES[name]
    opt, (names, seqs, offs, quals), rows = oracle_rows(argv, files, index.l_seed)
    paired = len(files) == 2
    lines = (pe_lines if paired else se_lines)(index, opt, names, seqs, offs, quals, rows)
    rc, diffs, summary = run_model(model, tmp_path, rows, lines, paired)
    assert rc == 0 and not diffs, diffs[:5]
    assert summary["rows"] == len(names) and summary["differences"] == 0
    # the fixture does what it is here for: alternative hits beside the primaries / skipped-free ragged reads with N / both strands
    n_mapped = int((rows["pos"] != 0xFFFFFFFF).sum())
    assert n_mapped > 0.8 * len(names)
    if name == "se_r1_m500":
        assert summary["hits"] > n_mapped and int(rows["n_hits"].sum()) >= summary["hits"] - n_mapped > 0
    if name == "ragged":
        assert sum(1 for i in range(len(names)) if (seqs[offs[i]:offs[i + 1]] == 4).any()) >= 20


def hand_rows():
    """rows the fixtures do not reach, with the reads they are printed with: (rows, paired)"""
    D = RESULT_DTYPE

    def row(pos=0xFFFFFFFF, strand=3, hits=((), ()), L=100):
        r = np.zeros(1, dtype=D)
        r["pos"], r["strand"], r["n_diff"], r["is_gap"], r["mapq"] = pos, strand, (255 if pos == 0xFFFFFFFF else 0), (255 if pos == 0xFFFFFFFF else 0), 0
        if pos != 0xFFFFFFFF:
            r["n_cigar"] = 1
            r["cigar"][0, 0] = (L << 4)
            r["seq_end"] = L - 1
        for s in (0, 1):
            r["n_hits"][0, s] = len(hits[s])
            for k, p in enumerate(hits[s]):
                r["hits"][0, s, k]["pos"], r["hits"][0, s, k]["n_diff"], r["hits"][0, s, k]["strand"] = p, 1, s
        return r
    se = np.concatenate([
        row(),                                                                   # unmapped
        row(1000, 0, ((), (1000,))),                                             # the only alternative hit: the primary's position, other strand
        row(50000, 1, ((100, 2000, 30000, 48400, 60000), ())),                   # five hits on one strand (both contigs), the primary on the other
        row(2000, 0, ((2000, 48502), (70000, 100))),                             # the primary among its own strand's hits; a hit at the second contig's first base
    ])
    pe = np.concatenate([
        row(), row(3000, 1, ((), (3400,))),                                      # own mate unmapped, the other mapped: flag 4 and the mate's RNAME, no primary
        row(4000, 0, ((4100,), ())), row(),                                      # ... and the other way round
        row(hits=((500,), (900,))), row(),                                       # an unmapped mate that still carries hits: they are printed, and read
    ])
    return se, pe


@pytest.mark.parametrize("paired", [False, True])
def test_the_hits_of_hand_made_rows_are_the_hits_of_their_sam_lines(paired, model, index, tmp_path):
    import salt_amd
    rows = hand_rows()[1 if paired else 0]
    n, L = len(rows), 100
    rng = np.random.default_rng(3)
    seqs = rng.integers(0, 4, n * L).astype(np.uint8)
    offs = (np.arange(n + 1) * L).astype(np.uint32)
    names = [b"hand%d" % (i // 2 if paired else i) for i in range(n)]
    quals = [b"I" * L] * n
    opt = salt_amd.AlnOpt(l_seed=index.l_seed, paired=1 if paired else 0, min_tlen=350, max_tlen=650)
    lines = (pe_lines if paired else se_lines)(index, opt, names, seqs, offs, quals, rows)
    rc, diffs, summary = run_model(model, tmp_path, rows, lines, paired)
    assert rc == 0 and not diffs, diffs
    f = [l.split(b"\t") for l in lines]
    if not paired:
        assert f[0][1] == b"4" and f[0][2] == b"*" and len(f[0]) == 11      # unmapped: no tags
        assert not any(x.startswith(b"XA") for x in f[1])                  # the hit at the primary's position is not printed
        assert f[2][1] == b"16" and [x for x in f[2] if x.startswith(b"XA")][0].count(b";") == 5
        assert summary["hits"] == 0 + 1 + 6 + 4
    else:
        assert int(f[0][1]) & 4 and f[0][2] != b"*" and int(f[1][1]) & 8    # printed at its mate's place
        assert int(f[4][1]) & 4 and any(x.startswith(b"XA") for x in f[4])
        assert summary["hits"] == (0 + 2) + (2 + 0) + (2 + 0)


def test_the_model_reports_a_row_whose_line_says_something_else(model, index, tmp_path):
    """the check can fail: a line with one XA item less, a line on the other strand"""
    import salt_amd
    rows = hand_rows()[0][2:3]
    opt = salt_amd.AlnOpt(l_seed=index.l_seed)
    seq = np.zeros(100, dtype=np.uint8)
    line = index.samse(opt, b"r", seq, b"I" * 100, rows)
    cut = line[:line.rindex(b";", 0, len(line) - 1) + 1]
    for bad in (cut, line.replace(b"\t16\t", b"\t0\t", 1)):
        assert bad != line
        rc, diffs, summary = run_model(model, tmp_path, rows, [bad], False)
        assert rc == 1 and len(diffs) == 1 and summary["differences"] == 1


def run_salt(args):
    return subprocess.run([SALT] + args, capture_output=True, timeout=120)


def test_polish_with_bam_is_refused_while_the_options_are_read():
    p = run_salt(["--polish", "--bam", "/nonexistent/idx", "/nonexistent/reads.fq"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"--polish" in p.stderr and b"--bam" in p.stderr
    assert b"Reload index" not in p.stderr                                  # before the index is touched, let alone a device
    p = run_salt(["--bam", "--polish=sw", "/nonexistent/idx", "/nonexistent/reads.fq"])
    assert p.returncode == 1 and b"--polish" in p.stderr and b"--bam" in p.stderr


def test_an_unknown_polish_mode_is_refused_while_the_options_are_read():
    p = run_salt(["--polish=nope", "/nonexistent/idx", "/nonexistent/reads.fq"])
    assert p.returncode == 1 and p.stdout == b""
    assert b"--polish=nope" in p.stderr and b"lv" in p.stderr and b"sw" in p.stderr
    assert b"Reload index" not in p.stderr


def test_the_usage_lists_the_option():
    p = run_salt(["-h"])
    assert b"--polish[=lv|sw]" in p.stderr
