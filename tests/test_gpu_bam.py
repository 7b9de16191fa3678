"""`salt --bam` on the device.  The record kernels (k_bam_len / k_bam_write) through the API -- BAM on, BGZF off: the raw record bytes of a
text call -- against the host encoder on the SAM text of the same call, byte for byte; then the `salt` binary with the option through the
text path (single and paired end), every leg a child process under its own time limit, decoded by tests/bam_check.py."""
import os
import subprocess

import pytest

import bam_check
from bgzf_check import EOF, strip_pg
from conftest import EXTRA_CASES, LAMBDA, ROOT, read_cases

pytestmark = pytest.mark.gpu

SALT = os.path.join(ROOT, "salt_amd", "bin", "salt")
SALT_IDX = os.path.join(ROOT, "salt_amd", "bin", "salt-idx")


def _golden(case):
    return open(os.path.join(LAMBDA, "expect_%s.sam" % case), "rb").read()


def _fq(name):
    return open(os.path.join(LAMBDA, name), "rb").read()


def _opt(ix, args):
    import salt_amd
    return salt_amd.AlnOpt.from_argv(list(args), ix.l_seed)[0]


def _both(ix, args, fastqs, max_reads=8192):
    """(the SAM text, the BAM records) of the same text call on one workspace, BAM off and on."""
    import salt_amd
    opt = _opt(ix, args)
    aln = salt_amd.GpuAligner(ix, device=0, max_reads=max_reads)
    try:
        aln.set_contigs(ix)
        call = (lambda: aln.align_pe_text(opt, ix, *fastqs)) if len(fastqs) == 2 else (lambda: aln.align_se_text(opt, fastqs[0]))
        sam, n = call()
        aln.set_sam_bam(True)
        bam, n2 = call()
        assert (bam, n2) == call(), "two BAM calls gave different bytes"
        aln.set_sam_bam(False)
        assert call() == (sam, n) and n2 == n
    finally:
        aln.close()
    return sam, bam


def _same_as_the_host_encoder(ix, sam, bam):
    import salt_amd
    want = salt_amd.bam_from_sam(ix, sam)
    if bam != want:
        refs = [(nm, ln) for _, ln, nm in ix.contigs()]
        a, b = bam_check.records(want, 0, refs), None
        try:
            b = bam_check.records(bam, 0, refs)
        except AssertionError as e:
            raise AssertionError("device records do not parse: %s" % e)
        bad = [(x["sam"][:200], x["bytes"].hex()[:120], y["bytes"].hex()[:120]) for x, y in zip(a, b) if x["bytes"] != y["bytes"]]
        raise AssertionError("%d / %d records differ (%d / %d bytes); first: %r" % (len(bad), len(a), len(bam), len(want), bad[:1]))
    return want


@pytest.fixture(scope="module")
def lambda_index():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield ix
    ix.destroy()


SETS = {
    "se_default": (["-d", "-c"], ["reads_se.fq"]), "se_plain": ([], ["reads_se.fq"]), "se_r1_m500": (["-d", "-c", "-r", "1", "-m", "500"], ["reads_se.fq"]),
    "se_rg": (["-d", "-g", "grp1"], ["reads_se.fq"]),
    "pe_default": (["-d", "-p", "-c", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"]),
    "pe_plain": (["-p", "-a", "350", "-b", "650"], ["reads_pe_1.fq", "reads_pe_2.fq"]),
    "ragged_default": EXTRA_CASES["ragged_default"], "ragged_pe": EXTRA_CASES["ragged_pe"], "span_default": EXTRA_CASES["span_default"],
}


@pytest.mark.parametrize("name", sorted(SETS))
def test_device_records_equal_the_host_encoder_byte_for_byte(name, lambda_index):
    args, files = SETS[name]
    sam, bam = _both(lambda_index, args, [_fq(f) for f in files])
    golden = {"se_default": "se_default", "se_plain": "se_plain_t4", "pe_default": "pe_default", "ragged_default": "ragged_default",
              "ragged_pe": "ragged_pe", "span_default": "span_default", "se_r1_m500": "se_r1_m500"}.get(name)
    if golden:                                                     # the SAM side of the comparison is the golden text
        assert sam == b"".join(l for l in _golden(golden).splitlines(keepends=True) if not l.startswith(b"@"))
    want = _same_as_the_host_encoder(lambda_index, sam, bam)
    refs = [(nm, ln) for _, ln, nm in lambda_index.contigs()]
    assert bam_check.decode_records(bam, refs) == bam_check.sam_records(sam) and len(want) > 1000
    if name.startswith("ragged"):                                  # odd lengths: the last nibble
        assert any(r["l_seq"] & 1 for r in bam_check.records(bam, 0, refs))


def test_bins_of_reads_at_the_16_kb_edges(lambda_index):
    """Reads that end on, or start next to, a multiple of 16 384: bin from POS - 1, not from POS."""
    sam, bam = _both(lambda_index, ["-d", "-c"], [bam_check.boundary_reads(os.path.join(LAMBDA, "genome.fa"))])
    _same_as_the_host_encoder(lambda_index, sam, bam)
    recs = bam_check.records(bam, 0, [(nm, ln) for _, ln, nm in lambda_index.contigs()])
    assert {r["pos"] for r in recs} >= {16284, 16383, 16384, 32668, 32767, 32768} and {r["bin"] for r in recs} >= {4681, 4682, 4683, 585}


def test_records_that_outgrow_their_slot_and_long_names(tmp_path):
    """Names of up to 254 bytes (the name is copied by the lanes, from the FASTQ text), and tags beyond the 224 bytes of the slot's tail: a
    contig name of 240 characters makes every XA list that names it outgrow the tail, and such a record is written whole by one lane."""
    import salt_amd
    fa = open(os.path.join(LAMBDA, "genome.fa"), "rb").read().split(b"\n")
    names = [l[1:].split()[0] for l in fa if l.startswith(b">")]
    long_of = {n: (n if k == 0 else n + b"_" + b"x" * (239 - len(n))) for k, n in enumerate(names)}
    (tmp_path / "g.fa").write_bytes(b"\n".join((b">" + long_of[l[1:].split()[0]]) if l.startswith(b">") else l for l in fa))
    snps = open(os.path.join(LAMBDA, "snps.txt"), "rb").read().split(b"\n")
    (tmp_path / "s.txt").write_bytes(b"\n".join(l for l in snps if l.split(b"\t")[0] == names[0]) + b"\n")
    prefix = str(tmp_path / "idx")
    subprocess.run([SALT_IDX, "-k", "19", str(tmp_path / "g.fa"), str(tmp_path / "s.txt"), prefix], check=True, stderr=subprocess.DEVNULL, timeout=600)
    ix = salt_amd.Index.reload(prefix)
    try:
        refs = [(nm, ln) for _, ln, nm in ix.contigs()]
        for files, args in ((["reads_se.fq"], ["-d", "-c"]), (["reads_pe_1.fq", "reads_pe_2.fq"], ["-d", "-c", "-p", "-a", "350", "-b", "650"])):
            fqs = []
            for f in files:
                lines = _fq(f).split(b"\n")
                for i in range(0, len(lines) - 3, 4):
                    if (i // 4) % 3 == 0:
                        lines[i] = b"@" + (b"n%d_" % (i // 4)).ljust(1 + (i // 4) % 254, b"y") + b" a comment"       # names of 1 .. 254 bytes
                fqs.append(b"\n".join(lines))
            sam, bam = _both(ix, args, fqs)
            _same_as_the_host_encoder(ix, sam, bam)
            recs = bam_check.records(bam, 0, refs)
            assert max(len(r["name"]) for r in recs) == 254
            tails = [len(r["bytes"]) - (36 + len(r["name"]) + 1 + 4 * len(r["cigar"]) + (r["l_seq"] + 1) // 2 + r["l_seq"]) for r in recs]
            assert sum(1 for t in tails if t > 224) > 3, "no record's tags outgrew the slot: the single-lane path was not tested"
    finally:
        ix.destroy()


def test_a_name_of_255_bytes_is_refused_by_the_device_path(lambda_index):
    import salt_amd
    lines = _fq("reads_se.fq").split(b"\n")
    lines[4 * 321] = b"@" + b"q" * 255
    aln = salt_amd.GpuAligner(lambda_index, device=0, max_reads=4096)
    try:
        aln.set_contigs(lambda_index)
        opt = _opt(lambda_index, ["-d", "-c"])
        sam, n = aln.align_se_text(opt, b"\n".join(lines))            # SAM has no such limit
        assert n == 2000 and b"q" * 255 + b"\t" in sam
        aln.set_sam_bam(True)
        with pytest.raises(salt_amd.SaltError, match="BAM: a read name in this block is longer than 254 bytes"):
            aln.align_se_text(opt, b"\n".join(lines))
        lines[4 * 321] = b"@" + b"q" * 254
        assert aln.align_se_text(opt, b"\n".join(lines))[1] == 2000
    finally:
        aln.close()


@pytest.fixture(scope="module")
def lambda_cli_index(tmp_path_factory):
    """The lambda fixture indexed by salt-idx (the committed index lacks the 64 MiB .C.lkt)."""
    prefix = str(tmp_path_factory.mktemp("lamidx") / "idx")
    subprocess.run([SALT_IDX, "-k", "19", os.path.join(LAMBDA, "genome.fa"), os.path.join(LAMBDA, "snps.txt"), prefix], check=True, stderr=subprocess.DEVNULL,
                   timeout=600)
    return prefix


def _run(cmd, env, rc=0):
    out = subprocess.run(cmd, capture_output=True, env=env, timeout=600)
    assert out.returncode == rc, out.stderr[-600:]
    return out


def _decodes_to(out, want):
    text, lines, recs = bam_check.decode_stream(out.stdout)
    assert strip_pg(text) == bam_check.sam_header(want) and lines == bam_check.sam_records(want)
    return recs


@pytest.mark.parametrize("case", ["se_default", "se_r1_m500", "pe_default", "pe_r5", "ragged_pe"])
def test_cli_bam_on_the_device_and_with_the_host_encoder(case, lambda_cli_index):
    args, files = EXTRA_CASES[case] if case in EXTRA_CASES else (read_cases()[case], ["reads_pe_1.fq", "reads_pe_2.fq"] if case.startswith("pe") else ["reads_se.fq"])
    cmd = [SALT] + args + ["--bam", lambda_cli_index] + [os.path.join(LAMBDA, f) for f in files]
    want = _golden(case)
    for env in (dict(os.environ, SALT_CHUNK_BYTES="3000"), dict(os.environ)):
        dev = _run(cmd, env)
        assert b"text path" in dev.stderr and b"[salt] BAM output: device records, " in dev.stderr and b"BGZF output: device deflate" in dev.stderr, dev.stderr[-600:]
        _decodes_to(dev, want)
        host = _run(cmd, dict(env, SALT_BAM_HOST="1"))
        assert b"[salt] BAM output: host records, " in host.stderr, host.stderr[-600:]
        _decodes_to(host, want)
        zhost = _run(cmd, dict(env, SALT_BGZF_HOST="1"))           # the device's records through zlib
        assert b"[salt] BAM output: device records, " in zhost.stderr and b"BGZF output: host deflate" in zhost.stderr
        _decodes_to(zhost, want)
    assert _run(cmd, dict(os.environ)).stdout == dev.stdout, "two device runs gave different files"


def test_cli_long_name_error_comes_from_the_device_path(lambda_cli_index, tmp_path):
    lines = _fq("reads_se.fq").split(b"\n")
    lines[4 * 900] = b"@" + b"q" * 255 + b" c"
    fq = tmp_path / "long.fq"
    fq.write_bytes(b"\n".join(lines))
    out = _run([SALT, "-d", "-c", "--bam", lambda_cli_index, str(fq)], dict(os.environ, SALT_CHUNK_BYTES="9000"), rc=1)
    assert b"BAM: a read name in this block is longer than 254 bytes" in out.stderr and b"the host parser takes over" not in out.stderr
    assert out.stdout[-28:] != EOF and b"BAM output:" not in out.stderr


def test_cli_without_the_option_nothing_changes(lambda_cli_index):
    out = _run([SALT] + read_cases()["se_default"] + [lambda_cli_index, os.path.join(LAMBDA, "reads_se.fq")], dict(os.environ, SALT_CHUNK_BYTES="3001"))
    assert strip_pg(out.stdout) == _golden("se_default") and b"BAM" not in out.stderr


def test_grch38_scale_cli_bam_equals_the_plain_run(tmp_path_factory):
    """Like test_config3_cli_fastq_to_sam_equals_the_oracle_cli: 300 000 reads on the GRCh38-scale index, 8-MiB chunks, several workers; the
    decoded BAM equals the plain run's SAM, record for record."""
    import torch
    from salt_amd import workload
    tmp = tmp_path_factory.mktemp("grch38bam")
    dev = torch.device("cuda", 0)
    g, p, m = workload.generate_device("grch38", dev)
    w = workload.prepare("grch38", str(tmp), gpu_device=0, arrays=(g, p, m))
    try:
        n = 300_000
        seqs, _, _, _ = workload.make_reads_hash(g, workload.make_site_map(g.numel(), p, m), n, 100, seed=9, batch=0)
        fq = str(tmp / "reads.fq")
        with open(fq, "wb") as f:
            f.write(workload.fastq_bytes(seqs.cpu().numpy(), n, 100))
        del g, p, m, seqs
        torch.cuda.empty_cache()
        env = dict(os.environ, SALT_CHUNK_MB="8")
        plain = subprocess.run([SALT, "-d", "-c", "-t", "32", w["prefix"], fq], capture_output=True, env=env, timeout=900)
        assert plain.returncode == 0 and b"text path" in plain.stderr, plain.stderr[-400:]
        bam = subprocess.run([SALT, "-d", "-c", "-t", "32", "--bam", w["prefix"], fq], capture_output=True, env=env, timeout=900)
        assert bam.returncode == 0 and b"BAM output: device records" in bam.stderr, bam.stderr[-400:]
        text, lines, recs = bam_check.decode_stream(bam.stdout)
        assert strip_pg(text) == strip_pg(bam_check.sam_header(plain.stdout))
        assert len(recs) == n and lines == bam_check.sam_records(plain.stdout)
    finally:
        for f in os.listdir(w["dir"]):
            os.unlink(os.path.join(w["dir"], f))
