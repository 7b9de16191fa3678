"""`salt-idx --vcf` without a GPU: the host twin of the device's VCF parser (salt_vcf_snps) against the Python statement of the rule
(vcf_check.model), and the tool itself on VCFs built from the committed genome.fa / snps.txt pairs -- the index it writes is
the one the real reference wrote from the SNP file, and the sites go to their contigs by NAME."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_check
import vcf_check as vc
from conftest import LAMBDA, ROOT
from vcf_check import SALT_IDX, SEED_LEN, same_dirs, same_index
EDGES = vc.edge_texts()


@pytest.fixture(scope="module")
def built():
    """case -> (contigs, snps, VCF text), built once"""
    out = {}
    for k, case in enumerate(sorted(vc.FIXTURES)):
        contigs, snps = vc.fixture(case)
        out[case] = (contigs, snps, vc.build_vcf(contigs, snps, seed=k + 1))
    return out


def host(contigs, text, **kw):
    import salt_amd
    return salt_amd.vcf_snps(vc.api_contigs(contigs), text, **kw)


def salt_idx(*args, ok=True):
    p = subprocess.run([SALT_IDX, "-k", str(SEED_LEN)] + [str(a) for a in args], capture_output=True, text=True)
    assert (p.returncode == 0) == ok, p.stderr
    return p.stderr


def counters_of(stderr):
    line = [l for l in stderr.splitlines() if " lines=" in l][0]
    return {k: int(v) for k, v in (kv.split("=") for kv in line.split(": ", 1)[1].split())}


# ---- 1. the host twin equals the Python model ----

@pytest.mark.parametrize("case", sorted(vc.FIXTURES))
@pytest.mark.parametrize("pass_only", [False, True])
def test_twin_equals_model_on_fixtures(built, case, pass_only):
    contigs, snps, text = built[case]
    want = vc.model(contigs, text, pass_only=pass_only)
    assert vc.same(host(contigs, text, pass_only=pass_only), want)
    if not pass_only:                                   # the noise loses nothing: the sites are the SNP file's, by name
        assert vc.same((want[0], {}), (vc.snp_groups(contigs, snps), {}))
        assert want[1]["sites"] == len(snps) and min(want[1][k] for k in ("unknown_contig", "not_snv")) > 0
    else:
        assert want[1]["filtered"] > 0


def test_pass_only_drops_sites_that_only_filtered_records_hold(built):
    contigs, snps, _ = built["dense"]
    text = vc.build_vcf(contigs, snps, seed=9, extra_filtered=True)
    every, passing = vc.model(contigs, text), vc.model(contigs, text, pass_only=True)
    assert every[1]["sites"] > passing[1]["sites"] > 0
    assert vc.same(host(contigs, text), every) and vc.same(host(contigs, text, pass_only=True), passing)


@pytest.mark.parametrize("name", sorted(EDGES))
@pytest.mark.parametrize("pass_only", [False, True])
def test_twin_equals_model_on_edges(name, pass_only):
    import salt_amd
    text, bad = EDGES[name]
    if bad is None:
        assert vc.same(host(vc.EDGE_CONTIGS, text, pass_only=pass_only), vc.model(vc.EDGE_CONTIGS, text, pass_only=pass_only))
    else:
        with pytest.raises(vc.Malformed) as m:
            vc.model(vc.EDGE_CONTIGS, text)
        assert m.value.line == bad
        with pytest.raises(salt_amd.SaltError, match=r"VCF line %d is malformed" % bad):
            host(vc.EDGE_CONTIGS, text, pass_only=pass_only)


def test_edges_say_what_the_rule_says():
    """the model itself, pinned on the cases where a wrong rule would still agree with a wrong twin"""
    m = lambda n, **kw: vc.model(vc.EDGE_CONTIGS, EDGES[n][0], **kw)
    g, c = m("pos_wraps_to_1")
    assert c["out_of_range"] == 1 and c["sites"] == 0                   # 2^32 + 1 is never site 1
    assert m("pos_1")[0][0][1].tolist() == [0] and m("pos_len")[0][0][1].tolist() == [20] and m("pos_len_plus_1")[1]["out_of_range"] == 1
    assert m("pos_0")[1]["out_of_range"] == 1 and m("pos_ten_digits")[1]["out_of_range"] == 1
    assert m("ref_disagrees")[1]["ref_mismatch"] == 1 and m("site_on_N")[1] == dict(m("site_on_N")[1], ref_mismatch=1, not_snv=1, sites=0)
    g, c = m("contig_borders")
    assert [x[1].tolist() for x in g] == [[20], [0, 13], [0]] and g[1][2].tolist() == [4 | 2, 15] and c["kept"] == 4
    g, c = m("prefix_names")
    assert c["unknown_contig"] == 2 and c["first_unknown_line"] == 3 and [len(x[1]) for x in g] == [1, 1, 0]
    assert m("or_of_lines")[0][0][2].tolist() == [2 | 8 | 4 | 1]
    assert m("empty")[1]["lines"] == 0 and m("header_only")[1]["lines"] == 0 and m("newlines_only")[1]["lines"] == 0
    assert m("filters", pass_only=True)[1] == dict(m("filters")[1], kept=4, filtered=3, sites=4)


def test_rename_map_in_memory():
    text = b"1\t2\t.\tC\tT\nab\t2\t.\tA\tC\na\t3\t.\tG\tT\nx\t1\t.\tC\tA\n"
    for rename in ({"1": "a", "x": "b"}, {"1": "a", "a": "nowhere"}, [("1", "b"), ("1", "a")], {"a": "ab", "ab": "a"}):
        assert vc.same(host(vc.EDGE_CONTIGS, text, rename=rename), vc.model(vc.EDGE_CONTIGS, text, rename=rename))


# ---- 2. the tool on the built VCFs: the reference's own index files ----

@pytest.mark.parametrize("case", ["two_contigs", "all_snp_contigs", "dense", "lambda"])
def test_tool_writes_the_reference_index_from_a_vcf(built, case, tmp_path):
    contigs, snps, text = built[case]
    (tmp_path / "in.vcf").write_bytes(text)
    err = salt_idx("--vcf", os.path.join(vc.FIXTURES[case], "genome.fa"), tmp_path / "in.vcf", tmp_path / "idx")
    want = vc.model(contigs, text)[1]
    assert counters_of(err) == {k: want[k] for k in vc.COUNTERS}
    assert "first unknown contig" in err and "at line %d" % want["first_unknown_line"] in err
    same_index(str(tmp_path / "idx"), vc.FIXTURES[case], sa_slack=0 if case == "lambda" else 1)


# ---- 3. by name, not by order ----

def test_gap_short_sites_land_on_their_contigs_by_name(built, tmp_path):
    import salt_amd
    contigs, snps, text = built["gap_short"]
    assert [c for c, _, _, _ in snps] == ["a", "c"] and [n for n, _ in contigs] == ["a", "b", "c"]
    fa = os.path.join(vc.FIXTURES["gap_short"], "genome.fa")
    (tmp_path / "in.vcf").write_bytes(text)
    salt_idx("--vcf", fa, tmp_path / "in.vcf", tmp_path / "idx")
    start = np.cumsum([0] + [len(s) for _, s in contigs])
    want = sorted(int(start[[n for n, _ in contigs].index(c)]) + p - 1 for c, p, _, _ in snps)
    ix = salt_amd.Index.reload(str(tmp_path / "idx"))
    assert salt_amd.snp_sites(ix).tolist() == want and start[2] <= want[1]
    ix.destroy()
    ref = np.fromfile(str(tmp_path / "idx.ref"), dtype=np.uint32)[1:]
    nib = lambda p: int(ref[p >> 3] >> (4 * (p & 7))) & 15
    for c, p, al, _ in snps:
        assert nib(int(start[[n for n, _ in contigs].index(c)]) + p - 1) == sum(vc.BIT[ord(a)] for a in al.split("/"))
    assert all(bin(nib(p)).count("1") == 1 for p in range(int(start[1]), int(start[2])))        # nothing on b
    # the file path lays the second group over b (the reference's by-order rule, which the golden files pin): the two differ
    by_order = np.fromfile(os.path.join(vc.FIXTURES["gap_short"], "idx.ref"), dtype=np.uint32)[1:]
    assert (by_order != ref).any()
    # the records of c in front of those of a: the same directory
    (tmp_path / "ca.vcf").write_bytes(vc.build_vcf(contigs, snps, seed=3, contig_order=["c", "a"]))
    salt_idx("--vcf", fa, tmp_path / "ca.vcf", tmp_path / "ca")
    same_dirs(str(tmp_path / "idx"), str(tmp_path / "ca"))


def test_memory_path_keeps_the_place_of_a_contig_without_sites(built, tmp_path):
    """vcf_snps composes with idx_build_mem: an empty group in the middle shifts nothing, and the files are the tool's"""
    import salt_amd
    contigs, snps, text = built["gap_short"]
    groups, _ = host(contigs, text)
    assert [len(g[1]) for g in groups] == [1, 0, 1]
    salt_amd.idx_build_mem(vc.api_contigs(contigs), groups, str(tmp_path / "mem"), SEED_LEN)
    (tmp_path / "in.vcf").write_bytes(text)
    salt_idx("--vcf", os.path.join(vc.FIXTURES["gap_short"], "genome.fa"), tmp_path / "in.vcf", tmp_path / "idx")
    for sfx in (".C.bwt", ".C.sa", ".lp", ".R.backward.bwt", ".R.backward.occ", ".R.backward.sa", ".ref"):
        assert open(str(tmp_path / "mem") + sfx, "rb").read() == open(str(tmp_path / "idx") + sfx, "rb").read(), sfx
    # the local pattern of c's site carries c's own offset: the header value is site + seed length - 1 in genome coordinates
    start = np.cumsum([0] + [len(s) for _, s in contigs])
    hdrs = [int(l.split("\t")[1]) for l in open(str(tmp_path / "idx.lp")).read().splitlines() if l.startswith(">")]
    assert hdrs == [int(start[i]) + int(g[1][0]) + SEED_LEN - 1 for i, g in enumerate(groups) if len(g[1])]


# ---- 4. --snp-out ----

def test_snp_out_reproduces_the_snp_file(built, tmp_path):
    contigs, snps, text = built["lambda"]
    fa = os.path.join(LAMBDA, "genome.fa")
    (tmp_path / "in.vcf").write_bytes(text)
    salt_idx("--vcf", "--snp-out", tmp_path / "out.txt", fa, tmp_path / "in.vcf", tmp_path / "idx")
    assert (tmp_path / "out.txt").read_bytes() == open(os.path.join(LAMBDA, "snps.txt"), "rb").read()
    salt_idx(fa, tmp_path / "out.txt", tmp_path / "plain")
    same_dirs(str(tmp_path / "idx"), str(tmp_path / "plain"))


# ---- 5. the rename map ----

def test_rename_map(built, tmp_path):
    contigs, snps, _ = built["two_contigs"]
    fa = os.path.join(vc.FIXTURES["two_contigs"], "genome.fa")
    text = vc.build_vcf(contigs, snps, seed=5, vcf_names={"a": "1", "c": "2"})
    (tmp_path / "in.vcf").write_bytes(text)
    err = salt_idx("--vcf", fa, tmp_path / "in.vcf", tmp_path / "none", ok=False)
    assert counters_of(err)["sites"] == 0 and counters_of(err)["unknown_contig"] == vc.model(contigs, text)[1]["unknown_contig"]
    assert "no local pattern was generated" in err and 'first unknown contig "' in err
    (tmp_path / "map.tsv").write_text("1\ta\n2\tc\n")
    err = salt_idx("--vcf", "--vcf-contigs", tmp_path / "map.tsv", fa, tmp_path / "in.vcf", tmp_path / "idx")
    assert counters_of(err)["sites"] == len(snps)
    same_index(str(tmp_path / "idx"), vc.FIXTURES["two_contigs"])


def test_options_without_vcf_are_refused_and_pass_only_counts(built, tmp_path):
    contigs, snps, _ = built["dense"]
    fa = os.path.join(vc.FIXTURES["dense"], "genome.fa")
    assert "go with --vcf" in salt_idx("--vcf-pass-only", fa, os.path.join(vc.FIXTURES["dense"], "snps.txt"), tmp_path / "x", ok=False)
    text = vc.build_vcf(contigs, snps, seed=9, extra_filtered=True)
    (tmp_path / "in.vcf").write_bytes(text)
    err = salt_idx("--vcf", "--vcf-pass-only", "--snp-out", tmp_path / "out.txt", fa, tmp_path / "in.vcf", tmp_path / "idx")
    want = vc.model(contigs, text, pass_only=True)
    assert counters_of(err) == {k: want[1][k] for k in vc.COUNTERS}
    assert len((tmp_path / "out.txt").read_text().splitlines()) == want[1]["sites"]


def test_malformed_line_is_named_by_the_tool(tmp_path):
    (tmp_path / "g.fa").write_text("".join(">%s\n%s\n" % (n, s.decode()) for n, s in vc.EDGE_CONTIGS))
    (tmp_path / "in.vcf").write_bytes(EDGES["pos_eleven_digits_and_12a"][0])
    assert "VCF line 3 is malformed" in salt_idx("--vcf", tmp_path / "g.fa", tmp_path / "in.vcf", tmp_path / "idx", ok=False)


# ---- 6. compressed input ----

def test_gzip_and_bgzf_input(built, tmp_path):
    contigs, snps, text = built["dense"]
    fa = os.path.join(vc.FIXTURES["dense"], "genome.fa")
    blocks = vc.bgzf(text)
    assert bgzf_check.stream_text(blocks) == text and len(bgzf_check.members(blocks)) > 3
    (tmp_path / "plain.vcf").write_bytes(text)
    (tmp_path / "one.vcf.gz").write_bytes(gzip.compress(text))
    (tmp_path / "blocks.vcf.gz").write_bytes(blocks)
    errs = [salt_idx("--vcf", fa, tmp_path / f, tmp_path / f.split(".")[0]) for f in ("plain.vcf", "one.vcf.gz", "blocks.vcf.gz")]
    assert counters_of(errs[0]) == counters_of(errs[1]) == counters_of(errs[2]) and counters_of(errs[0])["sites"] == len(snps)
    same_dirs(str(tmp_path / "plain"), str(tmp_path / "one"))
    same_dirs(str(tmp_path / "plain"), str(tmp_path / "blocks"))
    same_index(str(tmp_path / "blocks"), vc.FIXTURES["dense"])


def test_python_file_path(built, tmp_path):
    import salt_amd
    contigs, snps, text = built["two_contigs"]
    (tmp_path / "in.vcf.gz").write_bytes(gzip.compress(text))
    ct = salt_amd.idx_build(os.path.join(vc.FIXTURES["two_contigs"], "genome.fa"), str(tmp_path / "in.vcf.gz"), str(tmp_path / "idx"), SEED_LEN, vcf=True,
                            vcf_opts={"snp_out": str(tmp_path / "out.txt")})
    assert ct == vc.model(contigs, text)[1]
    same_index(str(tmp_path / "idx"), vc.FIXTURES["two_contigs"])
    assert (tmp_path / "out.txt").read_bytes() == open(os.path.join(vc.FIXTURES["two_contigs"], "snps.txt"), "rb").read()


# ---- 7. the twin as a program under AddressSanitizer + UBSan ----

@pytest.fixture(scope="module")
def vcf_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("vcfmodel")
    exe = str(d / "vcf_model.san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-o", exe, os.path.join(ROOT, "tools", "vcf_model.cc"), os.path.join(ROOT, "salt_amd", "host", "salt_idx.cc"), "-lz", "-lpthread"], check=True)
    (d / "g.fa").write_text("".join(">%s\n%s\n" % (n, s.decode()) for n, s in vc.EDGE_CONTIGS))
    return exe, d


def test_twin_under_sanitizers_on_the_edge_texts(vcf_model, built):
    exe, d = vcf_model

    def run(fa, text, pass_only, contigs):
        (d / "in.vcf").write_bytes(text)
        p = subprocess.run([exe] + (["--pass-only"] if pass_only else []) + [str(fa), str(d / "in.vcf")], capture_output=True, text=True)
        assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
        try:
            groups, ct = vc.model(contigs, text, pass_only=pass_only)
        except vc.Malformed as m:
            assert p.returncode == 3 and "VCF line %d is malformed" % m.line in p.stderr
            return
        assert p.returncode == 0, p.stderr
        want = ["%s\t%d\t%d\t%d" % (n, a, b, c) for n, pos, al, rf in groups for a, b, c in zip(pos.tolist(), al.tolist(), rf.tolist())]
        want.append(" ".join("%s=%d" % (k, ct[k]) for k in vc.COUNTERS + ("first_unknown_line",)))
        assert p.stdout.splitlines() == want

    for name in sorted(EDGES):
        for pass_only in (False, True):
            run(d / "g.fa", EDGES[name][0], pass_only, vc.EDGE_CONTIGS)
    # texts that end inside every field of a line: nothing is read behind the text's last byte
    line = b"a\t2\trs\tC\tT,G\t9\tq10\tX=1"
    for cut in range(len(line) + 1):
        run(d / "g.fa", b"a\t3\t.\tG\tA\n" + line[:cut], True, vc.EDGE_CONTIGS)
    contigs, snps, text = built["gap_short"]
    run(os.path.join(vc.FIXTURES["gap_short"], "genome.fa"), text, False, contigs)
