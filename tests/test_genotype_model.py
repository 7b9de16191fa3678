"""The genotype calls without a GPU: the penalty table against its formula; the host twin (salt_gt_add_sam, salt_gt_text, salt_gt_header)
against the Python statement (tests/gt_check.py) on the lambda goldens; a hand-made sums table that holds every case of the call rule
through salt_gt_text; and tools/genotype_model.cc, the twin and its printer as a program of its own under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

import gt_check
import snp_check
from conftest import LAMBDA, ROOT

SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


@pytest.fixture(scope="module")
def lam():
    import salt_amd
    ix = salt_amd.Index.reload(os.path.join(LAMBDA, "idx"))
    yield salt_amd, ix, gt_check.Genome()
    ix.destroy()


def test_the_table_in_the_header_is_the_formula():
    import salt_amd
    got = salt_amd.gt_table()
    assert got.shape == (94, 3) and got.dtype == np.uint32 and np.array_equal(got, np.array(gt_check.TABLE, dtype=np.uint32))
    for q, row in ((0, (17733, 27735, 22040)), (2, (17733, 27735, 22040)), (20, (179, 101463, 12449)), (30, (18, 142423, 12342)), (40, (2, 183383, 12331)),
                   (60, (0, 265303, 12330)), (93, (0, 265303, 12330))):
        assert tuple(int(x) for x in got[q]) == row
    assert gt_check.tie_margin() > 0.0047                            # no entry near a rounding tie: the libm in use does not matter
    assert salt_amd.GT_Q_NONE == gt_check.Q_NONE == 20
    # the header holds the numbers once, as literals, and both libraries' sources take them from there
    text = open(os.path.join(ROOT, "include", "salt_gt_table.h")).read()
    rows = re.findall(r"\{ (\d+), (\d+), (\d+) \}", text)
    assert [[int(x) for x in r] for r in rows] == gt_check.TABLE
    for src in ("salt_amd/csrc/salt_gt.hip", "salt_amd/host/salt_host.cc"):
        code = open(os.path.join(ROOT, src)).read()
        assert "salt_gt_table.h" in code and "log10(" not in code.split("Genotypes at the SNP sites")[-1] and "101463" not in code


@pytest.mark.parametrize("min_mapq", [0, 20, 255])
@pytest.mark.parametrize("name", sorted(snp_check.GOLDENS))
def test_the_twins_sums_and_text_equal_the_python_statement(name, min_mapq, lam):
    salt_amd, ix, genome = lam
    sam = snp_check.golden_sam(name)
    want, n_want = gt_check.add_sam(genome, sam, min_mapq)
    got, n = salt_amd.gt_add_sam(ix, sam, min_mapq)
    assert n == n_want == (0 if min_mapq == 255 else snp_check.GOLDENS[name][0 if min_mapq == 0 else 1])
    assert np.array_equal(got, gt_check.as_array(want)) and got[:, :, 0].any() == (min_mapq != 255)
    counts, _ = snp_check.count_sam(genome.sites, genome.offsets, sam, min_mapq)
    assert np.array_equal(got[:, :, 0], counts.astype(np.uint64))    # n is the SNP counts' table
    assert salt_amd.gt_text(ix, got) == gt_check.text(genome, want)
    assert salt_amd.gt_text(ix, got[1000:1100], first=1000) == gt_check.text(genome, want[1000:1100], first=1000)
    again, _ = salt_amd.gt_add_sam(ix, sam, min_mapq, sums=got.copy())
    assert np.array_equal(again, 2 * got)


def test_qual_star_and_bytes_outside_the_range_count_at_q_none(lam):
    salt_amd, ix, genome = lam
    sam = snp_check.golden_sam("expect_se_default.sam")
    star = b"\n".join(b"\t".join(f[:10] + [b"*"] + f[11:]) if len(f) > 10 else b"\t".join(f) for f in (l.split(b"\t") for l in sam.split(b"\n")))
    odd = b"\n".join(b"\t".join(f[:10] + [b"\x7f" * len(f[10])] + f[11:]) if len(f) > 10 else b"\t".join(f) for f in (l.split(b"\t") for l in sam.split(b"\n")))
    for text in (star, odd):
        got, _ = salt_amd.gt_add_sam(ix, text, 0)
        want, _ = gt_check.add_sam(genome, text, 0)
        assert np.array_equal(got, gt_check.as_array(want)) and got[:, :, 0].sum() == 7574
        for k in range(3):
            assert np.array_equal(got[:, :, 1 + k], got[:, :, 0] * np.uint64(gt_check.TABLE[20][k]))
    assert salt_amd.gt_header(ix) == gt_check.header(genome) and salt_amd.gt_header(ix, "NA12878") == gt_check.header(genome, "NA12878")
    with pytest.raises(salt_amd.SaltError, match="sample name"):
        salt_amd.gt_header(ix, "a\tb")


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    import salt_amd
    prefix = gt_check.synth_index(tmp_path_factory.mktemp("gtsynth"))
    ix = salt_amd.Index.reload(prefix)
    yield salt_amd, ix, gt_check.Genome(prefix)
    ix.destroy()


def test_a_hand_made_table_holds_every_case_of_the_call_rule_and_the_printer_follows_it(synth):
    salt_amd, ix, genome = synth
    sums, census = gt_check.hand_made(genome)
    want = gt_check.text(genome, sums)
    assert salt_amd.gt_text(ix, gt_check.as_array(sums)) == want
    lines = want.decode().split("\n")[:-1]
    assert len(lines) == len(genome.sites)

    def called(s):
        g = int(genome.sites[s])
        return gt_check.call(int(genome.masks[g]), int(genome.bases[g]), sums[s])

    # each case occurs
    for n_al, n_gt in ((2, 3), (3, 6), (4, 10)):                     # two-, three- and four-allele sites with depth
        hit = [s for s in census["by_alleles"][n_al] if called(s)["dp"] > 0]
        assert len(hit) >= 5 and all(len(called(s)["pl"]) == n_gt and len(lines[s].split("\t")[4].split(",")) == n_al - 1 for s in hit)
    c = called(census["tie"])                                        # a tie: the lowest VCF index wins
    assert c["raw"][0] == c["raw"][2] == min(c["raw"]) and c["gt"] == (0, 0) and c["gq"] == 0 and "\t0/0:3,3:6:0:0," in lines[census["tie"]]
    ties = [s for s in range(len(sums)) if called(s)["dp"] and called(s)["raw"].count(min(called(s)["raw"])) > 1]
    assert census["tie"] in ties
    for key, pl in (("d2047", 0), ("d2048", 1)):                     # raw differences of exactly 2047 and 2048
        c = called(census[key])
        assert c["raw"][2] - c["raw"][0] == 2047 + pl and c["k"] == 0 and c["pl"][2] == pl and lines[census[key]].endswith(",%d" % pl)
    assert [called(s)["pl"][1] for s in census["gq"]] == [98, 99, 100] and [called(s)["gq"] for s in census["gq"]] == [98, 99, 99]      # GQ below, at and above 99
    assert [lines[s].split("\t")[9].split(":")[3] for s in census["gq"]] == ["98", "99", "99"]
    c = called(census["zero"])                                       # DP == 0
    assert c["dp"] == 0 and lines[census["zero"]].split("\t")[5:] == [".", ".", "DP=0", "GT:AD:DP:GQ:PL", "./.:0,0:0:.:."]
    assert sum(1 for l in lines if "\t./.:" in l) > 10 and any("./.:0,0,0:0" in l for l in lines) and any("./.:0,0,0,0:0" in l for l in lines)
    c = called(census["outside"])                                    # bases outside the allele set: in DP, in no AD, errors under every genotype
    assert c["dp"] == 17 and sum(c["ad"]) == 12 and min(c["raw"]) > 0 and "DP=17\t" in lines[census["outside"]] and ":12,0:17:" in lines[census["outside"]]
    c = called(census["big"])                                        # sums above 2^32
    assert max(max(w) for w in sums[census["big"]]) > 1 << 32 and max(c["pl"]) > 1 << 20 and c["dp"] == 700000
    edge = census["edge"]                                            # site 0, the last site, both sides of the contig boundaries
    assert edge[0] == 0 and edge[-1] == len(sums) - 1 and len(edge) == 6 and all(called(s)["dp"] > 0 for s in edge)
    names = [lines[s].split("\t")[0] for s in edge]
    assert names == ["synth1", "synth1", "synth2", "synth2", "synth3", "synth3"]
    assert [int(lines[s].split("\t")[1]) for s in edge] == [1, 2000, 1, 2000, 1, 2000]
    # the text of a range is the range of the text
    assert salt_amd.gt_text(ix, gt_check.as_array(sums[100:164]), first=100) == "".join(l + "\n" for l in lines[100:164]).encode()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("gtmodel")
    exe = str(d / "genotype_model.san")
    host = os.path.join(ROOT, "salt_amd", "host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tools", "genotype_model.cc"), os.path.join(host, "salt_host.cc"), "-lz", "-lpthread"], check=True)
    return exe


def _fnv(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("min_mapq", [0, 20])
def test_the_twin_and_the_printer_over_the_goldens_under_sanitizers(min_mapq, model, lam):
    salt_amd, ix, genome = lam
    names = sorted(snp_check.GOLDENS)
    p = subprocess.run([model, os.path.join(LAMBDA, "idx"), str(min_mapq)] + [os.path.join(LAMBDA, n) for n in names], capture_output=True, env=SAN_ENV, timeout=300)
    for word in (b"runtime error", b"AddressSanitizer"):
        assert word not in p.stderr, p.stderr.decode()[-3000:]
    assert p.returncode == 0, (p.returncode, p.stderr[-600:])
    out = p.stdout.decode().split("\n")
    head = gt_check.header(genome, "NA12878")
    assert out[len(names)] == "sites 3858 header %d hfnv %d" % (len(head), _fnv(head))
    assert out[len(names) + 1].startswith("refused ") and int(out[len(names) + 1].split()[1]) >= 12
    for name, line in zip(names, out):
        want, n_rec = gt_check.add_sam(genome, snp_check.golden_sam(name), min_mapq)
        arr, text = gt_check.as_array(want), gt_check.text(genome, want)
        f = line.split(" ")
        got = dict(zip(f[1::2], map(int, f[2::2])))
        assert got == {"records": n_rec, "events": int(arr[:, :, 0].sum()), "fnv": _fnv(arr.tobytes()), "text": len(text), "tfnv": _fnv(text)}, name
