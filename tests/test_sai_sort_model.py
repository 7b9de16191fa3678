"""The seed-interval sort (salt_amd/csrc/salt_sai_sort.h) on the host: tests/sai_sort_main.cpp runs the serial replica the
heavy kernels used before the header (arrays addressed by index), the header's template on the triples in place and the header's template on a key and an index per element (the form the
heavy kernels keep in lanes), and asks for the same order from all three, equal keys included.  Built with ASan + UBSan: a stand-alone
program, no GPU."""
import os
import subprocess

from conftest import ROOT

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=97", UBSAN_OPTIONS="halt_on_error=1:exitcode=98:print_stacktrace=1")


def test_lane_form_gives_klibs_permutation(tmp_path):
    exe = str(tmp_path / "sai_sort")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(ROOT, "tests", "sai_sort_main.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, env=ENV)
    assert p.returncode == 0, (p.stdout + p.stderr).decode()[-2000:]
    assert b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr, p.stderr.decode()[-2000:]
    assert b"all three forms agree" in p.stdout, p.stdout.decode()[-500:]
