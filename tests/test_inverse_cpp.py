"""ringsnark::amd::inv_or_zero (include/ringsnark_amd/inverse.hpp), the C++ adapter of the device inverse-or-zero:
tests/cpp/inverse_run.cpp compiled with plain g++ against the headers and linked against librs_hip.so (CPU), and run on the
device (-m gpu): the is-zero assignment of three elements with planted zeros, its inv rows made on the device inside the
assignment, checked with the adapter's own ring operations."""
import os
import re
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def inverse_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("inverse_run") / "inverse_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "inverse_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_inverse_adapter_compiles_and_links(inverse_run_exe):
    """inv_or_zero exists in its three forms, no reference header is needed, and the library has the entry point."""
    assert os.path.exists(inverse_run_exe)
    src = open(os.path.join(ROOT, "tests", "cpp", "inverse_run.cpp")).read()
    assert "libsnark" not in src and "<ringsnark/" not in src


@pytest.mark.gpu
def test_inverse_adapter_runs_against_the_library(inverse_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([inverse_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = re.search(r"^inverse_run: OK blocks=(\d+) n_zero=(\d+) first=(\d+)/(\d+)/(\d+)$", r.stdout, flags=re.M)
    assert line, r.stdout + r.stderr
    blocks, n_zero, elem, limb, slot = (int(g) for g in line.groups())
    # what the program plants: block 0 every third word of the limbs after the first, block 1 every fourth word, block 2
    # every fifth (a random word that is zero by itself: 3 * 64 draws below 2^30)
    rw = prm.ring_words
    planted = len([i for i in range(prm.N, rw) if i % 3 == 0]) + len(range(0, rw, 4)) + len(range(0, rw, 5))
    first = next(i for i in range(prm.N, rw) if i % 3 == 0)
    assert blocks == 3 and n_zero >= planted and n_zero - planted <= 1
    assert (elem, limb, slot) == (0, first // prm.N, first % prm.N)
