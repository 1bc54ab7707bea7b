"""ringsnark::amd::is_satisfied (include/ringsnark_amd/r1cs_check.hpp), the C++ adapter of the device satisfaction check:
tests/cpp/check_run.cpp compiled with plain g++ against the header and linked against librs_hip.so (CPU), and run on the
device (-m gpu)."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("check_run") / "check_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "check_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_check_adapter_compiles_and_links(check_run_exe):
    """is_satisfied / r1cs_violation exist with the reference's argument order, and the library has the entry point."""
    assert os.path.exists(check_run_exe)


@pytest.mark.gpu
def test_check_adapter_runs_against_the_library(check_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([check_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "check_run: OK" in r.stdout, r.stdout + r.stderr
