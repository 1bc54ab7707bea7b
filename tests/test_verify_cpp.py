"""ringsnark::amd::groth16::verifier / ringsnark::amd::rinocchio::verifier (include/ringsnark_amd/verify.hpp), the C++
adapters of the device verifiers: tests/cpp/verify_run.cpp compiled with plain g++ against the header and linked against
librs_hip.so (CPU), and run on the device (-m gpu): one accepted and one rejected proof per scheme."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verify_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("verify_run") / "verify_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "verify_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_verify_adapter_compiles_and_links(verify_run_exe):
    """the two verifiers and their key structs exist with the reference's argument order, and the library has the entry points"""
    assert os.path.exists(verify_run_exe)


@pytest.mark.gpu
def test_verify_adapter_runs_against_the_library(verify_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([verify_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "verify_run: OK" in r.stdout, r.stdout + r.stderr
