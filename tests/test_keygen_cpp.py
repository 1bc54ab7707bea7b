"""ringsnark::amd::groth16::generator / ringsnark::amd::rinocchio::generator (include/ringsnark_amd/keygen.hpp), the C++
adapters of the device generators: tests/cpp/keygen_run.cpp compiled with plain g++ against the header and linked against
librs_hip.so (CPU), and run on the device (-m gpu): generator -> prover -> verifier per scheme, a rejected proof, and two
generator calls with different trapdoors."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def keygen_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("keygen_run") / "keygen_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "keygen_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_keygen_adapter_compiles_and_links(keygen_run_exe):
    """the two generators return {generated_proving_key (a proving_key_device), verification_key}, and the library has the entry points"""
    assert os.path.exists(keygen_run_exe)


@pytest.mark.gpu
def test_keygen_adapter_runs_against_the_library(keygen_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([keygen_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "keygen_run: OK" in r.stdout, r.stdout + r.stderr
