"""ringsnark::amd::groth16::verify_batch / ringsnark::amd::rinocchio::verify_batch (include/ringsnark_amd/verify_batch.hpp),
the C++ adapters of batched verification: tests/cpp/verify_batch_run.cpp compiled with plain g++ against the header and
linked against librs_hip.so (CPU), and run on the device (-m gpu): three proofs and a tampered member per scheme, every
verdict the single verifier's."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def verify_batch_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("verify_batch_run") / "verify_batch_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "verify_batch_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_verify_batch_adapter_compiles_and_links(verify_batch_run_exe):
    """verify_batch exists for both schemes, on proofs and on switched proofs, and the library has the entry points"""
    assert os.path.exists(verify_batch_run_exe)


@pytest.mark.gpu
def test_verify_batch_adapter_runs_against_the_library(verify_batch_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([verify_batch_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "verify_batch_run: OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("accepted") == 5 and r.stdout.count("rejected") == 3
