"""ringsnark::amd::bit_decompose (include/ringsnark_amd/bits.hpp), the C++ adapter of the device bit decomposition:
tests/cpp/bits_run.cpp compiled with plain g++ against the headers and linked against librs_hip.so (CPU), and run on the
device (-m gpu): the range check without constants, its bits made on the device inside the assignment, through
is_satisfied and the Rinocchio generator, prover and verifier."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bits_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("bits_run") / "bits_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "bits_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_bits_adapter_compiles_and_links(bits_run_exe):
    """bit_decompose exists in both forms, no reference header is needed, and the library has the entry point."""
    assert os.path.exists(bits_run_exe)
    src = open(os.path.join(ROOT, "tests", "cpp", "bits_run.cpp")).read()
    assert "libsnark" not in src and "<ringsnark/" not in src


@pytest.mark.gpu
def test_bits_adapter_runs_against_the_library(bits_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([bits_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bits_run: OK" in r.stdout, r.stdout + r.stderr
