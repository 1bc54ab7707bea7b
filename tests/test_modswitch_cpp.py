"""ringsnark::amd::mod_switch and the verifier overloads on switched proofs (include/ringsnark_amd/modswitch.hpp), the C++
adapters of ringsnark_amd/modswitch.h: tests/cpp/modswitch_run.cpp compiled with plain g++ against the header and linked
against librs_hip.so (CPU), and run on the device (-m gpu): per scheme a proof is generated, proved, switched to K - 1
primes, accepted, and rejected for a changed primary input."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def modswitch_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("modswitch_run") / "modswitch_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "modswitch_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_modswitch_adapter_compiles_and_links(modswitch_run_exe):
    """the switched types, mod_switch for both schemes and the verifier overloads exist, and the library has the entry points"""
    assert os.path.exists(modswitch_run_exe)


@pytest.mark.gpu
def test_modswitch_adapter_runs_against_the_library(modswitch_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([modswitch_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "modswitch_run: OK" in r.stdout, r.stdout + r.stderr
