"""Packed keys through the C++ adapters (include/ringsnark_amd/packed.hpp: generator(cs, packed), prover and prove_batch on a
packed_proving_key): tests/cpp/packed_run.cpp compiled with plain g++ and linked against librs_hip.so (CPU), and run on the
device (-m gpu): generator(packed) -> prover -> verifier per scheme, and the proofs equal, word for word, to the seeded
prover's on the seeded key of the same seeds."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def packed_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("packed_run") / "packed_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "packed_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_packed_adapter_compiles_and_links(packed_run_exe):
    """generator(cs, packed), prover and prove_batch on a packed_proving_key, and the library's _packed entry points"""
    assert os.path.exists(packed_run_exe)


@pytest.mark.gpu
def test_packed_adapter_runs(packed_run_exe):
    """toy, as tests/test_seeded_cpp.py: 41-bit rows with a pad word; the program's Rinocchio proofs with sampled ZK elements
    need a noise budget that the wider toy presets do not leave (tests/test_verify.py)"""
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([packed_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "packed_run: OK" in r.stdout, r.stdout + r.stderr
