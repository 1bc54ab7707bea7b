"""Batched proving through the C++ adapter (include/ringsnark_amd/batch.hpp: groth16::prove_batch, rinocchio::prove_batch on a
proving_key_device and on a seeded_proving_key): tests/cpp/batch_run.cpp compiled with plain g++ and linked against
librs_hip.so (CPU), and run on the device (-m gpu): prove_batch of three statements on a generated key and on a seeded key,
every proof equal to prover of that member and accepted by verifier with that member's primary input only."""
import os
import shutil
import subprocess

import pytest

from ringsnark_amd import params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batch_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("batch_run") / "batch_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "batch_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_batch_adapter_compiles_and_links(batch_run_exe):
    """prove_batch on both key types of both schemes, and the library's _batch entry points"""
    assert os.path.exists(batch_run_exe)


@pytest.mark.gpu
def test_batch_adapter_proofs_equal_the_single_prover_and_verify(batch_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([batch_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "batch_run: OK" in r.stdout, r.stdout + r.stderr
