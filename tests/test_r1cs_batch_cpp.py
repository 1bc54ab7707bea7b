"""ringsnark::amd::solve_batch / is_satisfied_batch (include/ringsnark_amd/r1cs_batch.hpp), the C++ adapter of the batched
assignment solver and satisfaction check: tests/cpp/r1cs_batch_run.cpp compiled with plain g++ against the header and linked
against librs_hip.so (CPU), and run on the device (-m gpu), where the digests it prints must equal the digests of the same
three statements solved through the Python path."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests.test_r1cs_solve_cpp import fnv1a, formula_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batch_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("r1cs_batch_run") / "r1cs_batch_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "r1cs_batch_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def statements(prm, B=3):
    """the system of tests/cpp/r1cs_batch_run.cpp and the two given wires of its B statements, by the same closed formulas"""
    cs = formula_system(prm)[0]
    s = np.arange(prm.N, dtype=object)
    asgs = []
    for b in range(B):
        asg = np.zeros((cs.n_vars, prm.L, prm.N), dtype=np.uint64)
        asg[0] = np.stack([((s * s + 3 + l + 17 * b) % int(p)).astype(np.uint64) for l, p in enumerate(prm.q)])
        asg[1] = np.stack([((7 * s + 11 + 5 * l + 29 * b) % int(p)).astype(np.uint64) for l, p in enumerate(prm.q)])
        asgs.append(asg)
    return cs, asgs


def test_batch_adapter_compiles_and_links(batch_run_exe):
    """solve_batch / is_satisfied_batch exist, and the library has the entry points."""
    assert os.path.exists(batch_run_exe)


def test_batch_header_compiles_alone():
    """r1cs_batch.hpp as the only include, plain C++17"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    src = "#include <ringsnark_amd/r1cs_batch.hpp>\nint main() { return 0; }\n"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_batch_adapter_runs_against_the_library(batch_run_exe):
    from ringsnark_amd.device import Device, to_host
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([batch_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "r1cs_batch_run: OK" in r.stdout, r.stdout + r.stderr
    digests = [int(d, 16) for d in re.search(r"digests ([0-9a-f]{16}) ([0-9a-f]{16}) ([0-9a-f]{16})", r.stdout).groups()]
    # the same statements through the Python path: the host mirror and the device give the adapter's words
    cs, asgs = statements(prm)
    exp = [R.solve(cs, {0, 1}, a, prm.q) for a in asgs]
    assert all(R.is_satisfied(cs, e, prm.q).satisfied for e in exp)
    assert [fnv1a(e.reshape(-1)) for e in exp] == digests and len(set(digests)) == 3
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    dasgs = [dev.put(a) for a in asgs]
    dev.r1cs_solve_batch(dev.r1cs_solve_plan(dcs, {0, 1}), dasgs)
    assert [fnv1a(to_host(d).reshape(-1)) for d in dasgs] == digests
    assert all(c.satisfied for c in dev.r1cs_check_batch(dcs, dasgs))
