"""ringsnark::amd::solve_plan / solve (include/ringsnark_amd/r1cs_solve.hpp), the C++ adapter of the device assignment solver:
tests/cpp/solve_run.cpp compiled with plain g++ against the header and linked against librs_hip.so (CPU), and run on the
device (-m gpu), where the digest it prints must equal the digest of the same system solved through the Python path."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def solve_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("solve_run") / "solve_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "solve_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def formula_system(prm, m=12):
    """the system and the two given wires of tests/cpp/solve_run.cpp, by the same closed formula"""
    rows = {"a": [], "b": [], "c": []}
    for i in range(m):
        rows["a"].append([(0, i % 4 + 1)] + [((7 * i + 3 * k) % (i + 2) + 1, ((i + k) % 5 - 2) or 1) for k in range(3)])
        rows["b"].append([(i + 2, 1)])
        rows["c"].append([(i + 3, 1)])
    cs = R.from_rows(m, m + 2, 2, rows, prm.q)
    s = np.arange(prm.N, dtype=object)
    x0 = np.stack([((s * s + 3 + l) % int(p)).astype(np.uint64) for l, p in enumerate(prm.q)])
    x1 = np.stack([((7 * s + 11 + 5 * l) % int(p)).astype(np.uint64) for l, p in enumerate(prm.q)])
    return cs, x0, x1


def fnv1a(words):
    h = 0xCBF29CE484222325
    for v in words:
        h = ((h ^ int(v)) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_solve_adapter_compiles_and_links(solve_run_exe):
    """solve_plan / solve exist, and the library has the entry points."""
    assert os.path.exists(solve_run_exe)


@pytest.mark.gpu
def test_solve_adapter_runs_against_the_library(solve_run_exe):
    from ringsnark_amd.device import Device, to_host
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([solve_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "solve_run: OK" in r.stdout, r.stdout + r.stderr
    digest = int(re.search(r"digest ([0-9a-f]{16})", r.stdout).group(1), 16)
    # the same system through the Python path: the host mirror and the device give the adapter's words
    cs, x0, x1 = formula_system(prm)
    asg = np.zeros((cs.n_vars, prm.L, prm.N), dtype=np.uint64)
    asg[0], asg[1] = x0, x1
    exp = R.solve(cs, {0, 1}, asg, prm.q)
    assert R.is_satisfied(cs, exp, prm.q).satisfied
    assert fnv1a(exp.reshape(-1)) == digest
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    dasg = dev.put(asg)
    dev.r1cs_solve(dev.r1cs_solve_plan(dcs, {0, 1}), dasg)
    assert fnv1a(to_host(dasg).reshape(-1)) == digest
