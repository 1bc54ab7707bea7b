"""ringsnark::amd::hint_plan / solve_hinted (include/ringsnark_amd/solve_hints.hpp), the C++ adapter of the device solver
with hints: tests/cpp/solve_hints_run.cpp compiled with plain g++ against the headers and linked against librs_hip.so (CPU),
and run on the device (-m gpu): the running maximum of three inputs in every mode and a quotient with a planted zero, checked
with the adapter's own is_satisfied and ring operations; its digest equals that of the host mirror's assignment."""
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
def solve_hints_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("solve_hints_run") / "solve_hints_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "solve_hints_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_solve_hints_adapter_compiles_and_links(solve_hints_run_exe):
    """hint_plan and solve_hinted exist, no reference header is needed, and the library has the entry points."""
    assert os.path.exists(solve_hints_run_exe)
    src = open(os.path.join(ROOT, "tests", "cpp", "solve_hints_run.cpp")).read()
    assert "libsnark" not in src and "<ringsnark/" not in src


@pytest.mark.gpu
def test_solve_hints_adapter_runs_against_the_library(solve_hints_run_exe):
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q]
    r = subprocess.run([solve_hints_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = re.search(r"^solve_hints_run: OK digest ([0-9a-f]{16})$", r.stdout, flags=re.M)
    assert line, r.stdout + r.stderr
    # the same circuit and inputs through the host mirror, and the program's FNV-1a over the assignment words
    cs, hints = R.running_max_r1cs(prm.q, 8, 2)
    s = np.arange(prm.N, dtype=np.uint64)
    asg = np.zeros((cs.n_vars, prm.L, prm.N), dtype=np.uint64)
    asg[0] = 1
    asg[1], asg[2], asg[3] = ((5 * s + 3) % 128)[None], ((11 * s + 70) % 128)[None], ((s * s) % 128)[None]
    out, rep = R.solve_hinted(cs, range(4), hints, asg, prm.q)
    assert rep.clean
    h = 0xcbf29ce484222325
    for v in out.reshape(-1):
        h = ((h ^ int(v)) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    assert int(line.group(1), 16) == h
