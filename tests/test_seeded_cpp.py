"""Seeded keys through the C++ adapters (include/ringsnark_amd/seeded.hpp: generator(cs, seeded), prover on a
seeded_proving_key): tests/cpp/seeded_run.cpp compiled with plain g++ and linked against librs_hip.so (CPU), and run on the
device (-m gpu): generator(seeded) -> prover -> verifier per scheme, and the proofs equal to the ones the Python path gives
for the same compact key and public seeds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def seeded_run_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("seeded_run") / "seeded_run")
    libdir = os.path.join(ROOT, "ringsnark_amd")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "seeded_run.cpp"), "-o", exe, "-L", libdir, "-lrs_hip",
                        "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_seeded_adapter_compiles_and_links(seeded_run_exe):
    """generator(cs, seeded), the provers on a seeded_proving_key, and the library's _seeded entry points"""
    assert os.path.exists(seeded_run_exe)


@pytest.mark.gpu
def test_seeded_adapter_runs_and_python_gives_the_same_proofs(seeded_run_exe, tmp_path):
    from ringsnark_amd.device import Device, to_host
    prm = P.preset("toy")
    args = [str(prm.N), str(prm.L)] + [str(x) for x in prm.q] + [str(prm.N_enc), str(prm.K)] + [str(x) for x in prm.Q] + [str(tmp_path)]
    r = subprocess.run([seeded_run_exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "seeded_run: OK" in r.stdout, r.stdout + r.stderr
    m = 6
    cs = R.chain_r1cs(m, prm.q)
    assert (cs.n_vars, cs.n_inputs) == (m + 2, 2)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    rd = lambda name: np.fromfile(str(tmp_path / name), dtype=np.uint64)
    compact = lambda name, n: dev.put(rd(name).reshape(n, prm.L, prm.K, prm.N_enc))
    full = lambda name: dev.put(rd(name).reshape(prm.L, 2, prm.K, prm.N_enc))
    inv = pow(65537, -1, 2**64)  # the dict holds seeds in enc_encode's convention, the C++ key the words of the C interface
    pub = lambda name: [(int(w) * inv) % 2**64 for w in rd(name)]
    asg = dev.put(rd("assignment.bin").reshape(m + 2, prm.L, prm.N))
    gpk = dict(s_pows=compact("g_s_pows.bin", m + 1), delta_ts=compact("g_delta_ts.bin", m + 1), delta_mid=compact("g_delta_mid.bin", m),
               alpha=full("g_alpha.bin"), beta=full("g_beta.bin"), pub_seeds=pub("g_pub.bin"))
    got, empty = dev.groth16_prove(dcs, gpk, asg)
    assert empty == [0, 0, 0] and (to_host(got).reshape(-1) == rd("g_proof.bin")).all()
    rpk = dict(s_pows=compact("r_s_pows.bin", m + 1), alpha_s_pows=compact("r_alpha_s_pows.bin", m + 1), beta_prods=compact("r_beta_prods.bin", m),
               beta_rv_ts=full("r_beta_rv_ts.bin"), beta_rw_ts=full("r_beta_rw_ts.bin"), beta_ry_ts=full("r_beta_ry_ts.bin"),
               pub_seeds=pub("r_pub.bin"))
    got, empty = dev.rinocchio_prove(dcs, rpk, asg)
    assert empty == [0] * 9 and (to_host(got).reshape(-1) == rd("r_proof.bin")).all()
