"""rs_r1cs_check: r1cs_constraint_system::is_satisfied (relations/constraint_satisfaction_problems/r1cs/r1cs.tcc:122-158)
as one fused pass on the device, with a report of where the system first fails.

CPU (-m "not gpu"): the entry point exists; the host mirror ringsnark_amd.r1cs.is_satisfied reproduces what the reference's
own headers printed (tests/golden/ref_r1cs_probe.json) and agrees with the CPU oracle's evaluations.
GPU (-m gpu): the device report and row flags equal an expectation computed from the CPU oracle's evaluations
(oracle.r1cs_evaluate per limb, multiply and compare in Python integers) -- exact equality everywhere, no tolerance.
Every field of the report is a function of the inputs, so equality is the whole test."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the fixture, loaded the way tests/test_golden.py loads it ---------------------------------------------------
def probe_cases():
    return json.load(open(os.path.join(GOLD, "ref_r1cs_probe.json")))["cases"]


def scalar_cases():
    return [c for c in probe_cases() if c["kind"] != "wide_poly"]


def poly_cases():
    return [c for c in probe_cases() if c["kind"] == "wide_poly"]


def probe_cs(case):
    rows = {}
    for name in "abc":
        mt = case["mats"][name]
        rp = mt["row_ptr"]
        rows[name] = [[(mt["col"][e], mt["coeff"][e]) for e in range(rp[i], rp[i + 1])] for i in range(case["m"])]
    return R.from_rows(case["m"], case["n_vars"], case["n_inputs"], rows, [case["q"]])


def probe_cs_poly(case, N=None):
    S = case["S"]
    reps = 1 if N is None else N // S
    rows = {}
    for name in "abc":
        mt = case["mats"][name]
        rp = mt["row_ptr"]
        coeff = lambda e: np.tile(np.array(mt["coeff"][e], dtype=np.uint64), reps)[None, :] if mt["is_poly"][e] else mt["coeff"][e][0]
        rows[name] = [[(mt["col"][e], coeff(e)) for e in range(rp[i], rp[i + 1])] for i in range(case["m"])]
    return R.from_rows(case["m"], case["n_vars"], case["n_inputs"], rows, [case["q"]])


def report_from_rows(triples, q, m, reps=1):
    """The expected report from the fixture's own rows: triples[i][s] = (a, b, c) of constraint i in fixture slot s, the
    fixture's slots tiled `reps` times over one limb."""
    S = len(triples[0])
    bad = np.array([[t[0] * t[1] % q != t[2] for t in row] for row in triples], dtype=bool)
    flags = bad.any(axis=1).astype(np.uint8)
    if not flags.any():
        return R.R1csCheck(0, m, 0, 0, 0, 0, 0, flags)
    row = int(np.argmax(flags))
    slot = int(np.argmax(bad[row]))  # its first copy is in the first tile: tiled slot `slot`
    assert slot < S * reps
    return R.R1csCheck(int(flags.sum()), row, 0, slot, *[int(v) for v in triples[row][slot]], flags)


# ---- the expectation of the GPU tests: the CPU oracle's evaluations, compared in Python integers --------------------
def expected_report(prm, cs, asg):
    ocs = H.oracle_cs(cs)
    m, L, N = cs.m, prm.L, prm.N
    ev = np.empty((3, m, L, N), dtype=object)
    for l in range(L):
        a_l = np.ascontiguousarray(asg[:, l, :])
        for k in range(3):
            ev[k, :, l, :] = O.r1cs_evaluate(int(prm.q[l]), ocs, k, l, a_l).astype(object)
    qs = np.array([int(p) for p in prm.q], dtype=object).reshape(1, L, 1)
    bad = ((ev[0] * ev[1]) % qs != ev[2]).reshape(m, L * N)
    flags = bad.any(axis=1).astype(np.uint8)
    if not flags.any():
        return R.R1csCheck(0, m, 0, 0, 0, 0, 0, flags)
    row = int(np.argmax(flags))
    idx = int(np.argmax(bad[row]))
    limb, slot = idx // N, idx % N
    return R.R1csCheck(int(flags.sum()), row, limb, slot, int(ev[0, row, limb, slot]), int(ev[1, row, limb, slot]),
                       int(ev[2, row, limb, slot]), flags)


FIELDS = ("n_violated", "first_row", "first_limb", "first_slot", "a", "b", "c")


def fields(r):
    return tuple(int(getattr(r, f)) for f in FIELDS)


def assert_same(got, exp):
    assert fields(got) == fields(exp), (fields(got), fields(exp))
    assert got.satisfied == exp.satisfied == (exp.n_violated == 0)
    gf = got.flags if isinstance(got.flags, np.ndarray) else got.flags.cpu().numpy()
    assert gf.dtype == np.uint8 and (gf == exp.flags).all(), (np.nonzero(gf)[0][:8], np.nonzero(exp.flags)[0][:8])


@functools.lru_cache(maxsize=None)
def system(preset, kind, m, width=8):
    """(prm, cs, satisfying assignment): computed once, shared, never written to (tampered copies are copies)."""
    prm = P.preset(preset)
    if kind == "wide":
        cs = R.wide_r1cs(m, prm.q, width=width)
    else:
        cs = R.wide_poly_r1cs(m, prm.q, prm.N)
    asg = H.make_assignment(H.oracle_ctx(prm), cs)
    asg.setflags(write=False)
    return prm, cs, asg


def tampered(prm, asg, *places):
    """a copy with 1 added (mod q) to wire w at (limb, slot) for every (w, limb, slot)"""
    out = asg.copy()
    for w, limb, slot in places:
        out[w, limb, slot] = (int(out[w, limb, slot]) + 1) % int(prm.q[limb])
    return out


def tamper_sets(prm, cs):
    L, N = prm.L, prm.N
    return {"first": [(0, 0, 0)],  # primary wire 0 at limb 0, slot 0
            "last": [(cs.n_vars - 1, L - 1, N - 1)],  # the last auxiliary wire at the last limb, slot N - 1
            # two wires at once, in different limbs -- on toy54, whose ring has ONE prime, in different slots of its only limb:
            # the two-limb case is covered by toy, toy49 and toy60 (asserted in the test)
            "two": [(1, 0, 5), (cs.n_vars - 1, L - 1, N - 2)]}


def hand_system(q, N):
    """Six rows with what wide_r1cs does not have: an empty `a` and `c` (0 * b = 0), constant terms only, constants mixed
    with variables, a constant `b`.  x1, x2 primary; returns (cs, assignment [6][L][N])."""
    rows = {"a": [[(1, 1)], [], [(0, 3)], [(0, 2), (1, 1)], [(3, 1), (0, 4)], [(4, 1)]],
            "b": [[(2, 1)], [(3, 1)], [(0, 5)], [(2, 1), (0, -1)], [(0, 1)], [(5, 1)]],
            "c": [[(3, 1)], [], [(0, 15)], [(4, 1)], [(5, 1)], [(6, 1)]]}
    cs = R.from_rows(6, 6, 2, rows, q)
    rng = np.random.RandomState(3)
    asg = np.zeros((6, len(q), N), dtype=np.uint64)
    for l, p in enumerate(q):
        p = int(p)
        for s in range(N):
            x1, x2 = int(rng.randint(1, 1 << 30)) % p, int(rng.randint(1, 1 << 30)) % p
            x3 = x1 * x2 % p
            x4 = (2 + x1) * (x2 - 1) % p
            x5 = (x3 + 4) % p
            asg[:, l, s] = [x1, x2, x3, x4, x5, x4 * x5 % p]
    return cs, asg


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_check():
    from ringsnark_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rs_r1cs_check") and "rs_r1cs_check" in _lib.CHECK_SIGNATURES
    assert lib.rs_version() >= 102
    # the header of the check declares what _lib binds for it, no more and no less (comments aside)
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ringsnark_amd", "r1cs_check.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code)) == set(_lib.CHECK_SIGNATURES)


def test_host_mirror_matches_reference_headers_fixture():
    """R.is_satisfied against what the reference's own headers printed: its verdict per slot / run, and -- where the
    fixture says `unsatisfied` -- the violated rows, the first of them and the three values there, all from the fixture's
    own rows.  The GPU tests' host references are pinned here."""
    cases = scalar_cases()
    assert len(cases) == 3
    for case in cases:
        q, m = case["q"], case["m"]
        cs = probe_cs(case)
        assert [s["satisfied"] for s in case["slots"]] == [1, 1, 1, 0]
        for s in case["slots"]:
            asg = np.array(s["assignment"], dtype=np.uint64).reshape(-1, 1, 1)
            got = R.is_satisfied(cs, asg, [q])
            assert int(got.satisfied) == s["satisfied"]
            exp = report_from_rows([[tuple(r)] for r in s["rows"]], q, m)
            assert int(exp.satisfied) == s["satisfied"]
            assert_same(got, exp)
    cases = poly_cases()
    assert len(cases) >= 2
    for case in cases:
        q, m, S = case["q"], case["m"], case["S"]
        cs = probe_cs_poly(case)
        assert [r["satisfied"] for r in case["runs"]] == [1, 0]
        for run in case["runs"]:
            asg = np.array(run["assignment"], dtype=np.uint64)[:, None, :]  # [n_vars][1][S]
            got = R.is_satisfied(cs, asg, [q])
            assert int(got.satisfied) == run["satisfied"]
            exp = report_from_rows([[tuple(run["rows"][i][k][s] for k in range(3)) for s in range(S)] for i in range(m)], q, m)
            assert int(exp.satisfied) == run["satisfied"]
            assert_same(got, exp)


def test_host_mirror_agrees_with_the_oracle_expectation():
    """the two host references of this file -- the exact mirror and the oracle's evaluations -- give the same report on
    multi-limb systems with polynomial coefficients, index-0 terms and empty rows"""
    prm, cs, asg = system("toy", "poly", 20)
    for a in (asg, tampered(prm, asg, (4, 1, 9)), tampered(prm, asg, (0, 0, 0), (7, 1, 31))):
        assert_same(R.is_satisfied(cs, a, prm.q), expected_report(prm, cs, a))
    prm = P.preset("toy")
    cs, asg = hand_system(prm.q, prm.N)
    exp = expected_report(prm, cs, asg)
    assert exp.satisfied
    assert_same(R.is_satisfied(cs, asg, prm.q), exp)
    bad = tampered(prm, asg, (2, 1, 7))
    exp = expected_report(prm, cs, bad)
    assert list(np.nonzero(exp.flags)[0]) == [0, 4] and (exp.first_limb, exp.first_slot) == (1, 7)  # row 1 has an empty `a`
    assert_same(R.is_satisfied(cs, bad, prm.q), exp)


# ---- GPU -----------------------------------------------------------------------------------------------------------
def device_report(dev, dcs, asg):
    return dev.r1cs_check(dcs, dev.put(np.array(asg)), want_flags=True)  # a copy: the shared assignments are read-only


@pytest.mark.gpu
def test_device_check_matches_reference_headers_fixture_scalar():
    from ringsnark_amd.device import Device
    toy = P.preset("toy")
    for case in scalar_cases():
        q, m = case["q"], case["m"]
        prm = P.RingParams(toy.N, [q], toy.N_enc, toy.Q, name="probe")
        dev = Device(prm)
        cs = probe_cs(case)
        S = len(case["slots"])
        asg = np.zeros((case["n_vars"], 1, prm.N), dtype=np.uint64)
        for slot in range(prm.N):
            asg[:, 0, slot] = case["slots"][slot % S]["assignment"]
        exp = report_from_rows([[tuple(case["slots"][s]["rows"][i]) for s in range(S)] for i in range(m)], q, m, prm.N // S)
        assert exp.n_violated >= 1 and exp.first_limb == 0 and exp.first_slot == S - 1  # the fixture's last slot is the tampered one
        dcs = dev.r1cs(cs)
        assert_same(device_report(dev, dcs, asg), exp)
        # the satisfied slots alone
        asg_ok = np.repeat(asg[:, :, :1], prm.N, axis=2)
        got = device_report(dev, dcs, asg_ok)
        assert fields(got) == (0, m, 0, 0, 0, 0, 0) and not got.flags.any()


@pytest.mark.gpu
@pytest.mark.parametrize("force_int", [0, 1])
def test_device_check_matches_reference_headers_fixture_poly(force_int):
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    toy = P.preset("toy")
    with _lib.tuning(force_int_arith=force_int):
        for case in poly_cases():
            q, m, S = case["q"], case["m"], case["S"]
            prm = P.RingParams(toy.N, [q], toy.N_enc, toy.Q, name="probe")
            dev = Device(prm)
            dcs = dev.r1cs(probe_cs_poly(case, prm.N))
            for run in case["runs"]:
                asg = np.tile(np.array(run["assignment"], dtype=np.uint64), (1, prm.N // S))[:, None, :].copy()
                exp = report_from_rows([[tuple(run["rows"][i][k][s] for k in range(3)) for s in range(S)] for i in range(m)], q, m,
                                       prm.N // S)
                assert int(exp.satisfied) == run["satisfied"] and exp.first_limb == 0
                assert_same(device_report(dev, dcs, asg), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 33, 1000])
@pytest.mark.parametrize("preset", ["toy", "toy49", "toy50", "toy54", "toy60"])
def test_device_check_both_arithmetics(preset, m):
    from ringsnark_amd.device import Device
    prm, cs, asg = system(preset, "wide", m)
    assert prm.L == (1 if preset == "toy54" else 2)
    two = tamper_sets(prm, cs)["two"]
    assert (two[0][1] != two[1][1]) == (prm.L > 1)  # the "two" set spans two limbs on every preset that has two
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    got = device_report(dev, dcs, asg)
    assert fields(got) == (0, m, 0, 0, 0, 0, 0) and got.satisfied and not got.flags.any()
    assert expected_report(prm, cs, asg).satisfied
    for name, places in tamper_sets(prm, cs).items():
        bad = tampered(prm, asg, *places)
        exp = expected_report(prm, cs, bad)
        assert exp.n_violated >= 1, name  # not vacuous: the tampered wire is used
        if m >= 33:
            assert exp.n_violated < m, name
        assert_same(device_report(dev, dcs, bad), exp)


@pytest.mark.gpu
def test_device_check_long_rows_at_the_fp64_corner():
    """rows of 68 terms on 49-bit primes: the lazy sums must be reduced every four terms (f64mod.hpp)"""
    from ringsnark_amd.device import Device
    prm, cs, asg = system("toy49", "wide", 40, 67)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    exp = expected_report(prm, cs, asg)
    assert exp.satisfied
    assert_same(device_report(dev, dcs, asg), exp)
    bad = tampered(prm, asg, (3, 1, 17))
    exp = expected_report(prm, cs, bad)
    assert 1 <= exp.n_violated < 40
    assert_same(device_report(dev, dcs, bad), exp)


@pytest.mark.gpu
def test_device_check_long_rows_at_the_top_of_the_fp64_range():
    """the same rows of 68 terms on primes just below 2^50: four products of up to 0.875 p each (f64mod.hpp's second regime)
    reach 3.5 p of the 4 p = 2^52 a reduction accepts"""
    from ringsnark_amd.device import Device
    prm, cs, asg = system("toy50", "wide", 40, 67)
    assert all(1 << 49 < p < 1 << 50 for p in prm.q)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    exp = expected_report(prm, cs, asg)
    assert exp.satisfied
    assert_same(device_report(dev, dcs, asg), exp)
    bad = tampered(prm, asg, (3, 1, 17))
    exp = expected_report(prm, cs, bad)
    assert 1 <= exp.n_violated < 40
    assert_same(device_report(dev, dcs, bad), exp)


@pytest.mark.gpu
def test_device_check_constant_terms_and_empty_rows():
    from ringsnark_amd.device import Device
    prm = P.preset("toy")
    cs, asg = hand_system(prm.q, prm.N)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    exp = expected_report(prm, cs, asg)
    assert exp.satisfied
    assert_same(device_report(dev, dcs, asg), exp)
    bad = tampered(prm, asg, (2, 1, 7))
    exp = expected_report(prm, cs, bad)
    assert list(np.nonzero(exp.flags)[0]) == [0, 4]
    assert_same(device_report(dev, dcs, bad), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["toy", "toy54"])
def test_device_check_polynomial_coefficients(preset):
    from ringsnark_amd.device import Device
    prm, cs, asg = system(preset, "poly", 20)
    assert cs.poly_table is not None and cs.poly_table.shape[0] > 1
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    exp = expected_report(prm, cs, asg)
    assert exp.satisfied
    assert_same(device_report(dev, dcs, asg), exp)
    bad = tampered(prm, asg, (4, prm.L - 1, 9))
    exp = expected_report(prm, cs, bad)
    assert 1 <= exp.n_violated < 20
    assert_same(device_report(dev, dcs, bad), exp)


@pytest.mark.gpu
def test_device_check_many_workgroups_along_the_slots():
    """N = 4096, L = 2: sixteen slot chunks.  The only violation sits in the last slot of the last limb; a second one in limb 0
    must take over as the first.  The same call twice gives the same report."""
    from ringsnark_amd.device import Device
    prm, cs, asg = system("C2", "wide", 70)
    assert (prm.N, prm.L) == (4096, 2)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    out_wire = cs.n_vars - 1  # the last row's output
    bad = tampered(prm, asg, (out_wire, 1, 4095))
    exp = expected_report(prm, cs, bad)
    assert (exp.n_violated, exp.first_row, exp.first_limb, exp.first_slot) == (1, 69, 1, 4095)
    got = device_report(dev, dcs, bad)
    assert_same(got, exp)
    again = device_report(dev, dcs, bad)
    assert fields(again) == fields(got) and (again.flags == got.flags).all()
    bad2 = tampered(prm, asg, (out_wire, 1, 4095), (out_wire, 0, 1))
    exp2 = expected_report(prm, cs, bad2)
    assert (exp2.n_violated, exp2.first_row, exp2.first_limb, exp2.first_slot) == (1, 69, 0, 1)
    got2 = device_report(dev, dcs, bad2)
    assert_same(got2, exp2)
    assert fields(device_report(dev, dcs, bad2)) == fields(got2)
    assert device_report(dev, dcs, asg).satisfied


@pytest.mark.gpu
def test_prover_with_check_refuses_an_unsatisfied_assignment():
    from ringsnark_amd.device import Device, to_host
    prm, cs, asg = system("toy", "wide", 33)
    ctx = H.oracle_ctx(prm)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    pk = {k: dev.put(v) for k, v in dict(s_pows=ctx.random_enc(1, cs.m + 1), delta_ts=ctx.random_enc(2, cs.m + 1),
                                         delta_mid=ctx.random_enc(3, cs.n_aux), alpha=ctx.random_enc(4), beta=ctx.random_enc(5)).items()}
    bad = tampered(prm, asg, *tamper_sets(prm, cs)["last"])
    exp = expected_report(prm, cs, bad)
    with pytest.raises(ValueError) as e:
        dev.groth16_prove(dcs, pk, dev.put(bad), check=True)
    assert "constraint %d at limb %d, slot %d" % (exp.first_row, exp.first_limb, exp.first_slot) in str(e.value)
    dasg = dev.put(np.array(asg))
    plain, empty = dev.groth16_prove(dcs, pk, dasg)
    checked, empty_c = dev.groth16_prove(dcs, pk, dasg, check=True)
    assert empty == empty_c and to_host(plain).tobytes() == to_host(checked).tobytes()


@pytest.mark.gpu
def test_rinocchio_prover_with_check_refuses_an_unsatisfied_assignment():
    from ringsnark_amd.device import Device, to_host
    prm, cs, asg = system("toy", "wide", 33)
    ctx = H.oracle_ctx(prm)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    pk = {k: dev.put(v) for k, v in dict(s_pows=ctx.random_enc(81, cs.m + 1), alpha_s_pows=ctx.random_enc(82, cs.m + 1),
                                         beta_prods=ctx.random_enc(83, cs.n_aux), beta_rv_ts=ctx.random_enc(84),
                                         beta_rw_ts=ctx.random_enc(85), beta_ry_ts=ctx.random_enc(86)).items()}
    ds = [dev.put(ctx.random_ring(60 + k)) for k in range(3)]
    bad = tampered(prm, asg, *tamper_sets(prm, cs)["first"])
    exp = expected_report(prm, cs, bad)
    with pytest.raises(ValueError) as e:
        dev.rinocchio_prove(dcs, pk, dev.put(bad), *ds, check=True)
    assert "constraint %d at limb %d, slot %d" % (exp.first_row, exp.first_limb, exp.first_slot) in str(e.value)
    dasg = dev.put(np.array(asg))
    plain, empty = dev.rinocchio_prove(dcs, pk, dasg, *ds)
    checked, empty_c = dev.rinocchio_prove(dcs, pk, dasg, *ds, check=True)
    assert empty == empty_c and to_host(plain).tobytes() == to_host(checked).tobytes()


@pytest.mark.gpu
def test_null_report_is_an_invalid_argument():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    prm, cs, asg = system("toy", "wide", 1)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    dasg = dev.put(np.array(asg))
    status = dev.lib.rs_r1cs_check(dev.h, dcs.h, C.c_void_p(dasg.data_ptr()), None, None, dev.stream())
    assert status == _lib.RS_ERR_INVALID
    assert dev.lib.rs_last_error().decode() == "null argument"
    rep = _lib.R1csReport()
    assert dev.lib.rs_r1cs_check(dev.h, dcs.h, None, None, C.byref(rep), dev.stream()) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_r1cs_check(dev.h, None, C.c_void_p(dasg.data_ptr()), None, C.byref(rep), dev.stream()) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_r1cs_check(None, dcs.h, C.c_void_p(dasg.data_ptr()), None, C.byref(rep), dev.stream()) == _lib.RS_ERR_INVALID
