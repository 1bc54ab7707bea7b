"""The assignment solver (ringsnark_amd/r1cs_solve.h): the full assignment of a forward-determined R1CS from its given wires.

CPU (-m "not gpu"): the entry points exist; the host mirror ringsnark_amd.r1cs.solve (exact Python integers) reproduces the
assignments the existing generators build with the CPU oracle's ring operations; ringsnark_amd.r1cs.solve_schedule agrees
with a naive round-by-round restatement of the rules and with the facts written down for the known circuits; one hand-built
system per blocked reason and coefficient rule.
GPU (-m gpu): the device plan equals the host schedule field for field, and every kernel (levels, walk, auto; both
arithmetics) produces the words of the host mirror -- exact equality everywhere, no tolerance.  Rows of unknown wires hold
0xFF bytes before every call: the solver must neither read them nor, where they stay unsolved, write them."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H

FILL = np.uint64(0xFFFFFFFFFFFFFFFF)
MODES = ("auto", "levels", "walk")


# ---- the rules of r1cs_solve.h restated naively: rescan every constraint in every round (quadratic; test-only) ---------
def naive_schedule(cs, given, q):
    known = R.given_mask(cs, given).astype(bool)
    wires = lambda name, j: [int(c) - 1 for c in cs.mats[name][1][int(cs.mats[name][0][j]):int(cs.mats[name][0][j + 1])] if c]
    steps, level_ptr, used = [], [0], set()
    while True:
        fresh = {}
        for j in range(cs.m):
            if j in used or any(not known[v] for v in wires("a", j) + wires("b", j)):
                continue
            unknown = sorted({v for v in wires("c", j) if not known[v]})
            if len(unknown) != 1 or unknown[0] in fresh:
                continue
            t = unknown[0]
            rp, col, coeff = cs.mats["c"]
            on_t = [e for e in range(int(rp[j]), int(rp[j + 1])) if col[e] == t + 1]
            if cs.poly_idx is not None and any(cs.poly_idx["c"][e] >= 0 for e in on_t):
                continue
            if any(sum(int(coeff[l, e]) for e in on_t) % int(p) == 0 for l, p in enumerate(q)):
                continue
            fresh[t] = j
        if not fresh:
            return steps, level_ptr
        for t, j in sorted(fresh.items(), key=lambda kv: kv[1]):
            steps.append((j, t))
            used.add(j)
            known[t] = True
        level_ptr.append(len(steps))


# ---- systems: (prm, cs, given, assignment with the unknown rows filled with 0xFF), built once and never written to ---------
def with_fill(cs, prm, given, rows):
    asg = np.full((cs.n_vars, prm.L, prm.N), FILL, dtype=np.uint64)
    for v, r in zip(given, rows):
        asg[v] = r
    asg.setflags(write=False)
    return asg


def ring256():
    """N = 256, three ring primes: 384 slot pairs, one full chunk of 256 and a ragged one of 128"""
    return P.make_params(256, [30, 30, 30], 256, [40, 41], ring_factor=1 << 12, name="ring256")


def mixed_r1cs(W, q):
    """W products of given pairs (one wide level), a depth-8 chain through the first of them (eight levels of width 1), W
    products with the chain's end (one wide level).  Variables: u_i = i, v_i = W + i (given), then p_i, c_1..c_8, r_i."""
    u, v, p, c, r = (lambda i: i + 1), (lambda i: W + i + 1), (lambda i: 2 * W + i + 1), (lambda k: 3 * W + k), (lambda i: 3 * W + 9 + i)
    rows = {"a": [], "b": [], "c": []}
    for i in range(W):
        rows["a"].append([(u(i), 1)]), rows["b"].append([(v(i), 1)]), rows["c"].append([(p(i), 1)])
    for k in range(8):
        rows["a"].append([(p(0) if k == 0 else c(k), 1)]), rows["b"].append([(u(k), 1), (0, k + 1)]), rows["c"].append([(c(k + 1), 1)])
    for i in range(W):
        rows["a"].append([(c(8), 1)]), rows["b"].append([(v(i), 1)]), rows["c"].append([(r(i), -1), (0, 3)])
    return R.from_rows(2 * W + 8, 4 * W + 8, 0, rows, q)


@functools.lru_cache(maxsize=None)
def system(name):
    """"<system>@<preset>": the system on that preset's ring instead of toy's"""
    name, _, preset = name.partition("@")
    if name in ("ring256_wide40", "mixed"):
        prm = ring256()
    else:
        prm = P.preset(preset or "toy")
    if name == "mixed":
        chunks = -(-(prm.L * prm.N // 2) // 256)
        W = -(-R.SOLVE_FILL_WORKGROUPS // chunks)  # the smallest width that RS_SOLVE_AUTO gives to the level kernel on this ring
        cs, given = mixed_r1cs(W, prm.q), list(range(2 * W))
        rng = np.random.RandomState(5)
        rows = [np.stack([rng.randint(0, int(p), prm.N).astype(np.uint64) for p in prm.q]) for _ in given]
        return prm, cs, given, with_fill(cs, prm, given, rows)
    ctx = H.oracle_ctx(prm)
    if name in ("wide40", "ring256_wide40"):
        cs, given = R.wide_r1cs(40, prm.q), [0, 1]
    elif name == "chain40":
        cs, given = R.chain_r1cs(40, prm.q), [0, 1]
    elif name == "poly20":
        cs, given = R.wide_poly_r1cs(20, prm.q, prm.N), [0, 1]
    elif name == "logreg4":
        cs, given = R.logreg_r1cs(prm.q, 4), list(range(16))
    elif name == "logreg4_partial":
        cs, given = R.logreg_r1cs(prm.q, 4), list(range(15))
    else:
        cs, given = hand_systems(prm)[name][:2]
    rows = ctx.random_ring(7, len(given)) if name.startswith("logreg") else [ctx.random_ring(7 + k) for k in range(len(given))]
    return prm, cs, given, with_fill(cs, prm, given, rows)


@functools.lru_cache(maxsize=None)
def solved(name):
    """R.solve of system(name): computed once, shared, read-only"""
    prm, cs, given, asg = system(name)
    out = R.solve(cs, given, asg, prm.q)
    out.setflags(write=False)
    return out


def hand_systems(prm):
    """name -> (cs, given, expected steps, expected (n_unused, first_blocked, blocked_reason)): one system per coefficient rule and
    per blocked reason.  Columns: 0 is the constant one, variable v is column v + 1; x1 x2 x3 x4 below are variables 0 1 2 3."""
    q = prm.q
    poly = np.stack([np.arange(1, prm.N + 1, dtype=np.uint64) % np.uint64(p) for p in q])
    one = lambda a, b, c, n_vars: R.from_rows(1, n_vars, 0, {"a": [a], "b": [b], "c": [c]}, q)
    return {
        # x1 * x2 = 3 x3 + 4 x3 - 2 x1 + 5: the target entered twice, a negative coefficient, a constant term: k = 7
        "k7": (one([(1, 1)], [(2, 1)], [(3, 3), (3, 4), (1, -2), (0, 5)], 3), [0, 1], [(0, 2)], (0, 1, 0)),
        "reason1": (one([(1, 1)], [(2, 1)], [(3, 1)], 3), [0], [], (1, 0, 1)),  # x2 unknown
        "reason2": (one([(1, 1)], [(2, 1)], [(3, 1), (4, 1)], 4), [0, 1], [], (1, 0, 2)),
        "reason3": (one([(1, 1)], [(2, 1)], [(3, poly)], 3), [0, 1], [], (1, 0, 3)),
        "reason4": (one([(1, 1)], [(2, 1)], [(3, int(q[0]))], 3), [0, 1], [], (1, 0, 4)),  # zero in limb 0 only
        "reason5": (one([(3, 1)], [(1, 1)], [(3, 1)], 3), [0, 1], [], (1, 0, 5)),
        # two constraints able to determine x3 in the same level: the lower one is the step, the other determines nothing
        "tie": (R.from_rows(2, 3, 0, {"a": [[(2, 1)], [(1, 1)]], "b": [[(1, 1)], [(2, 1)]], "c": [[(3, 1)], [(3, 1)]]}, q), [0, 1], [(0, 2)],
                (1, 2, 0)),
    }


HAND = ("k7", "reason1", "reason2", "reason3", "reason4", "reason5", "tie")
SCHEDULED = ("chain40", "wide40", "poly20", "logreg4", "logreg4_partial") + HAND  # the systems of the plan-against-mirror test


def info_tuple(i):
    return tuple(int(getattr(i, f)) for f in ("n_given", "n_solved", "n_unsolved", "first_unsolved", "n_levels", "max_width", "n_unused",
                                              "first_blocked", "blocked_reason"))


# ---- CPU -----------------------------------------------------------------------------------------------------------
def test_library_exports_the_solver():
    from ringsnark_amd import _lib
    lib = _lib.load()
    names = {"rs_r1cs_solve_plan_create", "rs_r1cs_solve_plan_steps", "rs_r1cs_solve_plan_destroy", "rs_r1cs_solve"}
    assert names == set(_lib.SOLVE_SIGNATURES) and all(hasattr(lib, n) for n in names)
    assert lib.rs_version() >= 107
    # the header of the solver declares what _lib binds for it, no more and no less (comments aside)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ringsnark_amd", "r1cs_solve.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code)) == set(_lib.SOLVE_SIGNATURES)
    # and nothing of it in ringsnark_amd.h
    assert "solve" not in open(os.path.join(root, "include", "ringsnark_amd.h")).read()


@pytest.mark.parametrize("name", ["wide40", "poly20"])
def test_host_solve_matches_solve_forward_on_the_oracle(name):
    prm, cs, given, asg = system(name)
    exp = H.make_assignment(H.oracle_ctx(prm), cs)  # R.solve_forward on the oracle's ring operations, x0, x1 from seeds 7, 8
    assert (exp[:2] == asg[:2]).all()
    got = solved(name)
    assert got.dtype == np.uint64 and (got == exp).all()
    assert R.is_satisfied(cs, got, prm.q).satisfied


def test_host_solve_matches_logreg_assignment_on_the_oracle():
    prm, cs, given, asg = system("logreg4")
    ctx = H.oracle_ctx(prm)
    exp = R.logreg_assignment(4, np.array(asg[:16]), ctx.ring_mul, ctx.ring_add, ctx.ring_mul_scalar)
    got = solved("logreg4")
    assert (got == exp).all()
    assert R.is_satisfied(cs, got, prm.q).satisfied


def test_schedule_facts():
    toy = P.preset("toy")
    for name in ("chain40", "wide40"):
        prm, cs, given, _ = system(name)
        steps, lp, info = R.solve_schedule(cs, given, prm.q)
        assert steps == [(i, i + 2) for i in range(40)] and lp == list(range(41))
        assert info_tuple(info) == (2, 40, 0, 42, 40, 1, 0, 40, 0)
    prm, cs, given, _ = system("logreg4")
    steps, lp, info = R.solve_schedule(cs, given, prm.q)
    assert list(np.diff(lp)) == [16, 6, 1] and info_tuple(info) == (16, 23, 0, 39, 3, 16, 0, 23, 0)
    assert steps[:16] == [(i, 21 + (i % 4) * 4 + i // 4) for i in range(16)]  # p00[i], p01[i], p10[i], p11[i] per feature
    assert steps[-1] == (20, 18)  # out2 = 2 s02 + s11 waits for both
    cs = R.logreg_r1cs(toy.q, 256)
    steps, lp, info = R.solve_schedule(cs, range(1024), toy.q)
    assert list(np.diff(lp)) == [1024, 6, 1] and info.n_unsolved == 0 and info.n_solved == 1031
    prm, cs, given, _ = system("logreg4_partial")
    info = R.solve_schedule(cs, given, prm.q)[2]
    assert (info.n_given, info.n_solved, info.n_unsolved, info.first_unsolved) == (15, 15, 9, 15)
    assert (info.first_blocked, info.blocked_reason) == (13, 1)  # in1[3][0] * in2[3][1]: its b side is the wire not given


@pytest.mark.parametrize("name", SCHEDULED + ("mixed",))
def test_schedule_agrees_with_the_naive_restatement(name):
    prm, cs, given, _ = system(name)
    steps, lp, info = R.solve_schedule(cs, given, prm.q)
    assert (steps, lp) == naive_schedule(cs, given, prm.q)
    assert info.n_solved == len(steps) and info.n_levels == len(lp) - 1 and info.n_unused == cs.m - len(steps)
    assert info.n_given + info.n_solved + info.n_unsolved == cs.n_vars
    # a bool mask says the same as the list of variables
    mask = np.zeros(cs.n_vars, dtype=bool)
    mask[list(given)] = True
    assert R.solve_schedule(cs, mask, prm.q)[:2] == (steps, lp)


@pytest.mark.parametrize("name", HAND)
def test_hand_built_rules(name):
    prm = P.preset("toy")
    cs, given, exp_steps, (n_unused, first_blocked, reason) = hand_systems(prm)[name]
    steps, lp, info = R.solve_schedule(cs, given, prm.q)
    assert steps == exp_steps and lp == ([0, len(steps)] if steps else [0])
    assert (info.n_unused, info.first_blocked, info.blocked_reason) == (n_unused, first_blocked, reason)
    assert info.n_unsolved == cs.n_vars - len(given) - len(steps)
    assert reason in R.SOLVE_BLOCKED
    _, _, _, asg = system(name)
    got = solved(name)
    unsolved = [v for v in range(cs.n_vars) if v not in given and v not in [t for _, t in steps]]
    assert (got[unsolved] == FILL).all() and (got[list(given)] == asg[list(given)]).all()
    if name == "k7":
        for l, p in enumerate(prm.q):
            x1, x2 = asg[0, l].astype(object), asg[1, l].astype(object)
            assert (got[2, l].astype(object) == (x1 * x2 + 2 * x1 - 5) * pow(7, -1, int(p)) % int(p)).all()
        assert R.is_satisfied(cs, got, prm.q).satisfied
    if name == "tie":
        assert R.is_satisfied(cs, got, prm.q).satisfied  # the constraint that determines nothing holds: it is a check


# ---- GPU -----------------------------------------------------------------------------------------------------------
def run_device(dev, dcs, plan, asg, mode, **kw):
    from ringsnark_amd.device import to_host
    dasg = dev.put(np.array(asg))  # a copy: the shared assignments are read-only
    stats = dev.r1cs_solve(plan, dasg, mode=mode, **kw)
    return to_host(dasg), stats, dasg


def assert_stats(stats, mode, info):
    if not info.n_solved:
        assert stats == (0, 0)
    elif mode == "levels":
        assert stats == (info.n_levels, 0)
    elif mode == "walk":
        assert stats == (0, 1)
    else:
        assert 1 <= sum(stats) <= info.n_levels


@pytest.mark.gpu
def test_device_plan_equals_the_host_schedule():
    from ringsnark_amd.device import Device
    dev = Device(P.preset("toy"))
    for name in SCHEDULED:
        prm, cs, given, _ = system(name)
        steps, lp, info = R.solve_schedule(cs, given, prm.q)
        plan = dev.r1cs_solve_plan(dev.r1cs(cs), given)
        assert info_tuple(plan.info) == info_tuple(info), name
        assert plan.steps() == (steps, lp), name
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("force_int", [0, 1])
@pytest.mark.parametrize("name", ["wide40", "poly20", "logreg4"])
def test_device_solve_every_mode_both_arithmetics(name, force_int):
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    prm, cs, given, asg = system(name)
    exp = solved(name)
    with _lib.tuning(force_int_arith=force_int):
        dev = Device(prm)
        dcs = dev.r1cs(cs)
        plan = dev.r1cs_solve_plan(dcs, given)
        assert plan.info.n_unsolved == 0
        for mode in MODES:
            got, stats, dasg = run_device(dev, dcs, plan, asg, mode)
            assert (got == exp).all(), (mode, np.argwhere(got != exp)[:4])
            assert dev.r1cs_check(dcs, dasg).n_violated == 0
            assert_stats(stats, mode, plan.info)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wide40@toy49", "wide40@toy50", "poly20@toy50"])
def test_device_solve_at_the_top_of_the_fp64_range(name):
    """49-bit primes and primes just below 2^50 (toy50: the largest the FP64 arithmetic accepts, N = 64): every product of
    two loaded wires is canonical x canonical, up to p^2 (f64mod.hpp's second regime).  Every mode against R.solve."""
    from ringsnark_amd.device import Device
    prm, cs, given, asg = system(name)
    assert all(p < 1 << 50 for p in prm.q + prm.Q) and (name.endswith("toy50")) == all(p > 1 << 49 for p in prm.q)
    exp = solved(name)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    assert plan.info.n_unsolved == 0
    for mode in MODES:
        got, stats, dasg = run_device(dev, dcs, plan, asg, mode)
        assert (got == exp).all(), (mode, np.argwhere(got != exp)[:4])
        assert dev.r1cs_check(dcs, dasg).n_violated == 0
        assert_stats(stats, mode, plan.info)


@pytest.mark.gpu
def test_device_solve_hand_built_rules():
    """k = 7 with its negative coefficient and constant term, and every blocked system: nothing read, nothing written"""
    from ringsnark_amd.device import Device
    dev = Device(P.preset("toy"))
    for name in HAND:
        prm, cs, given, asg = system(name)
        dcs = dev.r1cs(cs)
        plan = dev.r1cs_solve_plan(dcs, given)
        for mode in MODES:
            got, stats, _ = run_device(dev, dcs, plan, asg, mode, allow_partial=True)
            assert (got == solved(name)).all(), (name, mode)
            assert_stats(stats, mode, plan.info)


@pytest.mark.gpu
def test_device_solve_partial_plan():
    from ringsnark_amd.device import Device
    prm, cs, given, asg = system("logreg4_partial")
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    with pytest.raises(ValueError) as e:
        dev.r1cs_solve(plan, dev.put(np.array(asg)))
    assert "first unsolved variable 15;" in str(e.value) and "first blocked constraint 13: an unknown wire in a or b" in str(e.value)
    exp = solved("logreg4_partial")
    steps = plan.steps()[0]
    done = [t for _, t in steps]
    rest = [v for v in range(cs.n_vars) if v not in given and v not in done]
    assert (len(done), len(rest)) == (15, 9)
    for mode in MODES:
        got, stats, _ = run_device(dev, dcs, plan, asg, mode, allow_partial=True)
        assert (got[done] == exp[done]).all() and (got[rest] == FILL).all() and (got == exp).all()
        assert_stats(stats, mode, plan.info)


@pytest.mark.gpu
def test_device_solve_equals_the_chain_kernel():
    from ringsnark_amd.device import Device, to_host
    prm = P.preset("toy")
    m = 5000
    dev = Device(prm)
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    base = dev.ring_empty(m + 2)
    base.fill_(-1)  # 0xFF bytes
    dev.fill_uniform(base[:2], 0, 9)
    exp = dev.chain_assignment(base.clone(), m)
    plan = dev.r1cs_solve_plan(dcs, [0, 1])
    assert info_tuple(plan.info) == (2, m, 0, m + 2, m, 1, 0, m, 0)
    for mode in MODES:
        got = base.clone()
        stats = dev.r1cs_solve(plan, got, mode=mode)
        assert to_host(got).tobytes() == to_host(exp).tobytes(), mode
        assert stats == {"auto": (0, 1), "levels": (m, 0), "walk": (0, 1)}[mode]
    assert dev.r1cs_check(dcs, exp).satisfied


@pytest.mark.gpu
def test_device_solve_equals_logreg_assignment_on_device_ring_ops():
    """logreg_r1cs(256) on C5 (N = 2048, one 54-bit ring prime: the integer arithmetic): the bespoke schedule of batched ring
    operations against the solver, device against device"""
    from ringsnark_amd.device import Device, to_host
    prm = P.preset("C5")
    F = 256
    dev = Device(prm)
    cs = R.logreg_r1cs(prm.q, F)
    dcs = dev.r1cs(cs)
    inputs = dev.fill_uniform(dev.ring_empty(4 * F), 0, 41)
    exp = R.logreg_assignment(F, inputs, dev.ring_mul, dev.ring_add, dev.ring_mul_scalar)
    plan = dev.r1cs_solve_plan(dcs, range(4 * F))
    assert info_tuple(plan.info) == (1024, 1031, 0, cs.n_vars, 3, 1024, 0, cs.m, 0)
    for mode in MODES:
        got = dev.ring_empty(cs.n_vars)
        got.fill_(-1)
        got[:4 * F] = inputs
        stats = dev.r1cs_solve(plan, got, mode=mode)
        assert to_host(got).tobytes() == to_host(exp).tobytes(), mode
        assert_stats(stats, mode, plan.info)
        assert dev.r1cs_check(dcs, got).satisfied


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["levels", "walk"])
def test_device_solve_full_and_ragged_slot_chunks(mode):
    """a thread owns a slot pair, a workgroup 256 of them: 384 pairs are one full chunk and a ragged one"""
    from ringsnark_amd.device import Device
    prm, cs, given, asg = system("ring256_wide40")
    assert prm.L * prm.N // 2 == 384
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    got, stats, dasg = run_device(dev, dcs, plan, asg, mode)
    assert (got == solved("ring256_wide40")).all()
    assert_stats(stats, mode, plan.info)
    assert dev.r1cs_check(dcs, dasg).satisfied


@pytest.mark.gpu
def test_device_solve_auto_uses_both_kernels():
    from ringsnark_amd.device import Device
    prm, cs, given, asg = system("mixed")
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    W = len(given) // 2
    _, lp, info = R.solve_schedule(cs, given, prm.q)
    assert list(np.diff(lp)) == [W] + [1] * 8 + [W] and info_tuple(plan.info) == info_tuple(info) and info.n_unsolved == 0
    exp = solved("mixed")
    for mode in MODES:
        got, stats, dasg = run_device(dev, dcs, plan, asg, mode)
        assert (got == exp).all(), mode
        assert_stats(stats, mode, plan.info)
        if mode == "auto":
            assert stats.level_launches >= 2 and stats.walk_launches >= 1
        assert dev.r1cs_check(dcs, dasg).satisfied


@pytest.mark.gpu
def test_plan_reuse_and_invalid_arguments():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device, to_host
    prm, cs, given, asg = system("wide40")
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_solve_plan(dcs, given)
    got, _, _ = run_device(dev, dcs, plan, asg, "auto")
    assert (got == solved("wide40")).all()
    other = np.array(asg)
    other[0], other[1] = H.oracle_ctx(prm).random_ring(21), H.oracle_ctx(prm).random_ring(22)
    got2, _, _ = run_device(dev, dcs, plan, other, "auto")
    assert (got2 == R.solve(cs, given, other, prm.q)).all() and not (got2[2:] == got[2:]).all()
    # a plan belongs to its context
    dasg = dev.put(np.array(asg))
    ptr = C.c_void_p(dasg.data_ptr())
    dev2 = Device(prm)
    assert dev2.lib.rs_r1cs_solve(dev2.h, plan.h, ptr, _lib.RS_SOLVE_AUTO, None, dev2.stream()) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_last_error().decode() == "solve plan of another context"
    assert dev.lib.rs_r1cs_solve(dev.h, plan.h, ptr, 3, None, dev.stream()) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_last_error().decode() == "unknown solve mode"
    assert dev.lib.rs_r1cs_solve(dev.h, None, ptr, 0, None, dev.stream()) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_r1cs_solve(dev.h, plan.h, None, 0, None, dev.stream()) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_r1cs_solve(None, plan.h, ptr, 0, None, dev.stream()) == _lib.RS_ERR_INVALID
    dev.sync()
    assert (to_host(dasg) == asg).all()  # none of the refused calls wrote anything
    # nothing to solve: a valid empty plan
    empty = dev.r1cs_solve_plan(dcs, range(cs.n_vars))
    assert info_tuple(empty.info) == (cs.n_vars, 0, 0, cs.n_vars, 0, 0, cs.m, cs.m, 0) and empty.steps() == ([], [0])
    assert dev.r1cs_solve(empty, dasg) == (0, 0)
