"""Solver hints (ringsnark_amd/solve_hints.h) on the host: the entry points exist, and the host mirrors
ringsnark_amd.r1cs.solve_hinted_schedule / solve_hinted follow the rules written in the header -- reservation, readiness,
levels, order, the refusals -- on the two circuits that need hints of solved wires (a running maximum, a continued
fraction) and on hand-built systems, one per rule.  The device plan is compared with these mirrors in
tests/test_solve_hints.py."""
import os
import re

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R

SENTINEL = 0xA5A5A5A5A5A5A5A5
NBITS, MAX_COUNT, CF_COUNT = 8, 3, 4


def running_max_inputs(prm, count, nbits=NBITS, seed=31):
    """x_0 .. x_count [count + 1][N]: integers below 2^(nbits-1), ties and a descending run included"""
    rng = np.random.RandomState(seed)
    xs = rng.randint(0, 1 << (nbits - 1), (count + 1, prm.N)).astype(np.uint64)
    xs[:, 0] = np.arange(count + 1, 0, -1)  # the first stays the maximum
    xs[:, 1] = 5  # ties
    xs[:, 2] = np.arange(count + 1)  # every stage replaces it
    xs[0, 3], xs[1, 3] = 0, (1 << (nbits - 1)) - 1  # the extreme difference
    return xs


def running_max_assignment(prm, cs, xs):
    """`one` and the inputs in every limb, a sentinel everywhere else; the given variables"""
    asg = np.full((cs.n_vars, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    asg[0] = 1
    asg[1:1 + xs.shape[0]] = xs[:, None, :]
    return asg, list(range(1 + xs.shape[0]))


def continued_fraction_assignment(prm, cs, count, seed=37):
    """`one`, y_0 and the c_j, d_j as random non-zero residues; the given variables"""
    rng = np.random.RandomState(seed)
    asg = np.full((cs.n_vars, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    asg[0] = 1
    for v in range(1, 2 + 2 * count):
        asg[v] = np.stack([rng.randint(1, int(p), prm.N, dtype=np.int64).astype(np.uint64) for p in prm.q])
    return asg, list(range(2 + 2 * count))


def test_library_exports_the_hinted_solver():
    from ringsnark_amd import _lib
    lib = _lib.load()
    names = {"rs_r1cs_hint_plan_create", "rs_r1cs_hint_plan_steps", "rs_r1cs_hint_plan_destroy", "rs_r1cs_solve_hinted"}
    assert names == set(_lib.HINT_SIGNATURES) and all(hasattr(lib, n) for n in names)
    assert lib.rs_version() >= 114
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ringsnark_amd", "solve_hints.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code)) == names
    assert "hint" not in open(os.path.join(root, "include", "ringsnark_amd.h")).read()
    assert (_lib.RS_HINT_BITS, _lib.RS_HINT_INV, _lib.RS_HINT_QUOT) == (R.RS_HINT_BITS, R.RS_HINT_INV, R.RS_HINT_QUOT) == (1, 2, 3)
    for k, v in ((1, "BITS"), (2, "INV"), (3, "QUOT")):
        assert re.search(r"#define RS_HINT_%s %d\b" % (v, k), hdr)


@pytest.mark.parametrize("make,given", [(lambda q: R.chain_r1cs(5, q), [0, 1]), (lambda q: R.wide_r1cs(16, q), [0, 1]),
                                        (lambda q: R.logreg_r1cs(q, 4), list(range(16))), (lambda q: R.logreg_r1cs(q, 4), list(range(15)))])
def test_no_hints_is_the_plain_schedule(make, given):
    q = P.preset("toy").q
    cs = make(q)
    steps, lp, info = R.solve_schedule(cs, given, q)
    hsteps, hlp, hinfo = R.solve_hinted_schedule(cs, given, [], q)
    assert hsteps == [(0, j, t) for j, t in steps] and hlp == lp
    for f in ("n_given", "n_solved", "n_unsolved", "first_unsolved", "n_levels", "max_width", "n_unused", "first_blocked", "blocked_reason"):
        assert getattr(hinfo, f) == getattr(info, f), f
    assert (hinfo.n_steps, hinfo.n_hints_run, hinfo.n_hints_blocked, hinfo.first_blocked_hint) == (len(steps), 0, 0, 0)


def test_running_max_needs_and_takes_its_hints():
    prm = P.preset("toy")
    cs, hints = R.running_max_r1cs(prm.q, NBITS, MAX_COUNT)
    xs = running_max_inputs(prm, MAX_COUNT)
    asg, given = running_max_assignment(prm, cs, xs)
    plain = R.solve_schedule(cs, given, prm.q)[2]
    assert (plain.n_solved, plain.blocked_reason) == (1, 1)  # the gap: s_0, then the packing constraint's a side waits for nothing
    steps, lp, info = R.solve_hinted_schedule(cs, given, hints, prm.q)
    assert info.n_unsolved == 0 and info.n_levels == 3 * MAX_COUNT == 9 and lp == list(range(10))
    assert [k for k, _, _ in steps] == [0, 1, 0] * MAX_COUNT and info.max_width == 1
    assert info.n_solved == MAX_COUNT * (NBITS + 2) and info.n_steps == 9 and info.n_unused == cs.m - 2 * MAX_COUNT
    assert (info.n_hints_run, info.n_hints_blocked, info.first_blocked_hint, info.blocked_reason) == (3, 0, 3, 0)
    lay = R.running_max_layout(NBITS, MAX_COUNT)
    assert [(k, w) for k, _, w in steps] == [x for s, b, m in lay for x in ((0, s), (1, b), (0, m))]
    out, rep = R.solve_hinted(cs, given, hints, asg, prm.q)
    assert rep.clean and tuple(rep) == (0,) * 8
    assert R.is_satisfied(cs, out, prm.q).satisfied
    running = np.maximum.accumulate(xs, axis=0)
    for j, (_, _, m) in enumerate(lay):
        assert (out[m] == running[j + 1][None, :]).all()
    assert not (out == SENTINEL).any()


def test_continued_fraction_needs_and_takes_its_hints():
    prm = P.preset("toy")
    cs, hints = R.continued_fraction_r1cs(prm.q, CF_COUNT)
    asg, given = continued_fraction_assignment(prm, cs, CF_COUNT)
    plain = R.solve_schedule(cs, given, prm.q)[2]
    assert (plain.n_solved, plain.blocked_reason) == (1, 1)
    steps, lp, info = R.solve_hinted_schedule(cs, given, hints, prm.q)
    assert info.n_unsolved == 0 and info.n_levels == 2 * CF_COUNT == 8 and info.n_solved == 8
    assert steps == [x for j in range(CF_COUNT) for x in ((0, 2 * j, 2 + 2 * CF_COUNT + 2 * j), (1, j, 3 + 2 * CF_COUNT + 2 * j))]
    out, rep = R.solve_hinted(cs, given, hints, asg, prm.q)
    assert R.is_satisfied(cs, out, prm.q).satisfied and rep.n_bits_bad == 0
    # y_{j+1} (y_j + d_j) = c_j, in exact integers
    y = asg[1]
    for j in range(CF_COUNT):
        t = [(y[l].astype(object) + asg[3 + 2 * j][l].astype(object)) % int(p) for l, p in enumerate(prm.q)]
        y = out[3 + 2 * CF_COUNT + 2 * j]
        for l, p in enumerate(prm.q):
            ok = (y[l].astype(object) * t[l] % int(p) == asg[2 + 2 * j][l].astype(object)) | (t[l] == 0)
            assert ok.all()


def one_row(q, a, b, c, n_vars):
    return R.from_rows(1, n_vars, 0, {"a": [a], "b": [b], "c": [c]}, q)


def test_a_packing_constraint_may_not_steal_a_reserved_bit():
    """x * one = b_0 would determine b_0 through its c side in level 1; b_0 is reserved, so the hint determines it"""
    q = P.preset("toy").q
    cs = one_row(q, [(2, 1)], [(1, 1)], [(3, 1)], 3)  # variables: one 0, x 1, b_0 2
    assert R.solve_schedule(cs, [0, 1], q)[0] == [(0, 2)]
    steps, lp, info = R.solve_hinted_schedule(cs, [0, 1], [R.Hint.bits(1, 2, 1)], q)
    assert steps == [(1, 0, 2)] and lp == [0, 1]
    assert (info.n_solved, info.n_unused, info.first_blocked, info.blocked_reason, info.n_hints_run) == (1, 1, 1, 0, 1)


def test_a_hint_with_an_unknown_source_leaves_reason_6():
    q = P.preset("toy").q
    # variables: one 0, x 1, b_0 2, u 3 (never known).  The hint reads u, so b_0 stays reserved and unknown.
    cs = one_row(q, [(2, 1)], [(1, 1)], [(3, 1)], 4)
    steps, lp, info = R.solve_hinted_schedule(cs, [0, 1], [R.Hint.bits(3, 2, 1)], q)
    assert steps == [] and lp == [0]
    assert (info.first_blocked, info.blocked_reason, info.n_hints_run, info.n_hints_blocked, info.first_blocked_hint) == (0, 6, 0, 1, 0)
    assert (info.n_unsolved, info.first_unsolved) == (2, 2) and 6 in R.SOLVE_BLOCKED


def test_a_cycle_across_hints_is_reported_not_refused():
    q = P.preset("toy").q
    cs = one_row(q, [(1, 1)], [(1, 1)], [(2, 1)], 4)  # x0 * x0 = x1; x2 and x3 only in the hints
    hints = [R.Hint.inv(3, 2), R.Hint.inv(2, 3)]
    steps, lp, info = R.solve_hinted_schedule(cs, [0], hints, q)
    assert steps == [(0, 0, 1)]
    assert (info.n_hints_run, info.n_hints_blocked, info.first_blocked_hint, info.n_unsolved) == (0, 2, 0, 2)
    # a hint that is ready runs beside them, and hints chain: x1^-1 -> x2, then x2 / x0 ... -> x3
    steps, lp, info = R.solve_hinted_schedule(cs, [0], [R.Hint.inv(1, 2), R.Hint.quot(2, 0, 3)], q)
    assert steps == [(0, 0, 1), (1, 0, 2), (1, 1, 3)] and lp == [0, 1, 2, 3] and info.n_unsolved == 0


def test_hint_and_constraint_steps_share_a_level_in_order():
    q = P.preset("toy").q
    # x0 * x0 = x1 and inv(x0) -> x2 are both level 1; x1 * x2 = x3 and inv(x1) -> x4 are level 2
    cs = R.from_rows(2, 5, 0, {"a": [[(1, 1)], [(2, 1)]], "b": [[(1, 1)], [(3, 1)]], "c": [[(2, 1)], [(4, 1)]]}, q)
    steps, lp, info = R.solve_hinted_schedule(cs, [0], [R.Hint.inv(1, 4), R.Hint.inv(0, 2)], q)
    assert steps == [(0, 0, 1), (1, 1, 2), (0, 1, 3), (1, 0, 4)] and lp == [0, 2, 4] and info.max_width == 2


REFUSED = {
    "unknown kind": [R.Hint(7, 0, 0, 2)],
    "src out of range": [R.Hint.inv(9, 2)],
    "num out of range": [R.Hint.quot(9, 0, 2)],
    "dst out of range": [R.Hint.inv(0, 9)],
    "last bit row out of range": [R.Hint.bits(0, 3, 2, 2)],
    "nbits 0": [R.Hint.bits(0, 2, 0)],
    "nbits above floor(log2 q)": [R.Hint.bits(0, 2, 30)],
    "dst_stride 0": [R.Hint.bits(0, 2, 2, 0)],
    "a target that is given": [R.Hint.inv(0, 1)],
    "a target named twice across hints": [R.Hint.inv(0, 2), R.Hint.inv(1, 2)],
    "a target named twice across a BITS hint and another": [R.Hint.bits(0, 2, 2), R.Hint.inv(1, 3)],
    "src among the targets": [R.Hint.bits(3, 2, 2)],
    "num among the targets": [R.Hint.quot(2, 0, 2)],
}


@pytest.mark.parametrize("why", sorted(REFUSED))
def test_refusals(why):
    prm = P.preset("toy")
    assert R.max_nbits(prm.q) == 29
    cs = one_row(prm.q, [(1, 1)], [(2, 1)], [(3, 1)], 5)  # variables 0, 1 given
    with pytest.raises(ValueError):
        R.solve_hinted_schedule(cs, [0, 1], REFUSED[why], prm.q)
    # the neighbours that are accepted
    R.solve_hinted_schedule(cs, [0, 1], [R.Hint.bits(0, 3, 2), R.Hint.inv(1, 2)], prm.q)
    R.solve_hinted_schedule(cs, [0, 1], [R.Hint.bits(0, 2, 2, 2)], prm.q)  # targets 2 and 4
    R.solve_hinted_schedule(cs, [0, 1], [R.Hint.bits(0, 2, 1, 29)], prm.q)  # one bit: the stride addresses nothing
