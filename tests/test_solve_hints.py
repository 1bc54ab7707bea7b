"""Solver hints on the device (ringsnark_amd/solve_hints.h): bit, inverse and quotient wires of wires the solver itself
produces, as steps of one plan.

GPU (-m gpu): the device plan equals the host schedule field for field; the hint-level kernel and the walk kernel with inline
hints produce the words of the host mirror ringsnark_amd.r1cs.solve_hinted in every mode and both arithmetics -- exact
equality, no tolerance -- on toy, toy50, toy60 and on C2's ring (16 slot chunks: limb 1 is in other workgroups than limb 0,
which a BITS step must read); the launch counts are those the header promises; bad bits and zero sources are reported where
they were planted and nowhere else.  Rows that are neither given nor solved hold a sentinel before every call."""
import functools

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import test_keygen as TK  # trapdoor, disjoint_seeds, with_r_y: the inputs of the device generators
from tests import helpers as H
from tests import test_solve_hints_host as TH

SENTINEL = TH.SENTINEL
NBITS = TH.NBITS
MODES = ("auto", "levels", "walk")
PRESETS = ("toy", "toy50", "toy60", "C2")


@functools.lru_cache(maxsize=None)
def system(circuit, name):
    """(prm, cs, hints, given, assignment with sentinels, count): built once, read-only.  On C2 two stages, so that the Python
    mirror stays within seconds."""
    prm = P.preset(name)
    if circuit == "max":
        count = 2 if name == "C2" else TH.MAX_COUNT
        cs, hints = R.running_max_r1cs(prm.q, NBITS, count)
        asg, given = TH.running_max_assignment(prm, cs, TH.running_max_inputs(prm, count))
    else:
        count = 2 if name == "C2" else TH.CF_COUNT
        cs, hints = R.continued_fraction_r1cs(prm.q, count)
        asg, given = TH.continued_fraction_assignment(prm, cs, count)
    asg.setflags(write=False)
    return prm, cs, tuple(hints), tuple(given), asg, count


@functools.lru_cache(maxsize=None)
def solved(circuit, name):
    prm, cs, hints, given, asg, _ = system(circuit, name)
    out, rep = R.solve_hinted(cs, given, hints, asg, prm.q)
    out.setflags(write=False)
    return out, rep


def run(dev, plan, asg, mode, **kw):
    from ringsnark_amd.device import to_host
    dasg = dev.put(np.array(asg))  # a copy: the shared assignments are read-only
    stats, rep = dev.r1cs_solve_hinted(plan, dasg, mode=mode, **kw)
    return to_host(dasg), stats, rep, dasg


def expected_stats(circuit, count, mode, chunks):
    """The table of solve_hints.h.  AUTO: every level of both circuits is one step wide, so width x chunks stays below the 256
    workgroups that give a level to the level kernel on every ring used here: the walk's launches."""
    assert chunks < R.SOLVE_FILL_WORKGROUPS
    if circuit == "max":
        return (2 * count, 0, count) if mode == "levels" else (0, count + 1, count)
    return (count, 0, count) if mode == "levels" else (0, 1, 0)


@pytest.mark.gpu
def test_device_plan_equals_the_host_schedule():
    from ringsnark_amd.device import Device
    prm = P.preset("toy")
    dev = Device(prm)
    q = prm.q
    one = lambda a, b, c, n: R.from_rows(1, n, 0, {"a": [a], "b": [b], "c": [c]}, q)
    two = R.from_rows(2, 5, 0, {"a": [[(1, 1)], [(2, 1)]], "b": [[(1, 1)], [(3, 1)]], "c": [[(2, 1)], [(4, 1)]]}, q)
    cases = [system("max", "toy")[1:4], system("cf", "toy")[1:4],
             (R.wide_r1cs(16, q), (), (0, 1)), (R.logreg_r1cs(q, 4), (), tuple(range(15))),
             (one([(2, 1)], [(1, 1)], [(3, 1)], 3), (R.Hint.bits(1, 2, 1),), (0, 1)),  # the reserved bit
             (one([(2, 1)], [(1, 1)], [(3, 1)], 4), (R.Hint.bits(3, 2, 1),), (0, 1)),  # reason 6
             (one([(1, 1)], [(1, 1)], [(2, 1)], 4), (R.Hint.inv(3, 2), R.Hint.inv(2, 3)), (0,)),  # a cycle
             (two, (R.Hint.inv(1, 4), R.Hint.inv(0, 2)), (0,))]  # hint and constraint steps in one level
    for cs, hints, given in cases:
        steps, lp, info = R.solve_hinted_schedule(cs, given, hints, q)
        plan = dev.r1cs_hint_plan(dev.r1cs(cs), given, hints)
        assert plan.info == info, (plan.info, info)
        assert plan.steps() == (steps, lp)
        plan.close()


@pytest.mark.gpu
def test_device_refuses_what_the_mirror_refuses():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    prm = P.preset("toy")
    dev = Device(prm)
    cs = TH.one_row(prm.q, [(1, 1)], [(2, 1)], [(3, 1)], 5)
    dcs = dev.r1cs(cs)
    for why, hints in TH.REFUSED.items():
        with pytest.raises(_lib.RsError) as e:
            dev.r1cs_hint_plan(dcs, [0, 1], hints)
        assert e.value.code == _lib.RS_ERR_INVALID, why
    dev.r1cs_hint_plan(dcs, [0, 1], [R.Hint.bits(0, 3, 2), R.Hint.inv(1, 2)]).close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", PRESETS)
@pytest.mark.parametrize("circuit", ["max", "cf"])
def test_parity_with_the_host_mirror_in_every_mode(circuit, name):
    from ringsnark_amd.device import Device
    prm, cs, hints, given, asg, count = system(circuit, name)
    exp, exp_rep = solved(circuit, name)
    assert exp_rep.clean
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_hint_plan(dcs, given, hints)
    assert plan.info.n_unsolved == 0 and plan.info.n_levels == (3 if circuit == "max" else 2) * count
    chunks = -(-(prm.L * prm.N // 2) // 256)
    assert chunks == (16 if name == "C2" else 1)
    for mode in MODES:
        got, stats, rep, dasg = run(dev, plan, asg, mode)
        assert (got == exp).all(), (mode, np.argwhere(got != exp)[:4])
        assert rep == exp_rep and tuple(rep) == (0,) * 8
        assert dev.r1cs_check(dcs, dasg).satisfied
        assert tuple(stats) == expected_stats(circuit, count, mode, chunks), (mode, stats)
        # enqueue only: the same words
        got2, stats2, rep2, _ = run(dev, plan, asg, mode, want_report=False)
        assert rep2 is None and stats2 == stats and (got2 == exp).all()
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "toy60"])
def test_partial_plan_leaves_the_sentinel(name):
    """without the last stage's hint its bits and its maximum stay unsolved: never read, never written"""
    from ringsnark_amd.device import Device
    prm, cs, hints, given, asg, count = system("max", name)
    hints = hints[:-1]
    exp, _ = R.solve_hinted(cs, given, hints, asg, prm.q)
    s, b, m = R.running_max_layout(NBITS, count)[-1]
    rest = list(range(b, m + 1))
    assert (exp[rest] == SENTINEL).all() and not (exp[: b] == SENTINEL).any()
    dev = Device(prm)
    plan = dev.r1cs_hint_plan(dev.r1cs(cs), given, hints)
    assert (plan.info.n_unsolved, plan.info.first_unsolved, plan.info.blocked_reason) == (NBITS + 1, b, 1)  # a bit constraint: its bit is on the a side
    with pytest.raises(ValueError, match="first unsolved variable %d;" % b):
        dev.r1cs_solve_hinted(plan, dev.put(np.array(asg)))
    for mode in MODES:
        got, _, rep, _ = run(dev, plan, asg, mode, allow_partial=True)
        assert (got == exp).all() and rep.clean


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "toy50", "toy60", "C2"])
def test_a_level_of_many_hints_of_every_kind(name):
    """Seven hints in one level -- more than a workgroup's group, INV, QUOT and BITS mixed, zeros among the sources -- and a
    hint of a hint's target in the next: the hint-level kernel's shared power, and the walk's split at the BITS step."""
    from ringsnark_amd.device import Device
    prm = P.preset(name)
    rng = np.random.RandomState(41)
    cs = R.from_rows(1, 16, 0, {"a": [[(7, 1)]], "b": [[(8, 1)]], "c": [[(15, 1)]]}, prm.q)  # x6 * x7 = x14, both from hints
    hints = [R.Hint.inv(0, 6), R.Hint.inv(1, 7), R.Hint.quot(2, 3, 8), R.Hint.bits(4, 9, 2, 2), R.Hint.inv(5, 10), R.Hint.inv(1, 12),
             R.Hint.quot(0, 0, 13), R.Hint.inv(14, 15)]
    given = list(range(6))
    asg = np.full((16, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    for v in given:
        asg[v] = np.stack([rng.randint(1, int(p), prm.N, dtype=np.int64).astype(np.uint64) for p in prm.q])
    asg[4] = rng.randint(0, 4, prm.N).astype(np.uint64)[None, :]
    asg[1, prm.L - 1, 5] = 0
    asg[0, 0, prm.N - 1] = 0
    asg[3, :, 9] = 0
    steps, lp, info = R.solve_hinted_schedule(cs, given, hints, prm.q)
    assert lp == [0, 7, 8, 9] and info.n_unsolved == 0 and info.max_width == 7
    exp, exp_rep = R.solve_hinted(cs, given, hints, asg, prm.q)
    # x0 has one zero (hints 0 and 6), x1 one (hints 1 and 5), x3 one per limb (hint 2), x14 = x0^-1 x1^-1 two (hint 7); the first: hint 0
    assert exp_rep.n_zero == 6 + prm.L and (exp_rep.zero_hint, exp_rep.zero_limb, exp_rep.zero_slot) == (0, 0, prm.N - 1)
    dev = Device(prm)
    plan = dev.r1cs_hint_plan(dev.r1cs(cs), given, hints)
    assert plan.steps() == (steps, lp)
    for mode in MODES:
        got, stats, rep, _ = run(dev, plan, asg, mode)
        assert (got == exp).all(), (mode, np.argwhere(got != exp)[:4])
        assert rep == exp_rep
        # level 1 holds a BITS step: its hint steps go to the hint-level kernel in every mode; level 2 is one constraint step
        # and level 3 one INV step, which a walk takes inline
        assert tuple(stats) == ((1, 0, 2) if mode == "levels" else (0, 1, 1)), (mode, stats)


@pytest.mark.gpu
def test_no_hints_is_the_plain_solver():
    from ringsnark_amd.device import Device, to_host
    prm = P.preset("toy")
    cs = R.wide_r1cs(64, prm.q)
    asg = np.full((cs.n_vars, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    asg[:2] = H.make_assignment(H.oracle_ctx(prm), cs)[:2]
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plain, plan = dev.r1cs_solve_plan(dcs, [0, 1]), dev.r1cs_hint_plan(dcs, [0, 1], [])
    assert plan.steps() == ([(0, j, t) for j, t in plain.steps()[0]], plain.steps()[1])
    assert plan.info == R.solve_hinted_schedule(cs, [0, 1], [], prm.q)[2]
    for mode in MODES:
        d0 = dev.put(asg.copy())
        s0 = dev.r1cs_solve(plain, d0, mode=mode)
        got, s1, rep, _ = run(dev, plan, asg, mode)
        assert (got == to_host(d0)).all() and not (got == SENTINEL).any()
        assert tuple(s1) == tuple(s0) + (0,) and rep.clean


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "toy60", "C2"])
def test_report_bad_bits(name):
    """s_1 >= 2^nbits at one slot (limb 0 is bad there), and x_2 different between the limbs at another slot (limb 1 is bad
    there): two bad positions of hint 1, the first by limb*N + slot; the low bits are written all the same, and the packing
    constraint of stage 1 fails where the bits do not add up to s_1."""
    from ringsnark_amd.device import Device
    prm, cs, hints, given, asg, count = system("max", name)
    slot_a, slot_b = prm.N - 3, 4
    bad = np.array(asg)
    bad[1, :, slot_a], bad[2, :, slot_a] = 127, 0  # s_0 = 255, m_0 = 127: stage 0 is clean
    # inputs are below 2^(nbits-1) by contract; break it: x_2 = q - 1 = -1, so s_1 = 127 + 1 + 128 = 256 = 2^nbits in every limb
    for l, p in enumerate(prm.q):
        bad[3, l, slot_a] = int(p) - 1
    bad[1, :, slot_b], bad[2, :, slot_b] = 90, 20
    bad[3, 0, slot_b], bad[3, prm.L - 1, slot_b] = 30, 31  # m_0 = 90 > x_2 in both limbs: m_1 = 90 in both, stage 2 is clean
    exp, exp_rep = R.solve_hinted(cs, given, hints, bad, prm.q)
    s1 = R.running_max_layout(NBITS, count)[1][0]
    assert exp[s1, 0, slot_a] == 256 and exp[s1, prm.L - 1, slot_b] == exp[s1, 0, slot_b] - 1
    assert tuple(exp_rep) == (2, 1, 0, slot_a, 0, 0, 0, 0)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_hint_plan(dcs, given, hints)
    packing = (NBITS + 3) + NBITS + 1
    for mode in MODES:
        got, _, rep, dasg = run(dev, plan, bad, mode)
        assert (got == exp).all() and rep == exp_rep
        chk = dev.r1cs_check(dcs, dasg)
        assert (chk.first_row, chk.first_limb, chk.first_slot) == (packing, 0, slot_a)
        assert (chk.a, chk.c) == (256, 0)  # s_1 against its low eight bits
        flags = dev.r1cs_check(dcs, dasg, want_flags=True).flags.cpu().numpy()
        assert flags[packing] == 1 and not flags[:packing].any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "toy60", "C2"])
def test_report_zero_sources(name):
    """d_0 = q - y_0 and c_0 = 0 at one position: t_0 is zero there, y_1 is 0, and y_1 t_0 = c_0 still holds"""
    from ringsnark_amd.device import Device
    prm, cs, hints, given, asg, count = system("cf", name)
    limb, slot = prm.L - 1, prm.N - 2
    z = np.array(asg)
    z[3, limb, slot] = int(prm.q[limb]) - int(z[1, limb, slot])
    z[2, limb, slot] = 0
    exp, exp_rep = R.solve_hinted(cs, given, hints, z, prm.q)
    assert tuple(exp_rep) == (0, 0, 0, 0, 1, 0, limb, slot)
    assert exp[2 + 2 * count, limb, slot] == 0 and exp[3 + 2 * count, limb, slot] == 0
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_hint_plan(dcs, given, hints)
    for mode in MODES:  # levels: the hint-level kernel sees the zero; walk: the inline step does
        got, _, rep, dasg = run(dev, plan, z, mode)
        assert (got == exp).all() and rep == exp_rep and rep.n_zero == 1
        assert dev.r1cs_check(dcs, dasg).satisfied


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["rinocchio", "groth16"])
def test_running_max_end_to_end(scheme):
    from ringsnark_amd.device import Device, to_host
    prm, cs, hints, given, asg, count = system("max", "toy")
    exp, _ = solved("max", "toy")
    ctx = H.oracle_ctx(prm)
    vk = TK.with_r_y(scheme, TK.trapdoor(scheme, prm, cs.m, 53, ctx.keygen(5)), prm.q)
    seeds = TK.disjoint_seeds(1900, len(TK.VECTORS[scheme]))
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    plan = dev.r1cs_hint_plan(dcs, given, hints)
    dasg = dev.put(np.array(asg))
    _, rep = dev.r1cs_solve_hinted(plan, dasg)
    assert rep.clean and (to_host(dasg) == exp).all()
    if scheme == "rinocchio":
        pk, dvk, prove, verify = dev.rinocchio_keygen(dcs, vk, seeds=seeds), dev.rinocchio_vk(dcs, vk), dev.rinocchio_prove, dev.rinocchio_verify
    else:
        pk, dvk, prove, verify = dev.groth16_keygen(dcs, vk, seeds=seeds), dev.groth16_vk(dcs, vk), dev.groth16_prove, dev.groth16_verify
    proof, empty = prove(dcs, pk, dasg, check=True)
    assert verify(dvk, dasg[: cs.n_inputs].contiguous(), proof, empty).accepted
    host_proof, host_empty = prove(dcs, pk, dev.put(np.array(exp)), check=True)
    assert empty == host_empty and (to_host(proof) == to_host(host_proof)).all()
