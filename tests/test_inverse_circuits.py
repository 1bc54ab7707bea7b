"""The is-zero and the division circuits (ringsnark_amd.r1cs.is_zero_r1cs, division_r1cs) through the whole device
pipeline: upload `one` and the inputs, make the inverse-or-zero and quotient wires on the device inside the assignment
(rs_ring_inv_or_zero), let the unchanged solver find what is left, check, generate, prove, verify.

GPU (-m gpu): the device-made assignment equals the host mirror's word for word, its proof equals the proof of the host
assignment on the same key and is accepted; a divisor with a zero slot is named by the report, by rs_r1cs_check and by the
provers' check; a forged zero indicator fails the check where it was forged."""
import functools

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests import test_keygen as TK  # trapdoor, disjoint_seeds, with_r_y: the inputs of the device generators

COUNT = 3
SENTINEL = 0xA5A5A5A5A5A5A5A5
CASES = [("rinocchio", "toy"), ("groth16", "toy"), ("rinocchio", "toy50"), ("rinocchio", "toy60")]


def inputs(prm, seed, zeros):
    """[COUNT][L][N] canonical residues; zeros: some slots of elements 0 and 2 are zero, in one limb or in all"""
    rng = np.random.RandomState(seed)
    x = np.stack([rng.randint(1, p, size=(COUNT, prm.N), dtype=np.uint64) for p in prm.q], axis=1)
    if zeros:
        x[0, 0, 0] = 0
        x[0, :, 7] = 0
        x[2, prm.L - 1, prm.N - 1] = 0
        x[2, :, 1::2] = 0
    return np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def case(scheme, name, circuit):
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    cs = (R.is_zero_r1cs if circuit == "is_zero" else R.division_r1cs)(prm.q, COUNT)
    vk = TK.with_r_y(scheme, TK.trapdoor(scheme, prm, cs.m, 53, ctx.keygen(5)), prm.q)
    return dict(prm=prm, cs=cs, vk=vk, seeds=TK.disjoint_seeds(1700, len(TK.VECTORS[scheme])))


def flow(dev, scheme, c, dcs):
    if scheme == "rinocchio":
        return dev.rinocchio_keygen(dcs, c["vk"], seeds=c["seeds"]), dev.rinocchio_vk(dcs, c["vk"]), dev.rinocchio_prove, dev.rinocchio_verify
    return dev.groth16_keygen(dcs, c["vk"], seeds=c["seeds"]), dev.groth16_vk(dcs, c["vk"]), dev.groth16_prove, dev.groth16_verify


def uploaded(dev, cs, width, rows):
    """The assignment as a caller has it before the hint wires exist: `one` and the input rows {row of a block: values},
    a sentinel everywhere else."""
    prm = dev.prm
    buf = np.full((cs.n_vars, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    buf[0] = 1
    for r, v in rows.items():
        buf[1 + r::width] = v
    return dev.put(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,name", CASES)
def test_is_zero_pipeline_on_device_made_inverses(scheme, name):
    from ringsnark_amd.device import Device, to_host
    c = case(scheme, name, "is_zero")
    prm, cs = c["prm"], c["cs"]
    xs = inputs(prm, 21, zeros=True)
    asg = R.is_zero_assignment(xs, prm.q)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    dasg = uploaded(dev, cs, 3, {0: xs})
    rep = dev.is_zero_fill(dasg, COUNT)
    zero = xs == 0
    assert rep.clean and rep.n_zero == int(zero.sum()) and (rep.zero_elem, rep.zero_limb, rep.zero_slot) == (0, 0, 0)
    given = [0] + [1 + 3 * p for p in range(COUNT)] + [2 + 3 * p for p in range(COUNT)]
    plan = dev.r1cs_solve_plan(dcs, given)
    assert plan.info.n_unsolved == 0 and plan.info.n_solved == COUNT
    dev.r1cs_solve(plan, dasg)
    plan.close()
    assert (to_host(dasg) == asg).all()
    assert dev.r1cs_check(dcs, dasg).satisfied
    pk, dvk, prove, verify = flow(dev, scheme, c, dcs)
    proof, empty = prove(dcs, pk, dasg, check=True)
    assert verify(dvk, dasg[: cs.n_inputs].contiguous(), proof, empty).accepted
    host_proof, host_empty = prove(dcs, pk, dev.put(asg), check=True)
    assert empty == host_empty and (to_host(proof) == to_host(host_proof)).all()

    # z forged to 0 at a zero slot of x_2: x * inv = 0 there, one - z = 1
    limb, slot = prm.L - 1, prm.N - 1
    assert xs[2, limb, slot] == 0
    dasg[3 + 3 * 2, limb, slot] = 0
    chk = dev.r1cs_check(dcs, dasg)
    assert (chk.n_violated, chk.first_row, chk.first_limb, chk.first_slot) == (1, 2 * 2, limb, slot)
    assert (chk.a, chk.b, chk.c) == (0, 0, 1)
    with pytest.raises(ValueError, match="does not satisfy"):
        prove(dcs, pk, dasg, check=True)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,name", CASES)
def test_division_pipeline_on_device_made_quotients(scheme, name):
    from ringsnark_amd.device import Device, to_host
    c = case(scheme, name, "division")
    prm, cs = c["prm"], c["cs"]
    a, b = inputs(prm, 22, zeros=True), inputs(prm, 23, zeros=False)
    asg = R.division_assignment(a, b, prm.q)
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    dasg = uploaded(dev, cs, 4, {0: a, 1: b})
    rep_binv, rep_y = dev.division_fill(dasg, COUNT)
    assert tuple(rep_binv) == tuple(rep_y) == (0,) * 10
    plan = dev.r1cs_solve_plan(dcs, range(cs.n_vars))  # every wire is there: nothing to solve
    assert plan.info.n_unsolved == 0 and plan.info.n_solved == 0
    plan.close()
    assert (to_host(dasg) == asg).all()
    assert dev.r1cs_check(dcs, dasg).satisfied
    pk, dvk, prove, verify = flow(dev, scheme, c, dcs)
    proof, empty = prove(dcs, pk, dasg, check=True)
    assert verify(dvk, dasg[: cs.n_inputs].contiguous(), proof, empty).accepted
    host_proof, host_empty = prove(dcs, pk, dev.put(asg), check=True)
    assert empty == host_empty and (to_host(proof) == to_host(host_proof)).all()

    # b_1 with a zero slot (a_1 zero there as well, so that y * b = a still holds): no binv exists
    limb, slot = prm.L - 1, 6
    bad_a, bad_b = a.copy(), b.copy()
    bad_a[1, limb, slot] = bad_b[1, limb, slot] = 0
    dbad = uploaded(dev, cs, 4, {0: bad_a, 1: bad_b})
    rep_binv, rep_y = dev.division_fill(dbad, COUNT)
    assert tuple(rep_binv) == tuple(rep_y) == (1, 1, limb, slot) + (0,) * 6
    assert (to_host(dbad) == R.division_assignment(bad_a, bad_b, prm.q)).all()
    chk = dev.r1cs_check(dcs, dbad)
    assert (chk.n_violated, chk.first_row, chk.first_limb, chk.first_slot) == (1, 2 * 1, limb, slot)
    assert (chk.a, chk.b, chk.c) == (0, 0, 1)  # b * binv against one
    with pytest.raises(ValueError, match="does not satisfy"):
        prove(dcs, pk, dbad, check=True)
