"""The range check by bit decomposition (ringsnark_amd.r1cs.plaintext_check_r1cs): the circuit of the reference's
examples/example_plaintext_check_SEAL.cpp and benchmarks/bench_plaintext_check_SEAL.cpp, in the reference's form and in the
form without constants that its verifier accepts, and the whole device pipeline on it -- upload x, make the bits on the
device (rs_ring_bit_decompose) inside the assignment, check, generate, prove, verify.

CPU (-m "not gpu"): the generator against rows written out by hand; the host assignment satisfies it; the constant-free
form passes the reference's flow (tests/snark_ref.py's Rinocchio generator, the oracle prover, snark_ref's verifier) with a
positive noise budget in every proof element; the reference's own form is satisfied and REJECTED, in exactly the two checks
that the double count of the constant one reaches (r1cs_to_qrp.tcc:175-201).
GPU (-m gpu): the proof of the device-made assignment equals, word for word, the proof of the host mirror's assignment on
the same key, and is accepted; an x that does not fit is named by the decomposition's report, by rs_r1cs_check and by the
provers' check."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests import snark_ref as S
from tests import test_keygen as TK  # trapdoor, disjoint_seeds, with_r_y: the inputs of the device generators

LOGT, COUNT = 8, 3
SENTINEL = 0xA5A5A5A5A5A5A5A5


def values(prm, count, logT, seed):
    """[count][L][N]: one integer below 2^logT per slot, the same word in every limb; 0 and 2^logT - 1 among them."""
    rng = np.random.RandomState(seed)
    v = rng.randint(0, 1 << logT, size=(count, prm.N), dtype=np.uint64)
    v[0, 0], v[0, 1], v[count - 1, prm.N - 1] = 0, (1 << logT) - 1, (1 << logT) - 1
    return np.ascontiguousarray(np.repeat(v[:, None, :], prm.L, axis=1))


def rows_of(cs, q):
    """{name: [[(index, coefficient mod q_0), ...] per row]} and, per limb, the same with that limb's residues checked"""
    out = {}
    for name in "abc":
        rp, col, coeff = cs.mats[name]
        out[name] = [[(int(col[e]), int(coeff[0, e])) for e in range(int(rp[i]), int(rp[i + 1]))] for i in range(cs.m)]
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_generator_against_rows_written_by_hand():
    q = P.preset("toy").q
    p0 = q[0]
    # logT = 3, count = 2, without constants: variable 1 = one; block 0 = b 2,3,4 and x 5; block 1 = b 6,7,8 and x 9
    cs = R.plaintext_check_r1cs(q, 3, 2)
    assert (cs.m, cs.n_vars, cs.n_inputs) == (8, 9, 1)
    assert cs.poly_table is None
    assert rows_of(cs, q) == {
        "a": [[(2, 1)], [(3, 1)], [(4, 1)], [(5, 1)], [(6, 1)], [(7, 1)], [(8, 1)], [(9, 1)]],
        "b": [[(1, 1), (2, p0 - 1)], [(1, 1), (3, p0 - 1)], [(1, 1), (4, p0 - 1)], [(1, 1)],
              [(1, 1), (6, p0 - 1)], [(1, 1), (7, p0 - 1)], [(1, 1), (8, p0 - 1)], [(1, 1)]],
        "c": [[], [], [], [(2, 1), (3, 2), (4, 4)], [], [], [], [(6, 1), (7, 2), (8, 4)]],
    }
    # the reference's file: the constant one (index 0) where `one` stood; block 0 = b 1,2,3 and x 4; block 1 = b 5,6,7 and x 8
    ref = R.plaintext_check_r1cs(q, 3, 2, constants=True)
    assert (ref.m, ref.n_vars, ref.n_inputs) == (8, 8, 1)
    assert rows_of(ref, q) == {
        "a": [[(1, 1)], [(2, 1)], [(3, 1)], [(4, 1)], [(5, 1)], [(6, 1)], [(7, 1)], [(8, 1)]],
        "b": [[(0, 1), (1, p0 - 1)], [(0, 1), (2, p0 - 1)], [(0, 1), (3, p0 - 1)], [(0, 1)],
              [(0, 1), (5, p0 - 1)], [(0, 1), (6, p0 - 1)], [(0, 1), (7, p0 - 1)], [(0, 1)]],
        "c": [[], [], [], [(1, 1), (2, 2), (3, 4)], [], [], [], [(5, 1), (6, 2), (7, 4)]],
    }
    assert R.plaintext_check_r1cs(q, 3, 1, constants=True, n_inputs=3).n_inputs == 3  # the benchmark: everything but x public
    # every limb holds its own residue of -1, and 2^i is the true power: 2^31 mod q_l at i = 31, not `1 << 31` in int
    for l, p in enumerate(q):
        assert int(cs.mats["b"][2][l, 1]) == p - 1
    big = R.plaintext_check_r1cs(P.preset("toy49").q, 32, 1)
    assert (big.m, big.n_vars) == (33, 34)
    assert [int(c) for c in big.mats["c"][2][0]] == [1 << i for i in range(32)]


@pytest.mark.parametrize("constants", [False, True])
def test_the_host_assignment_satisfies_the_circuit(constants):
    prm = P.preset("toy")
    cs = R.plaintext_check_r1cs(prm.q, LOGT, COUNT, constants=constants)
    xs = values(prm, COUNT, LOGT, 3)
    asg = R.plaintext_check_assignment(cs, xs, prm.q)
    assert asg.shape == (cs.n_vars, prm.L, prm.N)
    assert (asg == R.plaintext_check_assignment(LOGT, xs, prm.q, constants=constants)).all()
    logT, first = R.plaintext_check_layout(cs, COUNT)
    assert (logT, first) == (LOGT, 0 if constants else 1)
    assert (asg[:first] == 1).all()
    assert (asg[first:].reshape(COUNT, LOGT + 1, prm.L, prm.N)[:, LOGT] == xs).all()
    assert R.is_satisfied(cs, asg, prm.q).satisfied
    bad = asg.copy()
    bad[first + LOGT + 1 + 2, 1, 4] ^= 1  # bit 2 of block 1, limb 1, slot 4: its own constraint holds (0 <-> 1), the packing fails
    r = R.is_satisfied(cs, bad, prm.q)
    assert (r.n_violated, r.first_row, r.first_limb, r.first_slot) == (1, 2 * (LOGT + 1) - 1, 1, 4)
    bad[first + LOGT + 1 + 2, 1, 4] = 2  # not a bit
    r = R.is_satisfied(cs, bad, prm.q)
    assert (r.n_violated, r.first_row, r.first_limb, r.first_slot) == (2, LOGT + 1 + 2, 1, 4)


@functools.lru_cache(maxsize=None)
def reference_flow(name, constants):
    """snark_ref's Rinocchio generator, the oracle prover, the decodings: computed once"""
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    cs = R.plaintext_check_r1cs(prm.q, LOGT, COUNT, constants=constants)
    asg = R.plaintext_check_assignment(cs, values(prm, COUNT, LOGT, 5), prm.q)
    pk, vk = S.rinocchio_generator(ctx, cs, 31, ctx.enc_encode)
    proof, empty = O.rinocchio_prove(ctx, H.oracle_cs(cs), pk, asg, None, None, None)
    return dict(prm=prm, ctx=ctx, cs=cs, asg=asg, vk=vk, proof=proof, empty=empty)


@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "toy60"])
def test_the_form_without_constants_passes_the_reference_flow(name):
    c = reference_flow(name, False)
    ctx, vk, cs = c["ctx"], c["vk"], c["cs"]
    assert R.is_satisfied(cs, c["asg"], c["prm"].q).satisfied
    assert c["empty"] == [0] * 9
    budgets = [min(ctx.noise_budget(vk["sk"], c["proof"][k])) for k in range(9)]
    print("min noise budget per proof element:", budgets)
    assert min(budgets) > 0, budgets
    dec = [ctx.enc_decode(vk["sk"], c["proof"][k]) for k in range(9)]
    ok, checks = S.rinocchio_verifier(ctx, cs, vk, c["asg"][: cs.n_inputs], dec)
    assert ok, checks


def test_the_reference_form_is_satisfied_and_rejected_by_the_reference_verifier():
    """Why constants=False is the default: the witness map counts the terms on the constant one twice."""
    c = reference_flow("toy", True)
    ctx, vk, cs = c["ctx"], c["vk"], c["cs"]
    assert R.is_satisfied(cs, c["asg"], c["prm"].q).satisfied
    for k in range(9):
        if not c["empty"][k]:
            assert min(ctx.noise_budget(vk["sk"], c["proof"][k])) > 0
    zero = np.zeros(ctx.ring_shape(), dtype=np.uint64)
    dec = [zero if c["empty"][k] else ctx.enc_decode(vk["sk"], c["proof"][k]) for k in range(9)]
    ok, checks = S.rinocchio_verifier(ctx, cs, vk, c["asg"][: cs.n_inputs], dec)
    assert not ok
    assert {k for k, v in checks.items() if not v} == {"L_beta = L", "P = H Z(s)"}, checks


# ---- GPU -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_case(scheme, name):
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    cs = R.plaintext_check_r1cs(prm.q, LOGT, COUNT)
    xs = values(prm, COUNT, LOGT, 11)
    asg = R.plaintext_check_assignment(cs, xs, prm.q)
    vk = TK.with_r_y(scheme, TK.trapdoor(scheme, prm, cs.m, 47, ctx.keygen(5)), prm.q)
    return dict(prm=prm, cs=cs, xs=xs, asg=asg, vk=vk, seeds=TK.disjoint_seeds(1300, len(TK.VECTORS[scheme])))


def uploaded(dev, cs, xs):
    """The assignment as a caller has it before the bits exist: `one` and the x rows, a sentinel everywhere else."""
    prm = dev.prm
    buf = np.full((cs.n_vars, prm.L, prm.N), SENTINEL, dtype=np.uint64)
    buf[0] = 1
    buf[1:].reshape(COUNT, LOGT + 1, prm.L, prm.N)[:, LOGT] = xs
    return dev.put(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,name", [("rinocchio", "toy"), ("groth16", "toy"), ("rinocchio", "toy50"), ("rinocchio", "toy60")])
def test_device_pipeline_on_device_made_bits(scheme, name):
    from ringsnark_amd.device import Device, to_host
    c = device_case(scheme, name)
    prm, cs, xs, asg, vk = c["prm"], c["cs"], c["xs"], c["asg"], c["vk"]
    dev = Device(prm)
    dcs = dev.r1cs(cs)
    prove = dev.rinocchio_prove if scheme == "rinocchio" else dev.groth16_prove
    dasg = uploaded(dev, cs, xs)
    rep = dev.plaintext_check_fill_bits(dasg, cs, COUNT)
    assert rep and tuple(rep) == (0, 0, 0, 0, 0, 0)
    assert (to_host(dasg) == asg).all()
    assert dev.r1cs_check(dcs, dasg).satisfied
    if scheme == "rinocchio":
        pk = dev.rinocchio_keygen(dcs, vk, seeds=c["seeds"])
        dvk = dev.rinocchio_vk(dcs, vk)
        verify = dev.rinocchio_verify
    else:
        pk = dev.groth16_keygen(dcs, vk, seeds=c["seeds"])
        dvk = dev.groth16_vk(dcs, vk)
        verify = dev.groth16_verify
    proof, empty = prove(dcs, pk, dasg, check=True)
    assert verify(dvk, dasg[: cs.n_inputs].contiguous(), proof, empty).accepted
    host_proof, host_empty = prove(dcs, pk, dev.put(asg), check=True)
    assert empty == host_empty and (to_host(proof) == to_host(host_proof)).all()

    # 2^logT in slot 6 of x_1: it does not fit
    bad_xs = xs.copy()
    bad_xs[1, :, 6] = 1 << LOGT
    dbad = uploaded(dev, cs, bad_xs)
    rep = dev.plaintext_check_fill_bits(dbad, cs, COUNT)
    assert not rep and tuple(rep) == (1, 1, 0, 6, 1 << LOGT, 1 << LOGT)
    chk = dev.r1cs_check(dcs, dbad)
    assert (chk.n_violated, chk.first_row, chk.first_limb, chk.first_slot) == (1, 2 * (LOGT + 1) - 1, 0, 6)
    assert (chk.a, chk.b, chk.c) == (1 << LOGT, 1, 0)  # x * one against the low logT bits
    with pytest.raises(ValueError, match="does not satisfy"):
        prove(dcs, pk, dbad, check=True)
