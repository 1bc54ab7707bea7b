"""Assignment wires held as RingElem SCALARS inside the provers (round-3 verdict, "What's missing" #2).

The reference hands auxiliary_input to EncodingElem::inner_product as it is (zk_proof_systems/groth16/groth16.tcc:108-111,
rinocchio/rinocchio.tcc:176-180).  There (seal/seal_ring.tcc:509-548) a RingElem that is_zero() is skipped (:391-396,
:416), one holding Scalar 1 passes the key element through UNCHANGED (:525-527), any other Scalar is flattened by
to_poly() (:529).  The pass-through is not the product with the batch encoding of all-ones when N_enc > N (the encoding of
a vector that fills half of the slots is not the constant polynomial 1), so the proof BYTES depend on the representation
of the wire although every decryption agrees.  rs_groth16_prove_kinds / rs_rinocchio_prove_kinds take the representation
(RS_KIND_ONE); the CPU tests pin what the oracle does with it, the GPU tests hold the device to the oracle."""
import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H


def _statement(prm, m=12, seed=7):
    ctx = H.oracle_ctx(prm)
    cs = R.wide_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs, seed).copy()
    kinds = np.zeros(cs.n_vars, dtype=np.uint8)
    a0 = cs.n_inputs
    # aux wires 1, 2, 3: RingElem(1), RingElem(0), RingElem(7) -- rows as to_poly() flattens them (all slots = the scalar)
    asg[a0 + 1] = 1
    kinds[a0 + 1] = O.KIND_ONE
    asg[a0 + 2] = 0
    asg[a0 + 3] = 7
    # ... and a POLYNOMIAL wire whose slots all hold 1: not a Scalar, so it is multiplied like any polynomial
    asg[a0 + 5] = 1
    return ctx, cs, np.ascontiguousarray(asg), kinds


def _g16_key(ctx, cs, seed=40):
    return dict(s_pows=ctx.random_enc(seed, cs.m + 1), delta_ts=ctx.random_enc(seed + 1, cs.m + 1),
                delta_mid=ctx.random_enc(seed + 2, cs.n_aux), alpha=ctx.random_enc(seed + 3), beta=ctx.random_enc(seed + 4))


def _rin_key(ctx, cs, seed=50):
    return dict(s_pows=ctx.random_enc(seed, cs.m + 1), alpha_s_pows=ctx.random_enc(seed + 1, cs.m + 1),
                beta_prods=ctx.random_enc(seed + 2, cs.n_aux), beta_rv_ts=ctx.random_enc(seed + 3),
                beta_rw_ts=ctx.random_enc(seed + 4), beta_ry_ts=ctx.random_enc(seed + 5))


def _mod_sub_add(ctx, prm, base, minus, plus):
    """(base - minus + plus) mod Q_j on encoding elements [L][2][K][N_enc]"""
    Q = np.array([int(x) for x in prm.Q], dtype=object).reshape(1, 1, prm.K, 1)
    return ((base.astype(object) - minus.astype(object) + plus.astype(object)) % Q).astype(np.uint64)


def test_oracle_scalar_one_wire_passes_the_key_element_through():
    prm = P.preset("toy")  # N = 32 < N_enc = 64
    ctx, cs, asg, kinds = _statement(prm)
    pk = _g16_key(ctx, cs)
    ocs = H.oracle_cs(cs)
    with_kinds, e1 = O.groth16_prove(ctx, ocs, pk, asg, kinds)
    all_poly, e0 = O.groth16_prove(ctx, ocs, pk, asg)
    assert e0 == e1
    assert (with_kinds[0] == all_poly[0]).all() and (with_kinds[1] == all_poly[1]).all()  # A, B do not read aux
    assert not (with_kinds[2] == all_poly[2]).all()  # C does: the bytes differ ...
    # ... by exactly the one term: delta_mid[1] itself instead of delta_mid[1] * encode(all-ones)
    t = 1
    times_ones, _ = ctx.inner_product(pk["delta_mid"][t:t + 1], asg[cs.n_inputs + t:cs.n_inputs + t + 1])
    assert (with_kinds[2] == _mod_sub_add(ctx, prm, all_poly[2], times_ones, pk["delta_mid"][t])).all()
    # Rinocchio: only F reads the auxiliary input (rinocchio.tcc:176-180)
    rk = _rin_key(ctx, cs)
    ds = [ctx.random_ring(60 + k) for k in range(3)]
    for zk in (False, True):
        d = ds if zk else [None] * 3
        pr1, _ = O.rinocchio_prove(ctx, ocs, rk, asg, *d, kinds=kinds)
        pr0, _ = O.rinocchio_prove(ctx, ocs, rk, asg, *d)
        assert (pr1[:8] == pr0[:8]).all() and not (pr1[8] == pr0[8]).all()
        times_ones, _ = ctx.inner_product(rk["beta_prods"][t:t + 1], asg[cs.n_inputs + t:cs.n_inputs + t + 1])
        assert (pr1[8] == _mod_sub_add(ctx, prm, pr0[8], times_ones, rk["beta_prods"][t])).all()


def test_oracle_scalar_one_is_invisible_when_the_encoding_degree_equals_the_ring_degree():
    """N_enc == N: the batch encoding of all-ones IS the constant polynomial 1, whose transform is all-ones, so the
    product equals the pass-through and the representation cannot change a byte."""
    prm = P.make_params(32, [30, 30], 32, [40, 40, 41], ring_factor=1 << 12, name="toy_same_degree")
    ctx, cs, asg, kinds = _statement(prm)
    pk = _g16_key(ctx, cs)
    a, _ = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg, kinds)
    b, _ = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
    assert (a == b).all()


def test_oracle_scalar_one_decrypts_like_the_polynomial_wire():
    """Real encryptions: the two representations give different ciphertexts of the SAME ring element."""
    prm = P.preset("toy")
    ctx, cs, asg, kinds = _statement(prm)
    sk = ctx.keygen(3)
    rings = ctx.random_ring(77, cs.n_aux)
    key = ctx.enc_encode(sk, rings, 5)
    aux = asg[cs.n_inputs:]
    ip1, _ = ctx.inner_product(key, aux, kinds[cs.n_inputs:])
    ip0, _ = ctx.inner_product(key, aux, None)
    assert not (ip1 == ip0).all()
    assert (ctx.enc_decode(sk, ip1) == ctx.enc_decode(sk, ip0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "toy60", "C2"])
def test_device_provers_honour_scalar_one_wires(name):
    from ringsnark_amd.device import Device, to_host
    prm = P.preset(name)
    m = 12 if prm.N_enc <= 128 else 6
    ctx, cs, asg, kinds = _statement(prm, m)
    dev = Device(prm)
    dcs, dasg = dev.r1cs(cs), dev.put(asg)
    ocs = H.oracle_cs(cs)
    pk = _g16_key(ctx, cs)
    dpk = {k: dev.put(v) for k, v in pk.items()}
    exp, exp_empty = O.groth16_prove(ctx, ocs, pk, asg, kinds)
    got, empty = dev.groth16_prove(dcs, dpk, dasg, kinds=kinds)
    assert empty == exp_empty and (to_host(got) == exp).all()
    plain, _ = dev.groth16_prove(dcs, dpk, dasg)
    exp0, _ = O.groth16_prove(ctx, ocs, pk, asg)
    assert (to_host(plain) == exp0).all() and not (exp0[2] == exp[2]).all()
    rk = _rin_key(ctx, cs)
    drk = {k: dev.put(v) for k, v in rk.items()}
    ds = [ctx.random_ring(60 + k) for k in range(3)]
    for zk in (False, True):
        d = ds if zk else [None] * 3
        exp, exp_empty = O.rinocchio_prove(ctx, ocs, rk, asg, *d, kinds=kinds)
        got, empty = dev.rinocchio_prove(dcs, drk, dasg, *[None if x is None else dev.put(x) for x in d], kinds=kinds)
        assert empty == exp_empty and (to_host(got) == exp).all(), zk


@pytest.mark.gpu
def test_device_prover_with_a_windowed_key_and_every_aux_wire_a_scalar_one():
    """All auxiliary wires Scalar 1 on a tiled key: <delta_mid, aux> is the plain sum of the key elements."""
    from ringsnark_amd.device import Device, to_host
    prm = P.preset("toy")
    ctx = H.oracle_ctx(prm)
    m = 40
    cs = R.wide_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs).copy()
    asg[cs.n_inputs:] = 1
    kinds = np.zeros(cs.n_vars, dtype=np.uint8)
    kinds[cs.n_inputs:] = O.KIND_ONE
    W = 8
    pkw = dict(s_pows=ctx.random_enc(1, W), delta_ts=ctx.random_enc(2, W), delta_mid=ctx.random_enc(3, W), alpha=ctx.random_enc(4),
               beta=ctx.random_enc(5))
    tile = lambda a, T: np.concatenate([a] * (-(-T // W)))[:T]
    pk = dict(pkw, s_pows=tile(pkw["s_pows"], m + 1), delta_ts=tile(pkw["delta_ts"], m + 1), delta_mid=tile(pkw["delta_mid"], cs.n_aux))
    exp, exp_empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg, kinds)
    dev = Device(prm)
    got, empty = dev.groth16_prove(dev.r1cs(cs), {k: dev.put(v) for k, v in pkw.items()}, dev.put(asg), window=W, kinds=kinds)
    assert empty == exp_empty and (to_host(got) == exp).all()
