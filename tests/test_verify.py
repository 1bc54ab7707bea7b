"""ringsnark_amd/verify.h: the public columns of the instance map at a point (rs_io_eval_at) and the two verifiers
(groth16.tcc:117-170, rinocchio.tcc:192-295) on the device.

Everything is exact: the device's residues are compared for equality, with rs_instance_map_eval (rows 0..n_inputs), with the
O(m^2) restatement of tests/snark_ref.py, and -- for a report -- with the lhs / rhs arrays the CPU computes from
snark_ref's ring operations the reference's way (evaluate on `primary || zeros`, interpolate, Horner at s).

The inputs of the GPU accept / reject tests are shown valid on the CPU alone (test_gpu_inputs_are_valid_by_the_reference):
keys from snark_ref's generators, the oracle's prover, positive noise budget everywhere, accepted by snark_ref's verifier.
Rinocchio with the ZK elements d1..d3 set multiplies every term of <s_pows, .> by TWO plaintexts (the coefficient of Z and
d_i, rinocchio.tcc:150-160): on `toy49` (and the integer presets `toy54`, `toy60`) that spends the whole budget of V..Y' --
the reference's verifier throws on such a proof -- so the ZK case runs on `toy`, whose 30-bit plain moduli leave 26 bits,
and `toy49` / `toy50` / `toy60` run without ZK elements."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests import snark_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 64  # rows per tile of rs_io_eval_at (ringsnark_amd.device.IO_EVAL_TILE)

G16_CASES = [("toy", 6), ("toy49", 12), ("toy50", 12), ("toy60", 6)]  # toy60: the integer (Montgomery) arithmetic
RIN_CASES = [("toy49", 9, False), ("toy50", 9, False), ("toy", 9, True), ("toy60", 9, False)]  # (preset, m, ZK elements set)


# ---- shared inputs (CPU, computed once) ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def g16_case(name, m):
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk, vk = S.groth16_generator(ctx, cs, 21, ctx.enc_encode)
    proof, empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
    return dict(prm=prm, ctx=ctx, cs=cs, asg=asg, pk=pk, vk=vk, proof=proof, empty=empty)


@functools.lru_cache(maxsize=None)
def rin_case(name, m, zk):
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk, vk = S.rinocchio_generator(ctx, cs, 31, ctx.enc_encode)
    d = ctx.random_ring(77, 3) if zk else [None] * 3
    proof, empty = O.rinocchio_prove(ctx, H.oracle_cs(cs), pk, asg, d[0], d[1], d[2])
    return dict(prm=prm, ctx=ctx, cs=cs, asg=asg, pk=pk, vk=vk, proof=proof, empty=empty, d=d)


def polys_at_s(ctx, cs, s, assignment):
    """A(s), B(s), C(s) of the three polynomials an assignment of all n_vars wires gives: evaluate the constraints on it,
    interpolate, Horner at s."""
    Rg = S.Ring(ctx)
    assert len(assignment) == cs.n_vars
    ocs = H.oracle_cs(cs)
    out = []
    for which in range(3):
        coeffs = np.empty((cs.m,) + ctx.ring_shape(), dtype=np.uint64)
        for limb, q in enumerate(ctx.q):
            ev = O.r1cs_evaluate(q, ocs, which, limb, np.ascontiguousarray(assignment[:, limb, :]))
            coeffs[:, limb, :] = O.interpolate(q, ev)
        out.append(S.poly_eval_ring(Rg, coeffs, s))
    return out


def io_at_s(ctx, cs, s, primary):
    """v_io(s), w_io(s), y_io(s) the reference's way (groth16.tcc:131-154): evaluate the constraints on `primary || zeros`,
    interpolate, Horner at s."""
    padded = np.zeros((cs.n_vars,) + ctx.ring_shape(), dtype=np.uint64)
    padded[: cs.n_inputs] = primary
    return polys_at_s(ctx, cs, s, padded)


def g16_sides(ctx, cs, vk, primary, dec, io=None):
    """[(lhs, rhs)] of groth16.tcc:159-169, in the reference's order of operations (division by gamma included).
    io: io_at_s(ctx, cs, vk["s"], primary), where the caller has it."""
    Rg = S.Ring(ctx)
    v, w, y = io if io is not None else io_at_s(ctx, cs, vk["s"], primary)
    f = Rg.add(Rg.add(Rg.mul(vk["beta"], v), Rg.mul(vk["alpha"], w)), y)
    f = Rg.mul(f, Rg.inv(vk["gamma"]))
    rhs = Rg.add(Rg.add(Rg.mul(vk["alpha"], vk["beta"]), Rg.mul(vk["gamma"], f)), Rg.mul(vk["delta"], dec[2]))
    return [(Rg.mul(dec[0], dec[1]), rhs)]


def rin_sides(ctx, cs, vk, primary, dec, io=None):
    """[(lhs, rhs)] of the six comparisons of rinocchio.tcc:223-293, in verify.h's order.  io: as in g16_sides."""
    Rg = S.Ring(ctx)
    V, Vp, W, Wp, Y, Yp, Hh, Hp, Lb = dec
    v, w, y = io if io is not None else io_at_s(ctx, cs, vk["s"], primary)
    L = Rg.mul(Rg.add(Rg.add(Rg.mul(V, vk["r_v"]), Rg.mul(W, vk["r_w"])), Rg.mul(Y, vk["r_y"])), vk["beta"])
    Pv = Rg.sub(Rg.mul(Rg.add(V, v), Rg.add(W, w)), Rg.add(Y, y))
    return [(Vp, Rg.mul(V, vk["alpha"])), (Wp, Rg.mul(W, vk["alpha"])), (Yp, Rg.mul(Y, vk["alpha"])), (Hp, Rg.mul(Hh, vk["alpha"])),
            (L, Lb), (Pv, Rg.mul(Hh, vk["Zt"]))]


def expected_report(sides, skip=()):
    """The fields of rs_verify_report from the lhs / rhs arrays of every check."""
    n_bad, first = [0] * 6, None
    for c, (lhs, rhs) in enumerate(sides):
        if c in skip:
            continue
        bad = (lhs != rhs).reshape(-1)
        n_bad[c] = int(bad.sum())
        if n_bad[c] and first is None:
            idx = int(np.argmax(bad))
            first = (c, idx // lhs.shape[1], idx % lhs.shape[1], int(lhs.reshape(-1)[idx]), int(rhs.reshape(-1)[idx]))
    failed = sum(1 << c for c in range(6) if n_bad[c])
    return dict(accepted=failed == 0, failed=failed, n_bad=tuple(n_bad), first=first or (0, 0, 0, 0, 0))


def assert_report(got, exp):
    assert bool(got.accepted) == exp["accepted"] and bool(got) == exp["accepted"]
    assert got.failed == exp["failed"], (got, exp)
    assert got.n_bad == exp["n_bad"], (got, exp)
    assert (got.first_check, got.first_limb, got.first_slot, got.lhs, got.rhs) == exp["first"], (got, exp)


def one_slot(ctx, limb, slot, value=1):
    e = np.zeros(ctx.ring_shape(), dtype=np.uint64)
    e[limb, slot] = value
    return e


def hand_rows():
    """n_inputs = 3 of n_vars = 6; entries of all three matrices on the constant one and on the three primary inputs;
    an empty row in `a`; m = 5."""
    a = [[(0, 2), (1, 1), (4, -1)], [], [(2, 3), (3, 1), (5, 2)], [(0, -1), (6, 1)], [(1, 4), (3, -2)]]
    b = [[(0, 1), (2, 3)], [(1, 1), (3, 5)], [(4, 1)], [(0, 7), (2, -1), (5, 1)], [(3, 1)]]
    c = [[(0, 5), (3, 1), (5, 1)], [(1, -3), (6, 1)], [(0, 1), (2, 2)], [(4, 1)], [(1, 1), (2, 1), (3, 1)]]
    return {"a": a, "b": b, "c": c}


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_library_exports_every_function_of_verify_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ringsnark_amd", "verify.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.VERIFY_SIGNATURES) and len(names) == 7
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 103
    # the report structure of the binding has the header's layout: 4 + 4 + 6 * 8 + 3 * 4 (+ 4 padding) + 2 * 8 bytes
    import ctypes as C
    assert C.sizeof(_lib.VerifyReport) == 88 and _lib.VerifyReport.lhs.offset == 72


def test_linearity_identity_is_the_reference_quantity():
    """sum_k x_k A_k(s) (x_0 = 1), with A_k(s) from the instance map with evaluation, equals what the reference's verifiers
    compute by evaluating on `primary || zeros`, interpolating and running Horner at s -- all three matrices, every limb
    and slot -- on a system with entries on the constant one and on three primary inputs in every matrix."""
    prm = P.preset("toy")
    ctx = H.oracle_ctx(prm)
    cs = R.from_rows(5, 6, 3, hand_rows(), prm.q)
    for name in "abc":
        cols = set(int(k) for k in cs.mats[name][1])
        assert {0, 1, 2, 3} <= cols
    Rg = S.Ring(ctx)
    s = Rg.random_exceptional(np.random.RandomState(8), cs.m)
    primary = ctx.random_ring(12, 3)
    At, Bt, Ct, _, _ = S.instance_map_with_evaluation(Rg, cs, s)
    ref = io_at_s(ctx, cs, s, primary)
    for cols, want in zip((At, Bt, Ct), ref):
        acc = cols[0]
        for k in range(cs.n_inputs):
            acc = Rg.add(acc, Rg.mul(primary[k], cols[k + 1]))
        assert (acc == want).all()
        assert want.any()


@pytest.mark.parametrize("name,m", G16_CASES)
def test_gpu_inputs_are_valid_by_the_reference_groth16(name, m):
    """The oracle prover under a snark_ref key: positive noise budget in every limb of every element, accepted by
    snark_ref's verifier.  (toy54 and toy60 both pass this at m = 6; toy60 stands for the integer arithmetic.)"""
    c = g16_case(name, m)
    ctx, vk = c["ctx"], c["vk"]
    assert c["empty"] == [0, 0, 0]
    for k in range(3):
        assert min(ctx.noise_budget(vk["sk"], c["proof"][k])) > 0
    dec = [ctx.enc_decode(vk["sk"], c["proof"][k]) for k in range(3)]
    assert S.groth16_verifier(ctx, c["cs"], vk, c["asg"][: c["cs"].n_inputs], *dec)
    assert expected_report(g16_sides(ctx, c["cs"], vk, c["asg"][: c["cs"].n_inputs], dec))["accepted"]


@pytest.mark.parametrize("name,m,zk", RIN_CASES)
def test_gpu_inputs_are_valid_by_the_reference_rinocchio(name, m, zk):
    c = rin_case(name, m, zk)
    ctx, vk = c["ctx"], c["vk"]
    assert c["empty"] == [0] * 9
    for k in range(9):
        assert min(ctx.noise_budget(vk["sk"], c["proof"][k])) > 0
    dec = [ctx.enc_decode(vk["sk"], c["proof"][k]) for k in range(9)]
    ok, checks = S.rinocchio_verifier(ctx, c["cs"], vk, c["asg"][: c["cs"].n_inputs], dec)
    assert ok, checks
    assert expected_report(rin_sides(ctx, c["cs"], vk, c["asg"][: c["cs"].n_inputs], dec))["accepted"]


def test_zk_elements_spend_the_budget_on_toy49():
    """why RIN_CASES has no ("toy49", 9, True): the reference's own guard refuses that proof"""
    prm = P.preset("toy49")
    ctx = H.oracle_ctx(prm)
    c = rin_case("toy49", 9, False)
    d = ctx.random_ring(77, 3)
    proof, _ = O.rinocchio_prove(ctx, H.oracle_cs(c["cs"]), c["pk"], c["asg"], d[0], d[1], d[2])
    assert max(ctx.noise_budget(c["vk"]["sk"], proof[0])) == 0


# ---- GPU: rs_io_eval_at -------------------------------------------------------------------------------------------------
def io_systems(prm):
    q = prm.q
    out = [("chain%d" % m, R.chain_r1cs(m, q)) for m in (1, 2, 5, TILE - 1, TILE, TILE + 1, 4 * TILE + 7)]
    out.append(("hand", R.from_rows(5, 6, 3, hand_rows(), q)))
    out.append(("wide_poly", R.wide_poly_r1cs(2 * TILE + 3, q, prm.N, constants=True)))  # polynomial coefficients on the constant one and on inputs
    out.append(("wide_inputs", R.wide_r1cs(TILE + 9, q, n_inputs=11)))  # 12 public columns: two column batches; 72 entries per eight rows of `a`
    rows = {"a": [[(1, 1)], [(0, 3), (2, 1)], [(3, 1)]], "b": [[(2, 1)], [(3, 2)], [(0, 1)]], "c": [[(3, 1)], [(4, 1)], [(1, 1), (0, 2)]]}
    out.append(("no_inputs", R.from_rows(3, 4, 0, rows, q)))
    return out


def assert_io_eval_matches_instance_map(dev, cs, s):
    from ringsnark_amd.device import to_host
    dcs = dev.r1cs(cs)
    ds = dev.put(s)
    At, Bt, Ct, _, Zt = dev.instance_map_eval(dcs, ds)
    got = dev.io_eval_at(dcs, ds)
    n1 = cs.n_inputs + 1
    for g, e in zip(got[:3], (At, Bt, Ct)):
        assert tuple(g.shape) == (n1, dev.L, dev.N)
        assert (to_host(g) == to_host(e[:n1])).all()
    assert (to_host(got[3]) == to_host(Zt)).all()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name,force_int", [("toy", 0), ("toy49", 0), ("toy50", 0), ("toy60", 0), ("toy", 1)])
def test_io_eval_at_matches_instance_map_eval(name, force_int):
    """Rows 0..n_inputs of At / Bt / Ct and Zt, bit for bit, on both arithmetics: m around the tile, several tiles with a
    ragged last one (more than one workgroup per slot chunk), an empty row, polynomial coefficients on public columns,
    more public columns than one batch, no inputs at all; with s hitting nodes in some slots; and against the O(m^2)
    restatement at m = 6."""
    from ringsnark_amd import _lib
    from ringsnark_amd import device as D
    assert D.IO_EVAL_TILE == TILE
    prm = P.preset(name)
    with _lib.tuning(force_int_arith=force_int):
        dev = D.Device(prm)
    ctx = H.oracle_ctx(prm)
    Rg = S.Ring(ctx)
    for label, cs in io_systems(prm):
        s = Rg.random_exceptional(np.random.RandomState(4), cs.m)
        assert_io_eval_matches_instance_map(dev, cs, s)
        if cs.m >= 5:  # nodes in some slots (legal: evaluation_domain.tcc:24-39 computes products, never divides)
            hit = s.copy()
            hit[0, 3] = 4
            hit[1 % prm.L, 0] = cs.m - 1
            assert_io_eval_matches_instance_map(dev, cs, hit)
    cs = R.wide_poly_r1cs(6, prm.q, prm.N, constants=True)
    s = Rg.random_exceptional(np.random.RandomState(5), 6)
    s[prm.L - 1, 7] = 2
    got = assert_io_eval_matches_instance_map(dev, cs, s)
    At, Bt, Ct, _, Zt = S.instance_map_with_evaluation(Rg, cs, s)
    for g, e in zip(got[:3], (At, Bt, Ct)):
        assert (D.to_host(g) == np.stack(e[: cs.n_inputs + 1])).all()
    assert (D.to_host(got[3]) == Zt).all()


@pytest.mark.gpu
def test_io_eval_at_refuses_a_domain_element_and_bad_arguments():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device, _ptr
    prm = P.preset("toy")
    dev = Device(prm)
    cs = R.chain_r1cs(TILE + 5, prm.q)
    dcs = dev.r1cs(cs)
    bad = np.full((prm.L, prm.N), 2, dtype=np.uint64)  # RingT(2): a domain element
    with pytest.raises(_lib.RsError) as ei:
        dev.io_eval_at(dcs, dev.put(bad))
    assert ei.value.code == _lib.RS_ERR_NOT_INVERTIBLE and "t cannot be one of the values in the domain" in str(ei.value)
    s = dev.put(S.Ring(H.oracle_ctx(prm)).random_exceptional(np.random.RandomState(1), cs.m))
    lib = dev.lib
    assert lib.rs_io_eval_at(dev.h, None, _ptr(s), None, None, None, None, None) == _lib.RS_ERR_INVALID
    assert lib.rs_io_eval_at(dev.h, dcs.h, None, None, None, None, None, None) == _lib.RS_ERR_INVALID
    assert lib.rs_io_eval_at(None, dcs.h, _ptr(s), None, None, None, None, None) == _lib.RS_ERR_INVALID
    # every output is optional: Z(s) alone
    Zt = dev.ring_empty()
    assert lib.rs_io_eval_at(dev.h, dcs.h, _ptr(s), None, None, None, _ptr(Zt), None) == _lib.RS_OK
    assert (Zt == dev.io_eval_at(dcs, s)[3]).all()
    # a constraint system of a context with another number of limbs
    dev1 = Device(P.preset("toy54"))
    s1 = dev1.put(np.full((1, 32), 12345, dtype=np.uint64))
    assert dev1.lib.rs_io_eval_at(dev1.h, dcs.h, _ptr(s1), None, None, None, None, None) == _lib.RS_ERR_INVALID
    assert b"constraint system of another context" in lib.rs_last_error()


# ---- GPU: the verifiers -----------------------------------------------------------------------------------------------
def on_device(dev):
    from ringsnark_amd.device import to_host
    return lambda sk, rings, seed: to_host(dev.enc_encode(dev.put(sk), dev.put(rings), seed))


def device_for(name):
    from ringsnark_amd.device import Device
    return Device(P.preset(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name,m", G16_CASES)
def test_groth16_verify_accepts_and_rejects(name, m):
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    c = g16_case(name, m)
    prm, ctx, cs, asg = c["prm"], c["ctx"], c["cs"], c["asg"]
    dev = device_for(name)
    dcs = dev.r1cs(cs)
    pk, vk = S.groth16_generator(ctx, cs, 21, on_device(dev))  # the key of the CPU test, encrypted on the device
    for k in pk:
        assert (pk[k] == c["pk"][k]).all()
    proof, empty = dev.groth16_prove(dcs, {k: dev.put(v) for k, v in pk.items()}, dev.put(asg))
    assert empty == [0, 0, 0] and (to_host(proof) == c["proof"]).all()
    dvk = dev.groth16_vk(dcs, vk)
    primary = asg[: cs.n_inputs]
    dprimary = dev.put(primary)

    def decode(p):
        h = to_host(p)
        return [ctx.enc_decode(vk["sk"], h[k]) for k in range(3)]

    # the device proof
    got = dev.groth16_verify(dvk, dprimary, proof, empty)
    assert_report(got, dict(accepted=True, failed=0, n_bad=(0,) * 6, first=(0, 0, 0, 0, 0)))
    assert got.accepted and dev.groth16_verify(dvk, dprimary, proof).accepted  # h_empty is optional
    # through the wire format
    back, em = dev.enc_deserialize(dev.enc_serialize(proof, empty=empty))
    assert dev.groth16_verify(dvk, dprimary, back, list(em)).accepted
    # one primary input changed in one (limb, slot)
    limb, slot = prm.L - 1, 5
    bad = primary.copy()
    bad[1, limb, slot] = (int(bad[1, limb, slot]) + 1) % prm.q[limb]
    exp = expected_report(g16_sides(ctx, cs, vk, bad, decode(proof)))
    assert exp["failed"] == 1 and exp["n_bad"][0] == 1 and exp["first"][:3] == (0, limb, slot)
    assert_report(dev.groth16_verify(dvk, dev.put(bad), proof, empty), exp)
    assert not S.groth16_verifier(ctx, cs, vk, bad, *decode(proof))
    # C + E(e), e non-zero in one slot of one limb
    e = one_slot(ctx, 0, 7, 3)
    tampered = proof.clone()
    tampered[2] = dev.enc_add(proof[2].contiguous(), dev.enc_encode(dev.put(vk["sk"]), dev.put(e), 99))
    dec = decode(tampered)
    assert (dec[2] == ctx.ring_add(decode(proof)[2], e)).all()
    exp = expected_report(g16_sides(ctx, cs, vk, primary, dec))
    assert exp["n_bad"][0] == 1 and exp["first"][:3] == (0, 0, 7)
    assert_report(dev.groth16_verify(dvk, dprimary, tampered, empty), exp)
    # an element marked EMPTY counts as zero, whatever its payload: A = 0 makes lhs zero in every position
    exp = expected_report(g16_sides(ctx, cs, vk, primary, [np.zeros_like(dec[0])] + decode(proof)[1:]))
    assert exp["n_bad"][0] > 1
    assert_report(dev.groth16_verify(dvk, dprimary, proof, [1, 0, 0]), exp)
    # gamma must be a unit (groth16.tcc:162 divides by it)
    vk_bad = dict(vk)
    vk_bad["gamma"] = vk["gamma"].copy()
    vk_bad["gamma"][limb, 2] = 0
    with pytest.raises(_lib.RsError) as ei:
        dev.groth16_vk(dcs, vk_bad)
    assert ei.value.code == _lib.RS_ERR_NOT_INVERTIBLE and "element is not invertible in ring" in str(ei.value)
    # a key belongs to its context, and to its scheme
    other = device_for(name)
    rep = _lib.VerifyReport()
    from ringsnark_amd.device import _ptr
    assert other.lib.rs_groth16_verify(other.h, dvk.h, _ptr(dprimary), _ptr(proof), None, rep, None) == _lib.RS_ERR_INVALID
    assert other.lib.rs_rinocchio_verify(dev.h, dvk.h, _ptr(dprimary), _ptr(proof), None, rep, None) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_groth16_verify(dev.h, dvk.h, _ptr(dprimary), _ptr(proof), None, None, None) == _lib.RS_ERR_INVALID
    dvk.close()
    assert dvk.h is None


def budget_ladder(ctx, sk, seed=3):
    """tests/test_encoding.py's ladder: a fresh encoding multiplied by a random ring element until its budget is spent."""
    r = ctx.random_ring(seed, 2)
    cur = ctx.enc_encode(sk, r[:1], 5)[0]
    out = [cur]
    for _ in range(16):
        cur = ctx.enc_mul_ring(cur, r[1])
        out.append(cur)
        if len(out) >= 5 and max(ctx.noise_budget(sk, out[-2])) == 0:
            break
    return np.stack(out)


@pytest.mark.gpu
def test_verify_refuses_a_proof_past_its_noise_budget():
    """the reference's verifier throws decoding_error there (seal_ring.tcc:446-454); so does this one, with its message"""
    from ringsnark_amd import _lib
    c = g16_case("toy", 6)
    ctx, cs, vk = c["ctx"], c["cs"], c["vk"]
    dev = device_for("toy")
    dcs = dev.r1cs(cs)
    dvk = dev.groth16_vk(dcs, vk)
    spent = budget_ladder(ctx, vk["sk"])[-1]
    assert max(ctx.noise_budget(vk["sk"], spent)) == 0
    proof = dev.put(c["proof"])
    proof[0] = dev.put(spent)
    with pytest.raises(_lib.RsError) as ei:
        dev.groth16_verify(dvk, dev.put(c["asg"][: cs.n_inputs]), proof, [0, 0, 0])
    assert ei.value.code == _lib.RS_ERR_NOISE and "has remaining noise budget 0 <= 0" in str(ei.value)
    # the same element marked EMPTY is not decoded at all
    assert not dev.groth16_verify(dvk, dev.put(c["asg"][: cs.n_inputs]), proof, [1, 0, 0]).accepted
    # a key outlives its context without harm (a garbage collector drops them in any order): destroy the context first
    dev.lib.rs_ctx_destroy(dev.h)
    dev.h = None
    dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,m,zk", RIN_CASES)
def test_rinocchio_verify_accepts_and_rejects(name, m, zk):
    from ringsnark_amd.device import to_host
    c = rin_case(name, m, zk)
    prm, ctx, cs, asg = c["prm"], c["ctx"], c["cs"], c["asg"]
    dev = device_for(name)
    dcs = dev.r1cs(cs)
    pk, vk = S.rinocchio_generator(ctx, cs, 31, on_device(dev))
    for k in pk:
        assert (pk[k] == c["pk"][k]).all()
    d = [None if x is None else dev.put(x) for x in c["d"]]
    proof, empty = dev.rinocchio_prove(dcs, {k: dev.put(v) for k, v in pk.items()}, dev.put(asg), d[0], d[1], d[2])
    assert empty == [0] * 9 and (to_host(proof) == c["proof"]).all()
    dvk = dev.rinocchio_vk(dcs, vk)
    primary = asg[: cs.n_inputs]
    dprimary, dsk = dev.put(primary), dev.put(vk["sk"])

    def decode(p):
        h = to_host(p)
        return [ctx.enc_decode(vk["sk"], h[k]) for k in range(9)]

    def shifted(k, e, seed):
        t = proof.clone()
        t[k] = dev.enc_add(proof[k].contiguous(), dev.enc_encode(dsk, dev.put(e), seed))
        return t

    got = dev.rinocchio_verify(dvk, dprimary, proof, empty)
    assert_report(got, dict(accepted=True, failed=0, n_bad=(0,) * 6, first=(0, 0, 0, 0, 0)))
    back, em = dev.enc_deserialize(dev.enc_serialize(proof, empty=empty))
    assert dev.rinocchio_verify(dvk, dprimary, back, list(em)).accepted
    # a tampered primary input: P = H Z(s) only
    bad = primary.copy()
    bad[0, prm.L - 1, 2] = (int(bad[0, prm.L - 1, 2]) + 1) % prm.q[prm.L - 1]
    exp = expected_report(rin_sides(ctx, cs, vk, bad, decode(proof)))
    assert exp["failed"] == 1 << 5 and exp["first"][:3] == (5, prm.L - 1, 2)
    assert_report(dev.rinocchio_verify(dvk, dev.put(bad), proof, empty), exp)
    # V' shifted by an encoding of a one-slot element: V' = alpha V only
    t = shifted(1, one_slot(ctx, 0, 9), 101)
    exp = expected_report(rin_sides(ctx, cs, vk, primary, decode(t)))
    assert exp["failed"] == 1 << 0 and exp["n_bad"][0] == 1 and exp["first"][:3] == (0, 0, 9)
    assert_report(dev.rinocchio_verify(dvk, dprimary, t, empty), exp)
    # V itself shifted: V', L_beta and P fail; the report names the lowest check first
    t = shifted(0, one_slot(ctx, prm.L - 1, 4, 2), 102)
    exp = expected_report(rin_sides(ctx, cs, vk, primary, decode(t)))
    assert exp["failed"] == (1 << 0) | (1 << 4) | (1 << 5) and exp["first"][0] == 0
    assert_report(dev.rinocchio_verify(dvk, dprimary, t, empty), exp)
    # F tampered: L_beta only -- and not at all when the last element is EMPTY (rinocchio.tcc:199-206, 283-288)
    t = shifted(8, one_slot(ctx, 0, 1), 103)
    exp = expected_report(rin_sides(ctx, cs, vk, primary, decode(t)))
    assert exp["failed"] == 1 << 4 and exp["first"][:3] == (4, 0, 1)
    assert_report(dev.rinocchio_verify(dvk, dprimary, t, empty), exp)
    got = dev.rinocchio_verify(dvk, dprimary, t, [0] * 8 + [1])
    assert_report(got, dict(accepted=True, failed=0, n_bad=(0,) * 6, first=(0, 0, 0, 0, 0)))
    dvk.close()
