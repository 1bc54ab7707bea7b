"""ringsnark_amd/verify_batch.h: a batch of proofs against one verification key in one pass.

The contract under test: member b's (status, report) is word for word what the single verifier (rs_*_verify_level) returns
for it alone -- so every comparison is equality, with the single call on the device and with the report the CPU computes
from snark_ref's ring operations (tests.test_verify.expected_report on g16_sides / rin_sides).

Members that must be accepted are shown valid on the CPU alone (test_batch_members_are_valid_by_the_reference): positive
noise budget on every ciphertext and accepted by snark_ref's verifier.  Two sources of such members: the oracle's prover
under a snark_ref key (the cases of tests/test_verify.py), and -- for the systems built here for their public columns (70
inputs, hand_rows, no inputs) -- ring elements SOLVED from the verifier's equations for a given primary input and freshly
encoded (`synthesized`): a verifier does not care where a proof came from, and the public sums it must get right depend
on the key and the primary input alone."""
import ctypes as C
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
from tests import test_verify as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NE = {"groth16": 3, "rinocchio": 9}
SWAPPED = {"groth16": 2, "rinocchio": 6}  # the element a "swapped" member replaces: C, resp. H
CASES = [("groth16", n, m, False) for n, m in TV.G16_CASES] + [("rinocchio", n, m, zk) for n, m, zk in TV.RIN_CASES]


# ---- CPU side ----------------------------------------------------------------------------------------------------------
def sides(scheme, ctx, cs, vk, primary, dec):
    return (TV.g16_sides if scheme == "groth16" else TV.rin_sides)(ctx, cs, vk, primary, dec)


def decode(ctx, vk, proof):
    return [ctx.enc_decode(vk["sk"], proof[k]) for k in range(len(proof))]


def expected(scheme, ctx, cs, vk, primary, proof, empty=None):
    """the CPU's report of one member; EMPTY elements count as zero and an EMPTY last Rinocchio element skips check 4"""
    dec = decode(ctx, vk, [p for p in proof]) if empty is None else [
        np.zeros(ctx.ring_shape(), dtype=np.uint64) if empty[k] else ctx.enc_decode(vk["sk"], proof[k]) for k in range(len(proof))]
    skip = (4,) if scheme == "rinocchio" and empty is not None and empty[8] else ()
    return TV.expected_report(sides(scheme, ctx, cs, vk, primary, dec), skip)


def reference_accepts(scheme, ctx, cs, vk, primary, proof):
    for k in range(len(proof)):
        if min(ctx.noise_budget(vk["sk"], proof[k])) <= 0:
            return False
    dec = decode(ctx, vk, proof)
    if scheme == "groth16":
        return bool(S.groth16_verifier(ctx, cs, vk, primary, *dec))
    return bool(S.rinocchio_verifier(ctx, cs, vk, primary, dec)[0])


def one_slot_changed(prm, primary, k, limb, slot):
    bad = primary.copy()
    bad[k, limb, slot] = (int(bad[k, limb, slot]) + 1) % prm.q[limb]
    return bad


def prove(scheme, ctx, cs, pk, asg, d=(None, None, None)):
    if scheme == "groth16":
        proof, empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
    else:
        proof, empty = O.rinocchio_prove(ctx, H.oracle_cs(cs), pk, asg, d[0], d[1], d[2])
    assert not any(empty)
    return proof


@functools.lru_cache(maxsize=None)
def four_kinds(scheme, name, m, zk):
    """[(primary, proof, valid)]: the case's proof; a valid proof of a second assignment; the first with one slot of one
    primary input changed; the first with C (Rinocchio: H) replaced by another valid encoding."""
    c = TV.g16_case(name, m) if scheme == "groth16" else TV.rin_case(name, m, zk)
    prm, ctx, cs, vk = c["prm"], c["ctx"], c["cs"], c["vk"]
    n = cs.n_inputs
    asg2 = H.make_assignment(ctx, cs, seed=23)
    assert (asg2[:n] != c["asg"][:n]).any()
    proof2 = prove(scheme, ctx, cs, c["pk"], asg2, c.get("d", (None,) * 3))
    swapped = c["proof"].copy()
    swapped[SWAPPED[scheme]] = ctx.enc_encode(vk["sk"], ctx.random_ring(91, 1), 17)[0]
    members = [(c["asg"][:n], c["proof"], True), (asg2[:n], proof2, True),
               (one_slot_changed(prm, c["asg"][:n], 1, prm.L - 1, 5), c["proof"], False), (c["asg"][:n], swapped, False)]
    return dict(prm=prm, ctx=ctx, cs=cs, vk=vk, members=members)


def wide_io_r1cs(q, m=8, n_inputs=70, seed=5):
    """row i: (sum_k c_ik x_k + c_i0) * 1 = w_i, small signed coefficients on EVERY input: satisfiable by construction"""
    rng = np.random.RandomState(seed)
    small = lambda: int(rng.randint(-3, 4)) or 2
    rows = {"a": [[(0, small())] + [(k, small()) for k in range(1, n_inputs + 1)] for _ in range(m)],
            "b": [[(0, 1)] for _ in range(m)], "c": [[(n_inputs + 1 + i, 1)] for i in range(m)]}
    return R.from_rows(m, n_inputs + m, n_inputs, rows, q)


def wide_io_assignment(ctx, cs, seed):
    x = ctx.random_ring(seed, cs.n_inputs)
    row = H.lincomb_oracle(ctx, cs)
    return np.ascontiguousarray(np.concatenate([x, np.stack([row("a", i, x) for i in range(cs.m)])]))


def synthesized(scheme, ctx, cs, vk, primary, seed):
    """Encodings of ring elements that satisfy every equation of the verifier for `primary`: two (three) random elements,
    the others solved for (delta and Z(s) are units)."""
    Rg = S.Ring(ctx)
    v, w, y = TV.io_at_s(ctx, cs, vk["s"], primary)
    r = ctx.random_ring(seed, 3)
    if scheme == "groth16":
        f = Rg.add(Rg.add(Rg.mul(vk["beta"], v), Rg.mul(vk["alpha"], w)), y)
        Cc = Rg.mul(Rg.sub(Rg.sub(Rg.mul(r[0], r[1]), Rg.mul(vk["alpha"], vk["beta"])), f), Rg.inv(vk["delta"]))
        els = [r[0], r[1], Cc]
    else:
        V, W, Y = r
        Hh = Rg.mul(Rg.sub(Rg.mul(Rg.add(V, v), Rg.add(W, w)), Rg.add(Y, y)), Rg.inv(vk["Zt"]))
        Lb = Rg.mul(Rg.add(Rg.add(Rg.mul(V, vk["r_v"]), Rg.mul(W, vk["r_w"])), Rg.mul(Y, vk["r_y"])), vk["beta"])
        a = vk["alpha"]
        els = [V, Rg.mul(V, a), W, Rg.mul(W, a), Y, Rg.mul(Y, a), Hh, Rg.mul(Hh, a), Lb]
    return ctx.enc_encode(vk["sk"], np.stack(els), seed + 1)


NO_INPUT_ROWS = {"a": [[(1, 1)], [(0, 3), (2, 1)], [(3, 1)]], "b": [[(2, 1)], [(3, 2)], [(0, 1)]], "c": [[(3, 1)], [(4, 1)], [(1, 1), (0, 2)]]}


@functools.lru_cache(maxsize=None)
def io_system(scheme, which):
    """preset toy.  "wide": 70 public inputs; "hand": tests.test_verify.hand_rows (3 inputs, an empty `a` row, entries on the
    constant one); "none": no inputs.  [(primary, proof, valid)]: two synthesized valid members, then -- with inputs -- each
    of them with one input slot changed, without -- one with an element replaced."""
    prm = P.preset("toy")
    ctx = H.oracle_ctx(prm)
    gen = S.groth16_generator if scheme == "groth16" else S.rinocchio_generator
    if which == "wide":
        cs = wide_io_r1cs(prm.q)
        assert (cs.m, cs.n_inputs, cs.n_vars) == (8, 70, 78)
        assert R.is_satisfied(cs, wide_io_assignment(ctx, cs, 3), prm.q).satisfied
    else:
        cs = R.from_rows(5, 6, 3, TV.hand_rows(), prm.q) if which == "hand" else R.from_rows(3, 4, 0, NO_INPUT_ROWS, prm.q)
    _, vk = gen(ctx, cs, 43, ctx.enc_encode)
    valid = []
    for seed in (3, 13):
        primary = ctx.random_ring(seed, cs.n_inputs) if cs.n_inputs else np.zeros((0,) + ctx.ring_shape(), dtype=np.uint64)
        valid.append((primary, synthesized(scheme, ctx, cs, vk, primary, seed + 100)))
    members = [(x, p, True) for x, p in valid]
    if cs.n_inputs:
        members.append((one_slot_changed(prm, valid[0][0], cs.n_inputs - 1, 0, 3), valid[0][1], False))
        members.append((one_slot_changed(prm, valid[1][0], 0, prm.L - 1, prm.N - 1), valid[1][1], False))
    else:
        swapped = valid[0][1].copy()
        swapped[SWAPPED[scheme]] = ctx.enc_encode(vk["sk"], ctx.random_ring(92, 1), 19)[0]
        members.append((valid[0][0], swapped, False))
    return dict(prm=prm, ctx=ctx, cs=cs, vk=vk, members=members)


@functools.lru_cache(maxsize=None)
def mid_system(scheme):
    """N = 1024, L = 2 (toy's bit sizes): 1024 slot pairs, four workgroups of the check kernel per group of proofs.  A
    three-constraint chain; two synthesized valid members; then the first with input slots changed at (limb, slot) =
    (0, 512), the first pair of the second workgroup, and (1, 1023), the last position of all; and the second with the two
    positions on either side of the limb boundary changed."""
    prm = P.make_params(1024, [30, 30], 1024, [40, 40, 41], ring_factor=1 << 12, name="mid")
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(3, prm.q)
    _, vk = (S.groth16_generator if scheme == "groth16" else S.rinocchio_generator)(ctx, cs, 47, ctx.enc_encode)
    valid = []
    for seed in (3, 13):
        primary = ctx.random_ring(seed, cs.n_inputs)
        valid.append((primary, synthesized(scheme, ctx, cs, vk, primary, seed + 100)))
    far = one_slot_changed(prm, one_slot_changed(prm, valid[0][0], 0, 0, 512), 0, 1, 1023)
    seam = one_slot_changed(prm, one_slot_changed(prm, valid[1][0], 1, 0, 1023), 1, 1, 0)
    members = [(x, p, True) for x, p in valid] + [(far, valid[0][1], False), (seam, valid[1][1], False)]
    return dict(prm=prm, ctx=ctx, cs=cs, vk=vk, members=members, first=[None, None, (0, 512), (0, 1023)])


def test_library_exports_every_function_of_verify_batch_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ringsnark_amd", "verify_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.VERIFY_BATCH_SIGNATURES) and len(names) == 3
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 110
    assert int(re.search(r"#define\s+RS_VERIFY_BATCH_MAX\s+(\d+)", code).group(1)) == _lib.VERIFY_BATCH_MAX == 64
    assert lib.rs_verify_batch_group() == _lib.VERIFY_BATCH_GROUP and 2 <= _lib.VERIFY_BATCH_GROUP < _lib.VERIFY_BATCH_MAX


@pytest.mark.parametrize("scheme,name,m,zk", CASES)
def test_batch_members_are_valid_by_the_reference(scheme, name, m, zk):
    k = four_kinds(scheme, name, m, zk)
    for primary, proof, valid in k["members"]:
        exp = expected(scheme, k["ctx"], k["cs"], k["vk"], primary, proof)
        assert exp["accepted"] == valid
        if valid:
            assert reference_accepts(scheme, k["ctx"], k["cs"], k["vk"], primary, proof)


@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
@pytest.mark.parametrize("which", ["wide", "hand", "none", "mid"])
def test_io_system_members_are_valid_by_the_reference(scheme, which):
    k = mid_system(scheme) if which == "mid" else io_system(scheme, which)
    for primary, proof, valid in k["members"]:
        assert expected(scheme, k["ctx"], k["cs"], k["vk"], primary, proof)["accepted"] == valid
        assert reference_accepts(scheme, k["ctx"], k["cs"], k["vk"], primary, proof) == valid


# ---- GPU side ----------------------------------------------------------------------------------------------------------
class OnDevice:
    """a key and members on the device, and the two ways to verify them"""

    def __init__(self, scheme, k, name="toy"):
        self.scheme, self.k = scheme, k
        self.dev = TV.device_for(name)
        self.dcs = self.dev.r1cs(k["cs"])
        self.dvk = (self.dev.groth16_vk if scheme == "groth16" else self.dev.rinocchio_vk)(self.dcs, k["vk"])
        self.n_inputs = k["cs"].n_inputs

    def put(self, members):
        return [(self.dev.put(x) if self.n_inputs else None, self.dev.put(p)) for x, p, *_ in members]

    def single(self, primary, proof, empty=None, level=None):
        fn = self.dev.groth16_verify if self.scheme == "groth16" else self.dev.rinocchio_verify
        return fn(self.dvk, primary, proof, empty, level)

    def batch(self, members, empties=None, level=None):
        fn = self.dev.groth16_verify_batch if self.scheme == "groth16" else self.dev.rinocchio_verify_batch
        return fn(self.dvk, [x for x, _ in members] if self.n_inputs else None, [p for _, p in members], empties, level)

    def raw(self, K_lvl, batch, primary, proofs, empty=None, n_out=None, vk="own", ctx=None, fn=None, status=True, reports=True, budget=True):
        """the C call: (return code, status [n_out], budget [n_out], reports [n_out]) with the outputs pre-filled with 0x55"""
        from ringsnark_amd import _lib
        from ringsnark_amd.device import _ptr
        n_out = max(batch, 1) if n_out is None else n_out
        st, bu, rp = (C.c_int * n_out)(), (C.c_int * n_out)(), (_lib.VerifyReport * n_out)()
        for buf in (st, bu, rp):
            C.memset(buf, 0x55, C.sizeof(buf))
        fn = fn or (self.dev.lib.rs_groth16_verify_batch if self.scheme == "groth16" else self.dev.lib.rs_rinocchio_verify_batch)
        em = None if empty is None else (C.c_int * len(empty))(*empty)
        rc = fn(ctx or self.dev.h, self.dvk.h if vk == "own" else vk, K_lvl, batch, _ptr(primary), _ptr(proofs), em, st if status else None,
                bu if budget else None, rp if reports else None, self.dev.stream())
        return rc, list(st), list(bu), [bytes(r) for r in rp]


def assert_verdict(got, want_result):
    assert got.result == want_result and not got.noise_spent and got.budget_min > 0
    assert bool(got) == bool(want_result.accepted)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,name,m,zk", CASES)
def test_batch_equals_the_single_verifier_and_the_cpu(scheme, name, m, zk):
    """Every batch size around the register group, accepted and rejected members alternating inside a group."""
    from ringsnark_amd import _lib
    k = four_kinds(scheme, name, m, zk)
    d = OnDevice(scheme, k, name)
    on = d.put(k["members"])
    single = [d.single(x, p) for x, p in on]
    for got, (primary, proof, _) in zip(single, k["members"]):
        TV.assert_report(got, expected(scheme, k["ctx"], k["cs"], k["vk"], primary, proof))
    assert [bool(s) for s in single] == [True, True, False, False]
    PB = _lib.VERIFY_BATCH_GROUP
    order = [0, 2, 1, 3]
    for B in sorted({1, 2, PB - 1, PB, PB + 1, 2 * PB + 1, 64}):
        idx = [order[b % 4] for b in range(B)]
        got = d.batch([on[i] for i in idx])
        assert len(got) == B
        for g, i in zip(got, idx):
            assert_verdict(g, single[i])
    # stacked tensors are taken as lists are
    import torch
    idx = [order[b % 4] for b in range(PB + 1)]
    stacked = d.dev.groth16_verify_batch if scheme == "groth16" else d.dev.rinocchio_verify_batch
    got = stacked(d.dvk, torch.stack([on[i][0] for i in idx]), torch.stack([on[i][1] for i in idx]))
    assert [g.result for g in got] == [single[i] for i in idx]
    d.dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_many_public_inputs_few_and_none(scheme):
    """70 inputs (the k-loop of the kernel, every column used), hand_rows (an empty row, entries on the constant one), and no
    inputs with d_primary = NULL; batches of 5 and 9."""
    for which in ("wide", "hand", "none"):
        k = io_system(scheme, which)
        d = OnDevice(scheme, k)
        on = d.put(k["members"])
        exps = [expected(scheme, k["ctx"], k["cs"], k["vk"], x, p) for x, p, _ in k["members"]]
        for e, (_, _, valid) in zip(exps, k["members"]):
            assert e["accepted"] == valid  # one changed input slot fails one position of the check that reads the public sums
            assert valid or not k["cs"].n_inputs or (e["n_bad"][0 if scheme == "groth16" else 5] == 1 and sum(e["n_bad"]) == 1)
        for B in (5, 9):
            idx = [b % len(on) for b in range(B)]
            got = d.batch([on[i] for i in idx])
            for g, i in zip(got, idx):
                TV.assert_report(g.result, exps[i])
                assert bool(g) == k["members"][i][2] and not g.noise_spent
        d.dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,force_int", [("groth16", 0), ("groth16", 1), ("rinocchio", 0), ("rinocchio", 1)])
def test_more_than_one_workgroup_per_proof(scheme, force_int):
    """both arithmetics at a size where the slot pairs of a proof span four workgroups: failures in the second and in the
    last of them, and on both sides of the limb boundary"""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device
    k = mid_system(scheme)
    check = 0 if scheme == "groth16" else 5
    exps = [expected(scheme, k["ctx"], k["cs"], k["vk"], x, p) for x, p, _ in k["members"]]
    for e, (_, _, valid), first in zip(exps, k["members"], k["first"]):
        assert e["accepted"] == valid and (valid or (e["n_bad"][check] == 2 and e["first"][:3] == (check,) + first))
    with _lib.tuning(force_int_arith=force_int):
        dev = Device(k["prm"])
    dvk = (dev.groth16_vk if scheme == "groth16" else dev.rinocchio_vk)(dev.r1cs(k["cs"]), k["vk"])
    verify, batch = (dev.groth16_verify, dev.groth16_verify_batch) if scheme == "groth16" else (dev.rinocchio_verify, dev.rinocchio_verify_batch)
    on = [(dev.put(x), dev.put(p)) for x, p, _ in k["members"]]
    idx = [b % 4 for b in range(_lib.VERIFY_BATCH_GROUP + 1)]
    got = batch(dvk, [on[i][0] for i in idx], [on[i][1] for i in idx])
    for g, i in zip(got, idx):
        TV.assert_report(g.result, exps[i])
        assert g.result == verify(dvk, *on[i]) and not g.noise_spent
    dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_mass_rejection_is_deterministic(scheme):
    """a primary input wrong in every slot of every limb: every wave of the kernel reports"""
    from ringsnark_amd import _lib
    k = four_kinds(scheme, "toy", 6 if scheme == "groth16" else 9, scheme == "rinocchio")
    prm, (primary, proof, _) = k["prm"], k["members"][0]
    wrong = primary.copy()
    for limb, q in enumerate(prm.q):
        wrong[0, limb] = (wrong[0, limb] + np.uint64(1)) % np.uint64(q)
    exp = expected(scheme, k["ctx"], k["cs"], k["vk"], wrong, proof)
    check = 0 if scheme == "groth16" else 5
    assert exp["n_bad"][check] == prm.L * prm.N and exp["first"][:3] == (check, 0, 0)  # the first input's column is a unit in every slot here
    d = OnDevice(scheme, k)
    good, bad = d.put(k["members"][:1])[0], d.put([(wrong, proof)])[0]
    PB = _lib.VERIFY_BATCH_GROUP
    first = d.batch([bad] + [good] * PB)
    again = d.batch([bad] + [good] * PB)
    last = d.batch([good] * PB + [bad])
    TV.assert_report(first[0].result, exp)
    assert first == again and first[0] == last[-1] and all(first[1:]) and all(last[:-1])
    d.dvk.close()


@pytest.mark.gpu
def test_a_spent_budget_is_the_verdict_of_that_member_only():
    from ringsnark_amd import _lib
    import torch
    k = four_kinds("groth16", "toy", 6, False)
    ctx, vk, prm = k["ctx"], k["vk"], k["prm"]
    d = OnDevice("groth16", k)
    on = d.put(k["members"])
    spent = TV.budget_ladder(ctx, vk["sk"])[-1]
    assert max(ctx.noise_budget(vk["sk"], spent)) == 0
    noisy = on[0][1].clone()
    noisy[0] = d.dev.put(spent)
    members = [on[0], on[2], (on[0][0], noisy), on[1], on[3]]
    with pytest.raises(_lib.RsError) as ei:
        d.single(*members[2])
    assert ei.value.code == _lib.RS_ERR_NOISE and "has remaining noise budget 0 <= 0" in str(ei.value)
    got = d.batch(members)
    without = d.batch(members[:2] + members[3:])
    assert got[:2] + got[3:] == without
    assert got[2].result is None and got[2].noise_spent and got[2].budget_min == 0 and not got[2]
    sk = d.dev.put(vk["sk"])
    assert [g.budget_min for g in got] == [int(d.dev.enc_noise_budget(sk, p.contiguous()).min()) for _, p in members]
    assert all(g.budget_min > 0 and not g.noise_spent for g in without)
    # the C call: RS_OK as a whole, RS_ERR_NOISE and an all-zero report for that member
    rc, status, budget, reports = d.raw(prm.K, 5, torch.stack([x for x, _ in members]), torch.stack([p for _, p in members]))
    assert rc == _lib.RS_OK and status == [_lib.RS_OK, _lib.RS_OK, _lib.RS_ERR_NOISE, _lib.RS_OK, _lib.RS_OK]
    assert reports[2] == bytes(C.sizeof(_lib.VerifyReport)) and budget == [g.budget_min for g in got]
    d.dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_empty_elements_count_as_zero_and_are_not_decoded(scheme):
    """EMPTY elements carry all-ones payloads (no residue of any prime): decoding them would report noise."""
    k = four_kinds(scheme, "toy", 6 if scheme == "groth16" else 9, scheme == "rinocchio")
    ctx, cs, vk, prm = k["ctx"], k["cs"], k["vk"], k["prm"]
    ne = NE[scheme]
    d = OnDevice(scheme, k)
    on = d.put(k["members"])

    def blanked(proof, flags):
        t = proof.clone()
        for e, f in enumerate(flags):
            if f:
                t[e] = -1
        return t

    first = [1] + [0] * (ne - 1)
    last = [0] * (ne - 1) + [1]
    none, every = [0] * ne, [1] * ne
    swapped_last = k["members"][0][1].copy()
    swapped_last[ne - 1] = ctx.enc_encode(vk["sk"], ctx.random_ring(93, 1), 21)[0]
    on_swapped = d.dev.put(swapped_last)
    m0, m1 = k["members"][0], k["members"][1]
    swapped = (on[0][0], on_swapped)
    # (member on the device, flags, its primary input and proof on the host)
    plan = [(on[0], none, m0[0], m0[1]), (on[0], first, m0[0], m0[1]), (on[1], last, m1[0], m1[1]), (swapped, none, m0[0], swapped_last),
            (on[0], every, m0[0], m0[1]), (on[1], none, m1[0], m1[1]), (swapped, last, m0[0], swapped_last)]
    members = [(x, blanked(p, flags)) for (x, p), flags, _, _ in plan]
    got = d.batch(members, [flags for _, flags, _, _ in plan])
    for g, (x, p), (_, flags, primary, proof) in zip(got, members, plan):
        assert not g.noise_spent and g.result == d.single(x, p, flags)
        TV.assert_report(g.result, expected(scheme, ctx, cs, vk, primary, proof, flags))
    assert got[0] and got[5] and not got[1] and not got[4]
    assert got[4].budget_min == H.noise_tb(prm.Q) - 1  # nothing decoded: the budget of a noiseless ciphertext
    if scheme == "rinocchio":
        # element 8 EMPTY: check 4 is skipped for that member -- and made for its neighbours
        assert got[2] and got[6] and got[3].result.failed == 1 << 4
    d.dvk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_a_batch_of_switched_proofs(scheme):
    import torch
    k = four_kinds(scheme, "toy", 6 if scheme == "groth16" else 9, scheme == "rinocchio")
    prm = k["prm"]
    d = OnDevice(scheme, k)
    lvl = prm.K - 1
    on = [(x, d.dev.enc_mod_switch(p.contiguous(), lvl)) for x, p in d.put(k["members"])]
    t = on[0][1].clone()  # a switched proof with one word changed: rejected, or past its budget
    t[1, 0, 0, 0, 2] = (t[1, 0, 0, 0, 2] + 1) % int(prm.Q[0])
    members = on + [(on[0][0], t)] + on[:2]
    got = d.batch(members, level=lvl)
    sk = d.dev.put(k["vk"]["sk"])
    for g, (x, p) in zip(got, members):
        assert g.budget_min == int(d.dev.enc_noise_budget(sk, p, level=lvl).min())
        if g.noise_spent:
            assert g.budget_min == 0 and g.result is None
        else:
            assert g.result == d.single(x, p, level=lvl)
    assert [bool(g) for g in got] == [True, True, False, False, False, True, True] and not any(g.noise_spent for g in got[:4])
    full = d.batch(d.put(k["members"]))
    assert [g.result for g in got[:4]] == [g.result for g in full]  # the report of the unswitched proof, field for field
    d.dvk.close()


@pytest.mark.gpu
def test_arguments_are_validated_and_outputs_untouched_on_error():
    from ringsnark_amd import _lib
    import torch
    k = four_kinds("groth16", "toy", 6, False)
    K = k["prm"].K
    d = OnDevice("groth16", k)
    on = d.put(k["members"])
    primary, proofs = torch.stack([x for x, _ in on]), torch.stack([p for _, p in on])
    untouched = lambda out: all(v == 0x55555555 for v in out[1] + out[2]) and all(r == b"\x55" * len(r) for r in out[3])
    ok = d.raw(K, 4, primary, proofs)
    assert ok[0] == _lib.RS_OK and ok[1] == [_lib.RS_OK] * 4
    zero = d.raw(K, 0, primary, proofs)
    assert zero[0] == _lib.RS_OK and untouched(zero)
    rin = four_kinds("rinocchio", "toy", 9, True)
    d_rin = OnDevice("rinocchio", rin)
    other = TV.device_for("toy")
    bad_calls = [dict(batch=65, n_out=65), dict(batch=-1), dict(K_lvl=0), dict(K_lvl=K + 1), dict(vk=d_rin.dvk.h),
                 dict(fn=d.dev.lib.rs_rinocchio_verify_batch), dict(ctx=other.h), dict(proofs=None), dict(status=False), dict(reports=False),
                 dict(primary=None), dict(vk=None)]
    for kw in bad_calls:
        args = dict(K_lvl=K, batch=4, primary=primary, proofs=proofs)
        args.update(kw)
        out = d.raw(**args)
        assert out[0] == _lib.RS_ERR_INVALID and untouched(out), kw
    assert d.dev.lib.rs_groth16_verify_batch(None, d.dvk.h, K, 4, None, None, None, None, None, None, None) == _lib.RS_ERR_INVALID
    # h_budget_min and h_empty are optional
    assert d.raw(K, 4, primary, proofs, budget=False)[1] == [_lib.RS_OK] * 4
    d.dvk.close()
    d_rin.dvk.close()
