"""Setup, prove and verify with real keys at the parameters of the configurations C2, C3 (the headline), C4 and C5.

The chain of a proof -- trapdoor, generator, prover, decode behind the noise guard, verification equation -- on the presets
the project is measured on, where every other test at these shapes multiplies uniform random words and decrypts nothing.

Tier A (TIER_A): bit for bit against the CPU.  The key is tests/test_keygen.py's cpu_key (snark_ref's O(m^2) instance map, the
oracle's ring operations and encoder, disjoint seeds), the proof the oracle prover's.  m = 8, m = 4 on C4.
Tier B (TIER_B): m = 64, no CPU key and no CPU prover.  The device generates the key and proves; the host checks what the
proof means: the oracle's decode and budgets of the downloaded proof, the closed forms A = alpha + A(s), B = beta + B(s),
snark_ref's verifier on the decoded elements, and the reports of tampered runs.

Every comparison is equality of integers.  The one inequality is the worst-case noise bound (noise_bound, derived in
DESIGN.md "End to end at configuration parameters"): a proof element is a sum of T terms, each a key element -- whose
c0 + c1 s is v = m - t e with a ternary e, |v| < 2^(bitlen(t) + 1) -- multiplied by `muls` plaintexts with centred coefficients
(|p| <= (t - 1) / 2 < 2^(bitlen(t) - 1), N_enc of them), so
    |v_sum| < T (N_enc 2^(bitlen(t) - 1))^muls |v_fresh|,
    budget >= fresh - muls (bitlen(max q_i) + log2 N_enc) - ceil(log2 T) - c,        c = 0
(the derivation leaves `muls` bits to spare: the centred plaintexts).  muls is 1 everywhere but in the six elements the ZK
terms of Rinocchio touch, where the prover multiplies <s_pows, Z> by d_k (rinocchio.tcc:167-174): one more plaintext, muls = 2.
`fresh` is the smallest budget the oracle reports over the elements of the case's key; that no element of any key has less
than tb - bitlen(max q_i) - 2 (fresh_floor) follows from the ternary error and is asserted against the measured value, so
the bound at a configuration's stated constraint count, whose key no test builds, stands on the floor.

CPU cases are built once per process (functools.lru_cache) and never modified; so is the device side of a case (on_gpu)."""
import functools
import json
import os
import re

import numpy as np
import pytest

from ringsnark_amd import modswitch as MS
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests import modswitch_cases as MC
from tests import snark_ref as S
from tests.test_keygen import VECTORS, assert_same_key, device_for, device_keygen, disjoint_seeds, e2e_case, trapdoor, with_r_y
from tests.test_verify import assert_report, expected_report, g16_sides, io_at_s, one_slot, polys_at_s, rin_sides

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G16, RIN = "groth16", "rinocchio"
# (scheme, preset, m, ZK elements set)
TIER_A = [(G16, "C2", 8, False), (G16, "C3", 8, False), (G16, "C5", 8, False), (G16, "C4", 4, False),
          (RIN, "C2", 8, True), (RIN, "C3", 8, True), (RIN, "C5", 8, True), (RIN, "C4", 4, True), (RIN, "C3", 8, False)]
TIER_B = [(G16, "C3", 64, False), (RIN, "C3", 64, True), (G16, "C2", 64, False)]
COMPACT = [(G16, "C3", 8, False), (RIN, "C2", 8, True)]
LEVELS = [(G16, "C2", 8, False), (G16, "C3", 8, False)]
BATCH = (G16, "C3", 8, False)
ACCEPTED = dict(accepted=True, failed=0, n_bad=(0,) * 6, first=(0, 0, 0, 0, 0))
NOISE_TEXT = "ciphertext #%d has remaining noise budget 0 <= 0"
C_SLACK = 0


def ident(case):
    return "%s-%s-m%d%s" % (case[0], case[1], case[2], "-zk" if case[3] else "")


# ---- the noise bound -------------------------------------------------------------------------------------------------
def ceil_log2(T):
    return (T - 1).bit_length()


def plain_bits(prm):
    """bits one multiplication by a plaintext can cost: bitlen(max q_i) + log2 N_enc"""
    return max(int(q).bit_length() for q in prm.q) + prm.N_enc.bit_length() - 1


def fresh_floor(prm):
    """the least budget of a freshly encoded element: |m - t e| <= (t - 1) / 2 + t < 2^(bitlen(t) + 1), e ternary"""
    return H.noise_tb(prm.Q) - max(int(q).bit_length() for q in prm.q) - 2


def noise_bound(prm, fresh, T, muls=1):
    """the least budget of a sum of T terms, each a key element of budget >= fresh times at most `muls` plaintexts"""
    return fresh - muls * plain_bits(prm) - ceil_log2(T) - C_SLACK


def proof_terms(scheme, m, n_aux, zk):
    """(T, muls) per proof element, read off the oracle's provers (oracle/rs_oracle.c, groth16.tcc:89-112,
    rinocchio.tcc:106-185).  ringGroth16: A, B = <s_pows, io> + <s_pows, mid> + alpha or beta; C = <delta_ts, H> + <delta_mid,
    aux>.  Rinocchio: V, V', W, W', Y, Y' = <., mid> (+ d_k <., Z>: m + 1 more terms, of two plaintexts each but the
    leading one); H, H' = <., H>; L_beta = <beta_prods, aux> (+ d_k beta_r?_ts: three more terms)."""
    if scheme == G16:
        return [(2 * m + 1, 1), (2 * m + 1, 1), (m + 1 + n_aux, 1)]
    mid = (2 * m + 1, 2) if zk else (m, 1)
    return [mid] * 6 + [(m + 1, 1)] * 2 + [(n_aux + (3 if zk else 0), 1)]


def stated_constraint_counts():
    """{preset: (scheme, m)} of the configurations BASELINE.json states with a prover and a constraint count"""
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        configs = json.load(f)["configs"]
    shapes = {(P.preset(n).N, P.preset(n).L): n for n in ("C2", "C3", "C4")}
    out = {}
    for line in configs:
        hit = re.search(r"(ringGroth16|Rinocchio) prover, 2\^(\d+) [^,]*constraints, N=(\d+), (\d+) RNS primes", line)
        if hit and (int(hit.group(3)), int(hit.group(4))) in shapes:
            out[shapes[(int(hit.group(3)), int(hit.group(4)))]] = (G16 if hit.group(1) == "ringGroth16" else RIN, 1 << int(hit.group(2)))
    return out


# ---- cases (CPU, computed once) --------------------------------------------------------------------------------------
def measured_fresh(ctx, sk, pk):
    """the smallest budget the oracle reports over every limb of every element of a key"""
    return min(min(ctx.noise_budget(sk, e)) for v in pk.values() for e in v.reshape((-1,) + ctx.enc_shape()))


@functools.lru_cache(maxsize=None)
def tier_a(scheme, name, m, zk):
    """tests/test_keygen.py's e2e_case, the oracle's budgets [n][L] and decodings of its proof, and the key's fresh budget"""
    c = dict(e2e_case(scheme, name, m, zk))
    ctx, sk = c["ctx"], c["vk"]["sk"]
    c["budget"] = np.array([ctx.noise_budget(sk, e) for e in c["proof"]])
    c["dec"] = [ctx.enc_decode(sk, e) for e in c["proof"]]
    c["fresh"] = measured_fresh(ctx, sk, c["pk"])
    return c


def vanishing_at(ctx, s, m):
    Rg = S.Ring(ctx)
    Zt = s
    for i in range(1, m):
        Zt = Rg.mul(Zt, Rg.sub(s, Rg.scalar(i)))
    return Zt


@functools.lru_cache(maxsize=None)
def tier_b(scheme, name, m, zk):
    """the trapdoor, seeds and assignment of e2e_case without the CPU key and the CPU proof"""
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 41 if scheme == G16 else 43, ctx.keygen(5)), prm.q)
    if scheme == RIN:
        vk["Zt"] = vanishing_at(ctx, vk["s"], cs.m)
    return dict(prm=prm, ctx=ctx, cs=cs, asg=H.make_assignment(ctx, cs), vk=vk, seeds=disjoint_seeds(900, len(VECTORS[scheme])),
                d=ctx.random_ring(77, 3) if zk else [None] * 3, fresh=fresh_floor(prm))


def verifier_accepts(scheme, ctx, cs, vk, primary, dec):
    if scheme == G16:
        return S.groth16_verifier(ctx, cs, vk, primary, *dec)
    return S.rinocchio_verifier(ctx, cs, vk, primary, list(dec))[0]


def bounds(scheme, c, zk):
    cs = c["cs"]
    return [noise_bound(c["prm"], c["fresh"], T, muls) for T, muls in proof_terms(scheme, cs.m, cs.n_aux, zk)]


# ---- CPU: statements about the inputs --------------------------------------------------------------------------------
def test_cases_are_the_configurations_shapes():
    shape = lambda n: (P.preset(n).N, P.preset(n).L, P.preset(n).N_enc, P.preset(n).K)
    assert shape("C2") == (4096, 2, 8192, 4) and shape("C3") == (8192, 4, 8192, 4)
    assert shape("C4") == (16384, 6, 16384, 8) and shape("C5") == (2048, 1, 16384, 8)
    assert max(P.preset("C5").q) >= 1 << 50  # the ring side of C5 runs on the integer arithmetic
    for scheme, name, m, zk in TIER_A + TIER_B:
        cs = R.chain_r1cs(m, P.preset(name).q)
        assert (cs.m, cs.n_inputs, cs.n_aux) == (m, 2, m)
    assert stated_constraint_counts() == {"C2": (G16, 1 << 10), "C3": (G16, 1 << 16), "C4": (RIN, 1 << 18)}


@pytest.mark.parametrize("case", TIER_A, ids=ident)
def test_inputs_are_valid_by_the_reference(case):
    """a positive oracle budget in every limb of every element (none is EMPTY), accepted by snark_ref's verifier"""
    scheme, name, m, zk = case
    c = tier_a(*case)
    ctx, cs, vk = c["ctx"], c["cs"], c["vk"]
    assert c["empty"] == [0] * len(c["proof"])
    print("%s: fresh %d, budgets %s" % (ident(case), c["fresh"], c["budget"].tolist()))
    assert (c["budget"] > 0).all()
    primary = c["asg"][: cs.n_inputs]
    assert verifier_accepts(scheme, ctx, cs, vk, primary, c["dec"])
    sides = g16_sides if scheme == G16 else rin_sides
    assert expected_report(sides(ctx, cs, vk, primary, c["dec"])) == ACCEPTED


@pytest.mark.parametrize("case", TIER_A, ids=ident)
def test_noise_bound_holds_for_the_oracle_budgets(case):
    """every limb of every element has at least noise_bound(fresh, T, muls) bits, fresh measured on the case's own key and no
    lower than the floor the ternary error implies; the bound itself is positive at these m"""
    scheme, name, m, zk = case
    c = tier_a(*case)
    assert c["fresh"] >= fresh_floor(c["prm"])
    want = bounds(scheme, c, zk)
    print("%s: fresh %d (floor %d), bound %s, least budget %s" % (ident(case), c["fresh"], fresh_floor(c["prm"]), want, c["budget"].min(axis=1).tolist()))
    for k, b in enumerate(want):
        assert b > 0 and c["budget"][k].min() >= b, (k, b, c["budget"][k].tolist())


def test_noise_bound_is_positive_at_the_stated_constraint_counts():
    """2^10 on C2, 2^16 on C3 (ringGroth16), 2^18 on C4 (Rinocchio, with and without the ZK elements), on the chain
    circuit's n_aux = m and the floor of a fresh budget: the proofs the headline numbers describe decode"""
    for name, (scheme, m) in sorted(stated_constraint_counts().items()):
        prm = P.preset(name)
        for zk in ((False, True) if scheme == RIN else (False,)):
            got = [noise_bound(prm, fresh_floor(prm), T, muls) for T, muls in proof_terms(scheme, m, m, zk)]
            print("%s %s m = 2^%d%s: fresh floor %d, bound %s" % (name, scheme, m.bit_length() - 1, " zk" if zk else "", fresh_floor(prm), got))
            assert min(got) > 0, (name, scheme, m, zk, got)


# ---- GPU -------------------------------------------------------------------------------------------------------------
device = functools.lru_cache(maxsize=None)(device_for)


def prove(dev, scheme, dcs, pk, asg, d):
    if scheme == G16:
        return dev.groth16_prove(dcs, pk, asg, check=True)
    return dev.rinocchio_prove(dcs, pk, asg, d[0], d[1], d[2], check=True)


@functools.lru_cache(maxsize=None)
def on_gpu(scheme, name, m, zk):
    """The device side of a case, once: key generated from the case's trapdoor and seeds, proof (check=True), verification
    key; the downloaded proof with the oracle's budgets and decodings of it (tier A: those of the CPU proof, which
    test_proof_bytes shows to be the same words); v_io(s), w_io(s), y_io(s) of the primary input."""
    from ringsnark_amd.device import to_host
    a = (scheme, name, m, zk) in TIER_A
    c = tier_a(scheme, name, m, zk) if a else tier_b(scheme, name, m, zk)
    ctx, cs, vk = c["ctx"], c["cs"], c["vk"]
    dev = device(name)
    dcs = dev.r1cs(cs)
    pk = device_keygen(dev, scheme, dcs, vk, seeds=c["seeds"])
    d = [None if x is None else dev.put(x) for x in c["d"]]
    dasg = dev.put(c["asg"])
    proof, empty = prove(dev, scheme, dcs, pk, dasg, d)
    dvk = (dev.groth16_vk if scheme == G16 else dev.rinocchio_vk)(dcs, vk)
    host = to_host(proof)
    g = dict(c=c, dev=dev, dcs=dcs, pk=pk, d=d, dasg=dasg, proof=proof, empty=empty, dvk=dvk, dsk=dev.put(vk["sk"]), host=host,
             verify=dev.groth16_verify if scheme == G16 else dev.rinocchio_verify, sides=g16_sides if scheme == G16 else rin_sides,
             primary=c["asg"][: cs.n_inputs], io=io_at_s(ctx, cs, vk["s"], c["asg"][: cs.n_inputs]))
    g["ref_budget"] = c["budget"] if a else np.array([ctx.noise_budget(vk["sk"], e) for e in host])
    g["ref_dec"] = c["dec"] if a else [ctx.enc_decode(vk["sk"], e) for e in host]
    return g


def tampered(g):
    """(a primary input changed in the last slot of the last limb, the proof with one word of its last element changed),
    once per case"""
    if "bad" not in g:
        c = g["c"]
        prm = c["prm"]
        bad = g["primary"].copy()
        bad[-1, prm.L - 1, prm.N - 1] = (int(bad[-1, prm.L - 1, prm.N - 1]) + 1) % prm.q[prm.L - 1]
        word = g["host"].copy()
        spot = (len(word) - 1, prm.L - 1, 1, prm.K - 1, prm.N_enc - 1)
        word[spot] = (int(word[spot]) + 1) % prm.Q[prm.K - 1]
        g["bad"], g["word"] = bad, word
    return g["bad"], g["word"]


def verdict(g, primary, proof):
    """the single verifier's answer: a VerifyResult, or the text of its RS_ERR_NOISE"""
    from ringsnark_amd import _lib
    try:
        return g["verify"](g["dvk"], g["dev"].put(primary), proof, g["empty"])
    except _lib.RsError as e:
        assert e.code == _lib.RS_ERR_NOISE
        return str(e)


def assert_verdict(g, got, primary, host_proof):
    """`got` (verdict) is what the oracle says of host_proof: the reference's refusal, naming the first spent limb, where it
    reports a spent budget; else the report of the sides computed from the oracle's decodings"""
    c = g["c"]
    ctx, sk = c["ctx"], c["vk"]["sk"]
    budget = np.array([ctx.noise_budget(sk, e) for e in host_proof])
    if (budget > 0).all():
        dec = [ctx.enc_decode(sk, e) for e in host_proof]
        io = g["io"] if primary is g["primary"] else None
        exp = expected_report(g["sides"](ctx, c["cs"], c["vk"], primary, dec, io))
        assert_report(got, exp)
        return exp
    k = int(np.argmax((budget <= 0).any(axis=1)))
    print("refused by the oracle's guard: element %d, budgets %s" % (k, budget[k].tolist()))
    assert isinstance(got, str) and NOISE_TEXT % int(np.argmax(budget[k] <= 0)) in got, (got, budget.tolist())
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIER_A, ids=ident)
def test_key_bytes_match_the_cpu(case):
    """every vector of the device-resident key, and of the key streamed to the host in tiles of 3, is the CPU's: 8192 points
    on 512 threads (C2, C3) and 16384 on 1024 (C4, C5), 16 coefficients per thread"""
    scheme = case[0]
    g = on_gpu(*case)
    c, dev = g["c"], g["dev"]
    assert_same_key(dev, scheme, g["pk"], c["pk"])
    hosted = device_keygen(dev, scheme, g["dcs"], c["vk"], seeds=c["seeds"], host=True, tile=3)
    assert_same_key(dev, scheme, hosted, c["pk"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIER_A, ids=ident)
def test_proof_bytes_match_the_oracle(case):
    g = on_gpu(*case)
    assert g["empty"] == g["c"]["empty"]
    assert (g["host"] == g["c"]["proof"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIER_A + TIER_B, ids=ident)
def test_decode_and_budgets_match_the_oracle(case):
    """rs_enc_decode and rs_enc_noise_budget of the proof, word for word; the budgets at or above the worst-case bound;
    ringGroth16: the decoded A and B are alpha + A(s) and beta + B(s) of the full assignment"""
    from ringsnark_amd.device import to_host
    scheme, name, m, zk = case
    g = on_gpu(*case)
    c, dev = g["c"], g["dev"]
    assert g["empty"] == [0] * len(g["host"])
    budget = dev.enc_noise_budget(g["dsk"], g["proof"])
    print("%s: budgets %s" % (ident(case), budget.tolist()))
    assert (budget == g["ref_budget"]).all(), (budget.tolist(), g["ref_budget"].tolist())
    for k, b in enumerate(bounds(scheme, c, zk)):
        assert budget[k].min() >= b > 0, (k, b, budget[k].tolist())
    dec = to_host(dev.enc_decode(g["dsk"], g["proof"]))
    for k in range(len(g["host"])):
        assert (dec[k] == g["ref_dec"][k]).all(), k
        one = to_host(dev.enc_decode(g["dsk"], g["proof"][k].contiguous()))  # one element: the launch of a single decode
        assert (one == dec[k]).all(), k
    if scheme == G16:
        ctx, vk = c["ctx"], c["vk"]
        As, Bs, _ = polys_at_s(ctx, c["cs"], vk["s"], c["asg"])
        assert (dec[0] == ctx.ring_add(vk["alpha"], As)).all()
        assert (dec[1] == ctx.ring_add(vk["beta"], Bs)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", TIER_A + TIER_B, ids=ident)
def test_verdicts_match_the_reference(case):
    """Accepted by the device and -- its decodings -- by snark_ref's verifier.  A primary input changed in the last slot of
    the last limb, one proof word changed, and the last element shifted by an encoding of a one-slot element: the report of
    expected_report field for field, or the reference's refusal where the oracle finds the budget spent (one word of a
    transform moves every coefficient of the noise polynomial)."""
    from ringsnark_amd.device import to_host
    scheme, name, m, zk = case
    g = on_gpu(*case)
    c, dev = g["c"], g["dev"]
    ctx, cs, vk, prm, primary = c["ctx"], c["cs"], c["vk"], c["prm"], g["primary"]
    assert_report(verdict(g, primary, g["proof"]), ACCEPTED)
    dec = list(to_host(dev.enc_decode(g["dsk"], g["proof"])))
    assert verifier_accepts(scheme, ctx, cs, vk, primary, dec)
    bad, word = tampered(g)
    assert not verifier_accepts(scheme, ctx, cs, vk, bad, dec)
    exp = assert_verdict(g, verdict(g, bad, g["proof"]), bad, g["host"])
    check = 0 if scheme == G16 else 5
    assert exp["failed"] == 1 << check and exp["n_bad"][check] == 1 and exp["first"][:3] == (check, prm.L - 1, prm.N - 1)
    assert_verdict(g, verdict(g, primary, dev.put(word)), primary, word)
    last = len(g["host"]) - 1
    e = one_slot(ctx, prm.L - 1, prm.N - 1, 3)
    shifted = g["proof"].clone()
    shifted[last] = dev.enc_add(g["proof"][last].contiguous(), dev.enc_encode(g["dsk"], dev.put(e), 99))
    exp = assert_verdict(g, verdict(g, primary, shifted), primary, to_host(shifted))
    check = 0 if scheme == G16 else 4
    assert exp["failed"] == 1 << check and exp["n_bad"][check] == 1 and exp["first"][:3] == (check, prm.L - 1, prm.N - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", COMPACT, ids=ident)
def test_compact_keys_prove_the_same_statement(case):
    """A seeded and a packed key of the same trapdoor and seeds: other ciphertexts (c1 comes from the public streams), the
    same plaintexts -- accepted, decoded element for element as the full key's proof -- and one proof between them."""
    from ringsnark_amd.device import to_host
    scheme = case[0]
    g = on_gpu(*case)
    c, dev = g["c"], g["dev"]
    pub = disjoint_seeds(5000, len(VECTORS[scheme]))
    proofs = []
    for packed in (False, True):
        pk = device_keygen(dev, scheme, g["dcs"], c["vk"], seeds=c["seeds"], seeded=True, packed=packed, pub_seeds=pub)
        assert bool(pk.get("packed")) == packed
        proof, empty = prove(dev, scheme, g["dcs"], pk, g["dasg"], g["d"])
        assert empty == g["empty"]
        assert_report(verdict(g, g["primary"], proof), ACCEPTED)
        proofs.append(proof)
    assert (to_host(proofs[1]) == to_host(proofs[0])).all()
    assert (to_host(proofs[0]) != g["host"]).any()
    dec = to_host(dev.enc_decode(g["dsk"], proofs[0]))
    for k in range(len(g["host"])):
        assert (dec[k] == g["ref_dec"][k]).all(), k


@pytest.mark.gpu
def test_batched_verification_is_the_single_verifier():
    """C3, five members -- a group of four and a remainder: the proof, a tampered primary input, a proof with one word
    changed, the proof twice more; status, report and least budget of every member are the single verifier's."""
    g = on_gpu(*BATCH)
    dev = g["dev"]
    bad, word = tampered(g)
    dword = dev.put(word)
    members = [(g["primary"], g["proof"]), (bad, g["proof"]), (g["primary"], dword), (g["primary"], g["proof"]), (g["primary"], g["proof"])]
    got = dev.groth16_verify_batch(g["dvk"], [dev.put(x) for x, _ in members], [p for _, p in members], [g["empty"]] * len(members))
    assert len(got) == 5
    singles = [verdict(g, x, p) for x, p in members]
    for b, (x, p) in enumerate(members):
        spent = isinstance(singles[b], str)
        assert got[b].noise_spent == spent and got[b].result == (None if spent else singles[b]), (b, got[b], singles[b])
        assert got[b].budget_min == int(dev.enc_noise_budget(g["dsk"], p).min()), b
    assert [bool(x) for x in got] == [True, False, False, True, True]
    assert_verdict(g, singles[2], g["primary"], word)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEVELS, ids=ident)
def test_every_level_is_the_truncated_context_oracle(case):
    """rs_enc_mod_switch of a real proof to every K_out < K: the words of the mirror (ringsnark_amd/modswitch.py); budget,
    decoding and verdict what the oracle context on Q[:K_out] gives for them -- accepted while that oracle reports budget
    in every limb, refused with the reference's message from the level at which it does not."""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    scheme, name, m, zk = case
    g = on_gpu(*case)
    c, dev = g["c"], g["dev"]
    prm, ctx, cs, vk, primary = c["prm"], c["ctx"], c["cs"], c["vk"], g["primary"]
    dprimary = dev.put(primary)
    sw, refused = g["host"], []
    for K_out in range(prm.K - 1, 0, -1):
        sw = MS.mod_switch(prm, sw, K_out + 1, K_out, MC.oracle_ntt(prm))
        dsw = dev.enc_mod_switch(g["proof"], K_out)
        assert (to_host(dsw) == sw).all(), K_out
        tctx = H.oracle_ctx(MC.truncated(prm, K_out))
        tsk = np.ascontiguousarray(vk["sk"][:K_out])
        budget = np.array([tctx.noise_budget(tsk, e) for e in sw])
        print("%s level %d: budgets %s" % (ident(case), K_out, budget.tolist()))
        assert (dev.enc_noise_budget(g["dsk"], dsw, level=K_out) == budget).all(), K_out
        if (budget > 0).all():
            assert not refused, "a level below a refused one has budget"
            dec = [MS.apply_level_factor(prm, tctx.enc_decode(tsk, e), K_out) for e in sw]
            assert (to_host(dev.enc_decode(g["dsk"], dsw, level=K_out)) == np.stack(dec)).all(), K_out
            assert all((x == y).all() for x, y in zip(dec, g["ref_dec"]))  # a switch keeps the plaintext
            assert S.groth16_verifier(ctx, cs, vk, primary, *dec)
            assert_report(dev.groth16_verify(g["dvk"], dprimary, dsw, g["empty"], level=K_out), ACCEPTED)
            bad, _ = tampered(g)
            exp = expected_report(g16_sides(ctx, cs, vk, bad, dec))
            assert not exp["accepted"]
            assert_report(dev.groth16_verify(g["dvk"], dev.put(bad), dsw, g["empty"], level=K_out), exp)
        else:
            refused.append(K_out)
            k = int(np.argmax((budget <= 0).any(axis=1)))
            with pytest.raises(_lib.RsError) as ei:
                dev.groth16_verify(g["dvk"], dprimary, dsw, g["empty"], level=K_out)
            assert ei.value.code == _lib.RS_ERR_NOISE and NOISE_TEXT % int(np.argmax(budget[k] <= 0)) in str(ei.value)
    assert refused and prm.K - 1 not in refused  # one level at least is free; the guard refuses the lowest
