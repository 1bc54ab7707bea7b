"""Mod-switched encodings and proofs on the device (include/ringsnark_amd/modswitch.h) against the Python mirror
(ringsnark_amd/modswitch.py, on the CPU oracle's transforms) and the CPU oracle's contexts on the truncated prime lists.
Every comparison is integer equality."""
import ctypes
import functools

import numpy as np
import pytest

from ringsnark_amd import modswitch as MS
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests import modswitch_cases as MC

pytestmark = pytest.mark.gpu

NOISE_TEXT = "has remaining noise budget 0 <= 0"


@functools.lru_cache(maxsize=None)
def device_for(name):
    from ringsnark_amd.device import Device
    return Device(P.preset(name))


def enc_threads(n):
    """threads of a workgroup that holds one transform of length n (csrc/rs_internal.hpp: enc_threads)"""
    return max(64, min(1024, n // 8))


def planted_input(prm, K_in, count, seed):
    """[count][L][2][K_in][N_enc]: uniform residues, except that
    * the dropped row K_in - 1 of every polynomial is the transform of a coefficient vector that holds, at the positions 0, 1,
      63, 64, T - 1, T, n / 2, n - 1 (T = enc_threads; those below n), the values 0, 1, p - 1, (p - 1) / 2, t and the largest
      multiple of t below p (where t < p), and p mod t -- the value that makes u = t - 1 (where it is below p) -- each value
      at each position for some (element, component);
    * the rows j < K_in - 1 hold 0 and Q_j - 1 alternately at the same positions."""
    ctx = H.oracle_ctx(prm)
    n, ntt = prm.N_enc, MC.oracle_ntt(prm)
    enc = np.ascontiguousarray(ctx.random_enc(seed, count)[:, :, :, :K_in])
    T = enc_threads(n)
    pos = sorted({x for x in (0, 1, 63, 64, T - 1, T, n // 2, n - 1) if x < n})
    p = int(prm.Q[K_in - 1])
    rng = np.random.RandomState(seed)
    for e in range(count):
        for i, t in enumerate(prm.q):
            t = int(t)
            vals = [0, 1, p - 1, (p - 1) // 2]
            if t < p:
                vals += [t, (p - 1) // t * t, p % t]
                assert (-(p % t) * pow(p, -1, t)) % t == t - 1
            for c in range(2):
                coeff = (rng.randint(0, 2**62, size=n, dtype=np.int64).astype(np.uint64) % np.uint64(p)).astype(np.uint64)
                for k, x in enumerate(pos):
                    coeff[x] = vals[(k + 2 * e + c) % len(vals)]
                enc[e, i, c, K_in - 1] = ntt(p).fwd(coeff)
                for j in range(K_in - 1):
                    for k, x in enumerate(pos):
                        enc[e, i, c, j, x] = 0 if (k + j + c) % 2 == 0 else int(prm.Q[j]) - 1
    return enc


def assert_switch_matches_mirror(dev, prm, enc, K_in, K_out):
    from ringsnark_amd.device import to_host
    want = MS.mod_switch(prm, enc, K_in, K_out, MC.oracle_ntt(prm))
    got = to_host(dev.enc_mod_switch(dev.put(enc), K_out))
    assert got.shape == want.shape
    assert (got == want).all(), (prm.name, K_in, K_out, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "toy54", "toy60"])
def test_mod_switch_is_the_mirror_word_for_word(name):
    """toy, toy49, toy50: the FP64 arithmetic; toy54, toy60: the integer one.  Every (K_in, K_out), count 1 and 5."""
    prm = P.preset(name)
    dev = device_for(name)
    assert (name in ("toy54", "toy60")) == any(p >= 1 << 50 for p in prm.q + prm.Q)
    for count in (1, 5):
        for K_in in range(1, prm.K + 1):
            enc = planted_input(prm, K_in, count, 100 + 10 * count + K_in)
            for K_out in range(1, K_in + 1):
                assert_switch_matches_mirror(dev, prm, enc, K_in, K_out)


@pytest.mark.parametrize("name,K_in,K_outs", [("C2", 4, (3, 2)), ("C5", 8, (7, 6))])
def test_mod_switch_at_8_and_16_coefficients_per_thread(name, K_in, K_outs):
    """C2: N_enc = 8192, 1024 threads, 8 coefficients each; C5: N_enc = 16384, 16 each (and the integer arithmetic)."""
    prm = P.preset(name)
    assert prm.K == K_in and prm.N_enc // enc_threads(prm.N_enc) == (8 if name == "C2" else 16)
    dev = device_for(name)
    enc = planted_input(prm, K_in, 1, 7)
    for K_out in K_outs:
        assert_switch_matches_mirror(dev, prm, enc, K_in, K_out)


@pytest.mark.parametrize("name", MC.PRESETS)
def test_level_decode_and_budget_are_the_truncated_context_oracle(name):
    """On the mirror's switched encodings of tests/test_modswitch.py: the budget of every level is the oracle's, the decoding
    is the oracle's times the level factor -- i.e. the ring element encoded -- and a spent level is refused with the
    reference's message.  Level K gives the words of rs_enc_decode / rs_enc_noise_budget."""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    c = MC.case(name)
    prm, dev = c.prm, device_for(name)
    sk = dev.put(c.sk)
    spent_seen = False
    for kind in MC.KINDS:
        for K_lvl in range(1, prm.K + 1):
            sw = dev.put(c.switched[kind][K_lvl])
            assert (dev.enc_noise_budget(sk, sw, level=K_lvl) == c.budget[kind][K_lvl]).all(), (kind, K_lvl)
            for k in range(MC.COUNT):
                if c.decoded[kind][K_lvl][k] is None:
                    spent_seen = True
                    with pytest.raises(_lib.RsError) as ei:
                        dev.enc_decode(sk, sw[k].contiguous(), level=K_lvl)
                    limb = int(np.argmin(c.budget[kind][K_lvl][k] > 0))
                    assert ei.value.code == _lib.RS_ERR_NOISE and ("ciphertext #%d %s" % (limb, NOISE_TEXT)) in str(ei.value)
                else:
                    got = to_host(dev.enc_decode(sk, sw[k].contiguous(), level=K_lvl))
                    assert (got == MS.apply_level_factor(prm, c.decoded[kind][K_lvl][k], K_lvl)).all(), (kind, K_lvl, k)
                    assert (got == c.ring[kind][k]).all()
        full = dev.put(c.enc[kind])
        assert (to_host(dev.enc_decode(sk, full, level=prm.K)) == to_host(dev.enc_decode(sk, full))).all()
        assert (dev.enc_noise_budget(sk, full, level=prm.K) == dev.enc_noise_budget(sk, full)).all()
    assert spent_seen == (name not in ("toy", "toyR"))


def test_level_wire_format_round_trip():
    """The bytes of a level are those a second context, created on the truncated preset, writes for the same words; they read
    back at their level, decode there, and the full context's rs_enc_deserialize refuses them."""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device, to_host
    c = MC.case("toy")
    prm, dev = c.prm, device_for("toy")
    sk = dev.put(c.sk)
    for K_lvl in range(1, prm.K + 1):
        words = c.switched["product"][K_lvl]
        sw = dev.enc_mod_switch(dev.put(c.enc["product"]), K_lvl)
        assert (to_host(sw) == words).all()
        small = Device(MC.truncated(prm, K_lvl))
        for empty in (None, [1, 0]):
            data = dev.enc_serialize(sw, empty=empty, level=K_lvl)
            assert data == small.enc_serialize(dev.put(words), empty=empty)
            assert data == MS.serialize_level(prm, words, K_lvl, empty)
            back, em, found = dev.enc_deserialize(data, level=0)
            assert found == K_lvl and list(em) == (empty or [0, 0])
            keep = [k for k in range(MC.COUNT) if not em[k]]
            assert (to_host(back)[keep] == words[keep]).all() and all((to_host(back)[k] == 0).all() for k in range(MC.COUNT) if em[k])
            for k in keep:
                assert (to_host(dev.enc_decode(sk, back[k].contiguous(), level=found)) == c.ring["product"][k]).all()
            if K_lvl < prm.K:
                with pytest.raises(_lib.RsError) as ei:
                    dev.enc_deserialize(data)
                assert ei.value.code == _lib.RS_ERR_INVALID
                with pytest.raises(_lib.RsError):
                    dev.enc_deserialize(data, level=K_lvl + 1)
        # a residue beyond its level's prime is refused
        bad = bytearray(dev.enc_serialize(sw, level=K_lvl))
        bad[-8:] = int(prm.Q[K_lvl - 1]).to_bytes(8, "little")
        with pytest.raises(_lib.RsError) as ei:
            dev.enc_deserialize(bytes(bad), level=0)
        assert ei.value.code == _lib.RS_ERR_INVALID and "residue out of range" in str(ei.value)


def trapdoor(scheme, prm, ctx, m, seed):
    """s with s - j a unit for every node j < m, the other elements units, r_y = r_v r_w, the oracle's secret key"""
    rng = np.random.RandomState(seed)
    units = lambda lo: np.stack([(rng.randint(0, 2**62, size=prm.N, dtype=np.int64).astype(np.uint64) % np.uint64(p - lo)) + np.uint64(lo)
                                 for p in prm.q])
    vk = {"s": units(m), "sk": ctx.keygen(5)}
    for k in (("alpha", "beta", "gamma", "delta") if scheme == "groth16" else ("alpha", "beta", "r_v", "r_w")):
        vk[k] = units(1)
    if scheme == "rinocchio":
        vk["r_y"] = ctx.ring_mul(vk["r_v"], vk["r_w"])
    return vk


@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_verify_level_reports_what_verify_reports(scheme):
    """toy, chain circuit, m = 6: key generated on the device, proof switched to every level; at every decodable level the
    report of rs_*_verify_level is field for field that of rs_*_verify on the unswitched proof -- for an honest proof and for
    one proved from a violated assignment; Rinocchio also with its last element flagged EMPTY.  A level past the budget is
    refused with the reference's message, and so is -- or it is rejected -- a switched proof with one word changed."""
    from ringsnark_amd import _lib
    prm = P.preset("toy")
    ctx, dev = H.oracle_ctx(prm), device_for("toy")
    m, n_el = 6, 3 if scheme == "groth16" else 9
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    vk = trapdoor(scheme, prm, ctx, m, 17)
    keygen, make_vk, prove, verify = ((dev.groth16_keygen, dev.groth16_vk, dev.groth16_prove, dev.groth16_verify) if scheme == "groth16" else
                                      (dev.rinocchio_keygen, dev.rinocchio_vk, dev.rinocchio_prove, dev.rinocchio_verify))
    pk, dvk, sk = keygen(dcs, vk, seeds=3), make_vk(dcs, vk), dev.put(vk["sk"])
    honest = H.make_assignment(ctx, cs)
    violated = honest.copy()
    violated[cs.n_inputs + 2, 0, 3] = (int(violated[cs.n_inputs + 2, 0, 3]) + 1) % prm.q[0]
    assert dev.r1cs_check(dcs, dev.put(honest)).satisfied and not dev.r1cs_check(dcs, dev.put(violated)).satisfied
    primary = dev.put(honest[: cs.n_inputs])
    flag_sets = [None] if scheme == "groth16" else [None, [0] * 8 + [1]]
    decodable = 0
    for asg, accepted in ((honest, True), (violated, False)):
        proof, empty = prove(dcs, pk, dev.put(asg), check=False)
        assert empty == [0] * n_el
        for flags in flag_sets:
            ref = verify(dvk, primary, proof, flags)
            assert ref.accepted == accepted
            for K_lvl in range(prm.K, 0, -1):
                sw = dev.enc_mod_switch(proof, K_lvl)
                read = [k for k in range(n_el) if not (flags and flags[k])]
                if (dev.enc_noise_budget(sk, sw, level=K_lvl)[read] > 0).all():
                    decodable += 1
                    assert verify(dvk, primary, sw, flags, level=K_lvl) == ref, (K_lvl, flags)
                    if accepted and flags is None:
                        t = sw.clone()
                        t[1, 0, 0, 0, 2] = (t[1, 0, 0, 0, 2] + 1) % int(prm.Q[0])
                        try:
                            assert not verify(dvk, primary, t, flags, level=K_lvl).accepted
                        except _lib.RsError as e:  # one word of a transform moves every coefficient: the noise guard may fire first
                            assert e.code == _lib.RS_ERR_NOISE and NOISE_TEXT in str(e)
                else:
                    assert K_lvl < prm.K - 1, "level K - 1 must be decodable"
                    with pytest.raises(_lib.RsError) as ei:
                        verify(dvk, primary, sw, flags, level=K_lvl)
                    assert ei.value.code == _lib.RS_ERR_NOISE and NOISE_TEXT in str(ei.value)
    assert decodable >= 2 * len(flag_sets) * 2  # levels K and K - 1 of both proofs at least
    dvk.close()


def test_arguments_are_validated():
    from ringsnark_amd import _lib
    from ringsnark_amd.device import Device, _ptr
    prm = P.preset("toy")
    dev = device_for("toy")
    lib, K = dev.lib, prm.K
    enc = dev.put(MC.case("toy").enc["fresh"])
    out = dev.enc_empty(MC.COUNT)
    call = lambda src, K_in, K_out, dst: lib.rs_enc_mod_switch(dev.h, _ptr(src), MC.COUNT, K_in, K_out, _ptr(dst), dev.stream())
    assert call(enc, K, K, out) == _lib.RS_OK and (out == enc).all()  # K_out == K_in: a copy
    assert call(enc, K - 1, K, out) == _lib.RS_ERR_INVALID   # K_out > K_in
    assert call(enc, K, 0, out) == _lib.RS_ERR_INVALID
    assert call(enc, K + 1, K, out) == _lib.RS_ERR_INVALID   # K_in > K
    assert call(enc, K, K - 1, enc) == _lib.RS_ERR_INVALID   # in place
    both = dev.enc_empty(2 * MC.COUNT)
    flat = both.view(-1)
    half = flat.numel() // 2
    assert call(flat[:half], K, K - 1, flat[half - 8:]) == _lib.RS_ERR_INVALID  # the output begins inside the input
    assert call(flat[half:], K, K - 1, flat[half // 2:]) == _lib.RS_ERR_INVALID  # the output ends inside the input
    assert call(flat[:half], K, K - 1, flat[half:]) == _lib.RS_OK               # adjacent ranges do not overlap
    sk = dev.put(MC.case("toy").sk)
    ring = dev.ring_empty(MC.COUNT)
    budget = (ctypes.c_int * (MC.COUNT * prm.L))()
    for lvl in (0, K + 1):
        assert lib.rs_enc_decode_level(dev.h, lvl, _ptr(sk), _ptr(enc), MC.COUNT, _ptr(ring), dev.stream()) == _lib.RS_ERR_INVALID
        assert lib.rs_enc_noise_budget_level(dev.h, lvl, _ptr(sk), _ptr(enc), MC.COUNT, budget, dev.stream()) == _lib.RS_ERR_INVALID
        assert lib.rs_enc_wire_size_level(dev.h, lvl, 1) == 0
        assert lib.rs_enc_serialize_level(dev.h, lvl, _ptr(enc), None, 0, ctypes.c_void_p(ring.data_ptr()), 0, dev.stream()) == _lib.RS_ERR_INVALID
    # a verification key belongs to its context; a level must be one of the context's
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(3, prm.q)
    dcs = dev.r1cs(cs)
    dvk = dev.groth16_vk(dcs, trapdoor("groth16", prm, ctx, 3, 5))
    other = Device(prm)
    rep = _lib.VerifyReport()
    primary, proof = dev.ring_empty(cs.n_inputs), dev.put(ctx.random_enc(3, 3)[:, :, :, : K - 1])
    args = (_ptr(primary), _ptr(proof), None, rep, None)
    assert lib.rs_groth16_verify_level(other.h, dvk.h, K - 1, *args) == _lib.RS_ERR_INVALID
    assert lib.rs_rinocchio_verify_level(dev.h, dvk.h, K - 1, *args) == _lib.RS_ERR_INVALID  # a key of the other scheme
    assert lib.rs_groth16_verify_level(dev.h, dvk.h, 0, *args) == _lib.RS_ERR_INVALID
    assert lib.rs_groth16_verify_level(dev.h, dvk.h, K + 1, *args) == _lib.RS_ERR_INVALID
    dvk.close()
