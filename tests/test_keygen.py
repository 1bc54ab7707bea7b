"""ringsnark_amd/keygen.h: the two generators (groth16.tcc:5-66, rinocchio.tcc:5-72) on the device.

Everything is exact, so every comparison is equality of uint64 words.  A key vector is compared
  * with the CPU: the rows from tests/snark_ref.py's O(m^2) instance map and the oracle's ring operations in the reference's
    order of operations, encoded by the oracle's encoder with the vector's seed;
  * with the composed device path of existing entry points (instance_map_eval, ring_mul / ring_add, enc_encode), each of
    which has parity tests of its own, where the CPU would be slow (N_enc = 8192) or adds nothing (polynomial coefficients).

The seeds of a key are disjoint (seed + v * 2^40 per vector): snark_ref's seed + 12, seed + 13, ... share streams between
vectors, which the device generator refuses.  The inputs of the end-to-end tests are shown valid on the CPU alone first
(test_keygen_inputs_are_valid_*): a key built from the same formulas with the same disjoint seeds, the oracle's prover, a
positive noise budget in every limb of every proof element, accepted by snark_ref's verifier.  The shapes are those
tests/test_verify.py showed valid (Rinocchio with ZK elements on `toy` only)."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 1 << 40
G16_CASES = [("toy", 6), ("toy49", 12), ("toy50", 12), ("toy60", 6)]  # toy60: the integer (Montgomery) arithmetic
RIN_CASES = [("toy49", 9, False), ("toy50", 9, False), ("toy", 9, True), ("toy60", 9, False)]  # (preset, m, ZK elements set)
G16_VECTORS = ("s_pows", "delta_ts", "delta_mid", "alpha", "beta")
RIN_VECTORS = ("s_pows", "alpha_s_pows", "beta_prods", "beta_rv_ts", "beta_rw_ts", "beta_ry_ts")
VECTORS = {"groth16": G16_VECTORS, "rinocchio": RIN_VECTORS}


def disjoint_seeds(seed, n):
    return [seed + v * STRIDE for v in range(n)]


# ---- trapdoors and rows (CPU) ----------------------------------------------------------------------------------------
def random_units(rng, q, N, lo=1):
    """[L][N] residues in [lo, q_i): units of the ring (every slot non-zero); lo = m: s - j is a unit for every node j < m"""
    return np.stack([(rng.randint(0, 2**62, size=N, dtype=np.int64).astype(np.uint64) % np.uint64(p - lo)) + np.uint64(lo) for p in q])


def trapdoor(scheme, prm, m, seed, sk):
    rng = np.random.RandomState(seed)
    vk = {"s": random_units(rng, prm.q, prm.N, m), "sk": sk}
    names = ("alpha", "beta", "gamma", "delta") if scheme == "groth16" else ("alpha", "beta", "r_v", "r_w")
    for k in names:
        vk[k] = random_units(rng, prm.q, prm.N)
    return vk


def hand_rows():
    """tests/test_verify.py's system: n_inputs = 3 of n_vars = 6; entries of all three matrices on the constant one and on
    the three primary inputs; an empty row in `a`; m = 5."""
    a = [[(0, 2), (1, 1), (4, -1)], [], [(2, 3), (3, 1), (5, 2)], [(0, -1), (6, 1)], [(1, 4), (3, -2)]]
    b = [[(0, 1), (2, 3)], [(1, 1), (3, 5)], [(4, 1)], [(0, 7), (2, -1), (5, 1)], [(3, 1)]]
    c = [[(0, 5), (3, 1), (5, 1)], [(1, -3), (6, 1)], [(0, 1), (2, 2)], [(4, 1)], [(1, 1), (2, 1), (3, 1)]]
    return {"a": a, "b": b, "c": c}


def systems(q):
    out = [("chain%d" % m, R.chain_r1cs(m, q)) for m in (1, 2, 12)]
    out.append(("hand", R.from_rows(5, 6, 3, hand_rows(), q)))
    rows = {"a": [[(1, 1)], [(0, 3), (2, 1)], [(3, 1)]], "b": [[(2, 1)], [(3, 2)], [(0, 1)]], "c": [[(3, 1)], [(1, 1)], [(1, 1), (0, 2)]]}
    out.append(("no_aux", R.from_rows(3, 3, 3, rows, q)))  # every variable is a primary input: delta_mid / beta_prods are empty
    return out


def key_rows(scheme, ctx, cs, vk):
    """The ring elements a generator encodes, per vector, in the reference's order of operations (groth16.tcc:21-55,
    rinocchio.tcc:21-47); rinocchio: sets vk["r_y"] = r_v r_w and vk["Zt"]."""
    Rg = S.Ring(ctx)
    At, Bt, Ct, Ht, Zt = S.instance_map_with_evaluation(Rg, cs, vk["s"])
    empty = np.zeros((0,) + ctx.ring_shape(), dtype=np.uint64)
    stack = lambda xs: np.stack(xs) if xs else empty
    aux = [i + cs.n_inputs + 1 for i in range(cs.n_aux)]
    if scheme == "groth16":
        dinv = Rg.inv(vk["delta"])
        mid = [Rg.mul(Rg.add(Rg.add(Rg.mul(vk["beta"], At[k]), Rg.mul(vk["alpha"], Bt[k])), Ct[k]), dinv) for k in aux]
        return dict(s_pows=np.stack(Ht), delta_ts=np.stack([Rg.mul(Rg.mul(x, Zt), dinv) for x in Ht]), delta_mid=stack(mid),
                    alpha=vk["alpha"][None], beta=vk["beta"][None])
    vk["r_y"] = Rg.mul(vk["r_v"], vk["r_w"])
    vk["Zt"] = Zt
    lin = [Rg.mul(Rg.add(Rg.add(Rg.mul(vk["r_v"], At[k]), Rg.mul(vk["r_w"], Bt[k])), Rg.mul(vk["r_y"], Ct[k])), vk["beta"]) for k in aux]
    bz = Rg.mul(vk["beta"], Zt)
    return dict(s_pows=np.stack(Ht), alpha_s_pows=np.stack([Rg.mul(x, vk["alpha"]) for x in Ht]), beta_prods=stack(lin),
                beta_rv_ts=Rg.mul(bz, vk["r_v"])[None], beta_rw_ts=Rg.mul(bz, vk["r_w"])[None], beta_ry_ts=Rg.mul(bz, vk["r_y"])[None])


def cpu_key(scheme, ctx, cs, vk, seeds):
    """name -> encodings [count][L][2][K][N_enc] by the oracle's encoder"""
    rows = key_rows(scheme, ctx, cs, vk)
    out = {}
    for v, name in enumerate(VECTORS[scheme]):
        out[name] = ctx.enc_encode(vk["sk"], rows[name], seeds[v]) if len(rows[name]) else np.zeros(ctx.enc_shape(0), dtype=np.uint64)
    return out


def as_prover_key(key):
    """single elements without their leading axis, as the provers take them"""
    return {k: (v[0] if k in ("alpha", "beta", "beta_rv_ts", "beta_rw_ts", "beta_ry_ts") else v) for k, v in key.items()}


@functools.lru_cache(maxsize=None)
def e2e_case(scheme, name, m, zk=False):
    """trapdoor, CPU key with disjoint seeds, assignment and the oracle's proof; computed once"""
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    vk = trapdoor(scheme, prm, cs.m, 41 if scheme == "groth16" else 43, ctx.keygen(5))
    seeds = disjoint_seeds(900, len(VECTORS[scheme]))
    pk = as_prover_key(cpu_key(scheme, ctx, cs, vk, seeds))
    d = ctx.random_ring(77, 3) if zk else [None] * 3
    if scheme == "groth16":
        proof, empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
    else:
        proof, empty = O.rinocchio_prove(ctx, H.oracle_cs(cs), pk, asg, d[0], d[1], d[2])
    return dict(prm=prm, ctx=ctx, cs=cs, asg=asg, vk=vk, seeds=seeds, pk=pk, proof=proof, empty=empty, d=d)


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_library_exports_every_function_of_keygen_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ringsnark_amd", "keygen.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.KEYGEN_SIGNATURES) and len(names) == 3
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 104
    # the output structures of the binding have the header's layout: pointers, int (+ 4 padding), size_t
    assert C.sizeof(_lib.Groth16KeyOut) == 56 and _lib.Groth16KeyOut.tile.offset == 48
    assert C.sizeof(_lib.RinocchioKeyOut) == 64 and _lib.RinocchioKeyOut.tile.offset == 56


def test_snark_ref_seeds_share_streams_and_disjoint_seeds_do_not():
    """why the tests do not reuse snark_ref's seeds: seed + 12 and seed + 13 give ranges 65537 apart, shorter vectors aside"""
    ranges = lambda seeds, lens: [((s * 65537) % 2**64, n) for s, n in zip(seeds, lens)]
    meet = lambda r: any(a < b + nb and b < a + na for i, (a, na) in enumerate(r) for (b, nb) in r[:i])
    lens = [2**17 + 1, 2**17 + 1, 2**17, 1, 1]
    assert meet(ranges([21 + 12, 21 + 14, 21 + 13, 21 + 10, 21 + 11], lens))
    assert not meet(ranges(disjoint_seeds(21, 5), lens))


@pytest.mark.parametrize("name,m", G16_CASES)
def test_keygen_inputs_are_valid_by_the_reference_groth16(name, m):
    c = e2e_case("groth16", name, m)
    ctx, vk, cs = c["ctx"], c["vk"], c["cs"]
    assert c["empty"] == [0, 0, 0]
    for k in range(3):
        assert min(ctx.noise_budget(vk["sk"], c["proof"][k])) > 0
    dec = [ctx.enc_decode(vk["sk"], c["proof"][k]) for k in range(3)]
    assert S.groth16_verifier(ctx, cs, vk, c["asg"][: cs.n_inputs], *dec)


@pytest.mark.parametrize("name,m,zk", RIN_CASES)
def test_keygen_inputs_are_valid_by_the_reference_rinocchio(name, m, zk):
    c = e2e_case("rinocchio", name, m, zk)
    ctx, vk, cs = c["ctx"], c["vk"], c["cs"]
    assert c["empty"] == [0] * 9
    for k in range(9):
        assert min(ctx.noise_budget(vk["sk"], c["proof"][k])) > 0
    dec = [ctx.enc_decode(vk["sk"], c["proof"][k]) for k in range(9)]
    ok, checks = S.rinocchio_verifier(ctx, cs, vk, c["asg"][: cs.n_inputs], dec)
    assert ok, checks


# ---- GPU helpers -----------------------------------------------------------------------------------------------------
def device_for(name):
    from ringsnark_amd.device import Device
    return Device(P.preset(name))


def device_keygen(dev, scheme, dcs, vk, **kw):
    return (dev.groth16_keygen if scheme == "groth16" else dev.rinocchio_keygen)(dcs, vk, **kw)


def key_words(dev, v):
    """a key vector (device tensor, HostWords or None) as uint64 words"""
    from ringsnark_amd.device import HostWords, to_host
    if v is None:
        return np.zeros(0, dtype=np.uint64)
    return np.array(v.array) if isinstance(v, HostWords) else to_host(v).reshape(-1)


def composed_key(dev, scheme, dcs, vk, seeds):
    """The parent's way on the device: rs_instance_map_eval, ring operations, one rs_enc_encode per vector."""
    put = lambda a: dev.put(a)
    At, Bt, Ct, Ht, Zt = dev.instance_map_eval(dcs, put(vk["s"]))
    k0, n_aux, sk = dcs.n_inputs + 1, dcs.n_vars - dcs.n_inputs, put(vk["sk"])
    rep = lambda e, n: e.unsqueeze(0).expand(n, dev.L, dev.N).contiguous()
    mul_by = lambda rows, e: dev.ring_mul(rows.contiguous(), rep(e, rows.shape[0]))
    if scheme == "groth16":
        alpha, beta = put(vk["alpha"]), put(vk["beta"])
        dinv = dev.ring_inv(put(vk["delta"]))
        rows = dict(s_pows=Ht, delta_ts=mul_by(mul_by(Ht, Zt), dinv), alpha=alpha[None], beta=beta[None])
        if n_aux:
            t = dev.ring_add(dev.ring_add(mul_by(At[k0:], beta), mul_by(Bt[k0:], alpha)), Ct[k0:].contiguous())
            rows["delta_mid"] = mul_by(t, dinv)
    else:
        alpha, beta, rv, rw = (put(vk[k]) for k in ("alpha", "beta", "r_v", "r_w"))
        ry = dev.ring_mul(rv, rw)
        bz = dev.ring_mul(beta, Zt)
        rows = dict(s_pows=Ht, alpha_s_pows=mul_by(Ht, alpha), beta_rv_ts=dev.ring_mul(bz, rv)[None], beta_rw_ts=dev.ring_mul(bz, rw)[None],
                    beta_ry_ts=dev.ring_mul(bz, ry)[None])
        if n_aux:
            t = dev.ring_add(dev.ring_add(mul_by(At[k0:], rv), mul_by(Bt[k0:], rw)), mul_by(Ct[k0:], ry))
            rows["beta_prods"] = mul_by(t, beta)
    out = {}
    for v, name in enumerate(VECTORS[scheme]):
        out[name] = dev.enc_encode(sk, rows[name].contiguous(), seeds[v]) if name in rows else None
    return out


def with_r_y(scheme, vk, q):
    """rinocchio: r_y = r_v r_w (rinocchio.tcc:15)"""
    if scheme == "rinocchio" and "r_y" not in vk:
        vk["r_y"] = np.stack([(vk["r_v"][l].astype(object) * vk["r_w"][l].astype(object) % int(p)).astype(np.uint64) for l, p in enumerate(q)])
    return vk


def assert_same_key(dev, scheme, got, exp):
    for name in VECTORS[scheme]:
        g, e = key_words(dev, got[name]), (exp[name].reshape(-1) if isinstance(exp[name], np.ndarray) else key_words(dev, exp[name]))
        assert g.shape == e.shape, (name, g.shape, e.shape)
        assert (g == e).all(), name


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "toy60"])
def test_key_bytes_match_the_cpu(name, scheme):
    """Every vector equals the oracle's encoding of the rows the reference's formulas give: m = 1, 2, 12, entries on the
    constant one and on inputs with an empty row, and no auxiliary variable at all (the third vector is NULL)."""
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    dev = device_for(name)
    for label, cs in systems(prm.q):
        vk = trapdoor(scheme, prm, cs.m, 11, ctx.keygen(3))
        seeds = disjoint_seeds(700, len(VECTORS[scheme]))
        exp = cpu_key(scheme, ctx, cs, vk, seeds)  # sets r_y
        got = device_keygen(dev, scheme, dev.r1cs(cs), vk, seeds=seeds)
        if cs.n_aux == 0:
            assert got[VECTORS[scheme][2]] is None
        assert_same_key(dev, scheme, got, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_polynomial_coefficients_match_the_composed_path(scheme):
    prm = P.preset("toy")
    dev = device_for("toy")
    sk = H.oracle_ctx(prm).keygen(3)
    for m in (1, 4):  # 1: the smallest system wide_poly_r1cs builds
        cs = R.wide_poly_r1cs(m, prm.q, prm.N)
        assert cs.poly_table is not None
        vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 12, sk), prm.q)
        seeds = disjoint_seeds(300, len(VECTORS[scheme]))
        dcs = dev.r1cs(cs)
        assert_same_key(dev, scheme, device_keygen(dev, scheme, dcs, vk, seeds=seeds), composed_key(dev, scheme, dcs, vk, seeds))


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_sixteen_coefficients_per_thread_match_the_composed_path(scheme):
    """C2: N_enc = 8192 on 512 threads (16 coefficients per thread), K = 4.  The secret key only has to be K rows of
    residues for the bytes to be comparable."""
    prm = P.preset("C2")
    assert prm.N_enc == 8192 and prm.K == 4
    dev = device_for("C2")
    rng = np.random.RandomState(2)
    sk = np.stack([rng.randint(0, 2**62, size=prm.N_enc, dtype=np.int64).astype(np.uint64) % np.uint64(Q) for Q in prm.Q])
    cs = R.chain_r1cs(3, prm.q)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 13, sk), prm.q)
    seeds = disjoint_seeds(500, len(VECTORS[scheme]))
    dcs = dev.r1cs(cs)
    assert_same_key(dev, scheme, device_keygen(dev, scheme, dcs, vk, seeds=seeds), composed_key(dev, scheme, dcs, vk, seeds))


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_host_key_streaming_crosses_tile_boundaries(scheme):
    """22 rows: tiles of 8 (two full, one partial), of 1, and one tile of 64; host vectors == device vectors == composed."""
    from ringsnark_amd.device import HostWords
    prm = P.preset("toy")
    dev = device_for("toy")
    cs = R.chain_r1cs(21, prm.q)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 14, H.oracle_ctx(prm).keygen(3)), prm.q)
    seeds = disjoint_seeds(100, len(VECTORS[scheme]))
    dcs = dev.r1cs(cs)
    resident = device_keygen(dev, scheme, dcs, vk, seeds=seeds)
    assert_same_key(dev, scheme, resident, composed_key(dev, scheme, dcs, vk, seeds))
    for tile in (8, 1, 64, 0):
        got = device_keygen(dev, scheme, dcs, vk, seeds=seeds, host=True, tile=tile)
        for v, name in enumerate(VECTORS[scheme]):
            assert isinstance(got[name], HostWords) == (v < 3), name
        assert_same_key(dev, scheme, got, resident)


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("name,m", G16_CASES)
def test_groth16_generate_prove_verify(name, m, host):
    from ringsnark_amd.device import to_host
    c = e2e_case("groth16", name, m)
    prm, cs, asg, vk = c["prm"], c["cs"], c["asg"], c["vk"]
    dev = device_for(name)
    dcs = dev.r1cs(cs)
    pk = dev.groth16_keygen(dcs, vk, seeds=c["seeds"], host=host, tile=4)
    proof, empty = dev.groth16_prove(dcs, pk, dev.put(asg), check=True)
    assert empty == c["empty"] and (to_host(proof) == c["proof"]).all()  # the CPU's key, the CPU's proof
    dvk = dev.groth16_vk(dcs, vk)
    primary = asg[: cs.n_inputs]
    assert dev.groth16_verify(dvk, dev.put(primary), proof, empty).accepted
    bad = primary.copy()
    bad[1, prm.L - 1, 5] = (int(bad[1, prm.L - 1, 5]) + 1) % prm.q[prm.L - 1]
    got = dev.groth16_verify(dvk, dev.put(bad), proof, empty)
    assert not got.accepted and got.n_bad[0] == 1 and (got.first_limb, got.first_slot) == (prm.L - 1, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("name,m,zk", RIN_CASES)
def test_rinocchio_generate_prove_verify(name, m, zk):
    from ringsnark_amd.device import to_host
    c = e2e_case("rinocchio", name, m, zk)
    prm, cs, asg, vk = c["prm"], c["cs"], c["asg"], c["vk"]
    dev = device_for(name)
    dcs = dev.r1cs(cs)
    pk = dev.rinocchio_keygen(dcs, vk, seeds=c["seeds"])
    d = [None if x is None else dev.put(x) for x in c["d"]]
    proof, empty = dev.rinocchio_prove(dcs, pk, dev.put(asg), d[0], d[1], d[2], check=True)
    assert empty == c["empty"] and (to_host(proof) == c["proof"]).all()
    dvk = dev.rinocchio_vk(dcs, vk)
    primary = asg[: cs.n_inputs]
    assert dev.rinocchio_verify(dvk, dev.put(primary), proof, empty).accepted
    bad = primary.copy()
    bad[0, prm.L - 1, 2] = (int(bad[0, prm.L - 1, 2]) + 1) % prm.q[prm.L - 1]
    got = dev.rinocchio_verify(dvk, dev.put(bad), proof, empty)
    assert not got.accepted and got.failed == 1 << 5 and (got.first_limb, got.first_slot) == (prm.L - 1, 2)


PATTERN = 0x5A5A5A5A5A5A5A5A


def raw_keygen(dev, scheme, dcs, vk, seeds):
    """The C entry point on output buffers filled with a pattern: (status, message, every output still holds the pattern)."""
    import torch
    from ringsnark_amd import _lib
    from ringsnark_amd.device import _ptr
    m, n_aux = dcs.m, dcs.n_vars - dcs.n_inputs
    lens = [m + 1, m + 1, n_aux] + [1] * (len(VECTORS[scheme]) - 3)
    outs = [torch.full((max(n, 1), dev.L, 2, dev.K, dev.N_enc), PATTERN, dtype=torch.int64, device=dev.device) for n in lens]
    t = {k: dev.put(v) for k, v in vk.items() if k != "Zt"}
    hs = (C.c_uint64 * len(lens))(*[(s * 65537) % 2**64 for s in seeds])
    dev.sync()
    if scheme == "groth16":
        out = _lib.Groth16KeyOut(*[o.data_ptr() for o in outs], 0, 0)
        st = dev.lib.rs_groth16_keygen(dev.h, dcs.h, _ptr(t["s"]), _ptr(t["alpha"]), _ptr(t["beta"]), _ptr(t["delta"]), _ptr(t["sk"]), hs,
                                       C.byref(out), None)
    else:
        out = _lib.RinocchioKeyOut(*[o.data_ptr() for o in outs], 0, 0)
        st = dev.lib.rs_rinocchio_keygen(dev.h, dcs.h, *[_ptr(t[k]) for k in ("s", "alpha", "beta", "r_v", "r_w", "r_y", "sk")], hs,
                                         C.byref(out), None)
    return st, dev.lib.rs_last_error().decode(), all(bool((o == PATTERN).all()) for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_errors_leave_the_outputs_untouched(scheme):
    from ringsnark_amd import _lib
    prm = P.preset("toy")
    dev = device_for("toy")
    cs = R.chain_r1cs(6, prm.q)
    dcs = dev.r1cs(cs)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 15, H.oracle_ctx(prm).keygen(3)), prm.q)
    nv = len(VECTORS[scheme])
    good = disjoint_seeds(50, nv)
    st, _, untouched = raw_keygen(dev, scheme, dcs, vk, good)
    assert st == _lib.RS_OK and not untouched
    # seed ranges that intersect, in the seed WORDS of the C interface: s_pows covers the streams [h0, h0 + m + 1)
    hs = [(x * 65537) % 2**64 for x in good]
    for v, w, off in ((1, 0, cs.m),      # the second vector starts on the last stream of s_pows
                      (1, 0, 0),         # the same seed twice
                      (nv - 1, 1, 3),    # a single element inside the second vector
                      (0, 3, -cs.m)):    # the last stream of s_pows is a single element's
        words = list(hs)
        words[v] = (hs[w] + off) % 2**64
        st, msg, untouched = raw_keygen_words(dev, scheme, dcs, vk, words)
        assert st == _lib.RS_ERR_INVALID and "intersect" in msg and untouched, (v, w, off, st, msg)
    words = list(hs)
    words[1], words[3] = 2**64 - 2, 1  # the streams of a vector wrap around 2^64 as the kernel's seed + k does
    st, msg, untouched = raw_keygen_words(dev, scheme, dcs, vk, words)
    assert st == _lib.RS_ERR_INVALID and "intersect" in msg and untouched
    # one stream past the end of s_pows is fine
    words = list(hs)
    words[1] = hs[0] + cs.m + 1
    assert raw_keygen_words(dev, scheme, dcs, vk, words)[0] == _lib.RS_OK
    # s = RingT(j): the error of rs_instance_map_eval
    bad = dict(vk)
    bad["s"] = np.full((prm.L, prm.N), 2, dtype=np.uint64)
    st, msg, untouched = raw_keygen(dev, scheme, dcs, bad, good)
    assert st == _lib.RS_ERR_NOT_INVERTIBLE and "t cannot be one of the values in the domain" in msg and untouched
    if scheme == "groth16":  # delta with one zero slot
        bad = dict(vk)
        bad["delta"] = vk["delta"].copy()
        bad["delta"][prm.L - 1, 2] = 0
        st, msg, untouched = raw_keygen(dev, scheme, dcs, bad, good)
        assert st == _lib.RS_ERR_NOT_INVERTIBLE and "element is not invertible in ring" in msg and untouched
    # null arguments
    assert dev.lib.rs_groth16_keygen(dev.h, dcs.h, None, None, None, None, None, None, None, None) == _lib.RS_ERR_INVALID
    assert dev.lib.rs_rinocchio_keygen(None, dcs.h, None, None, None, None, None, None, None, None, None, None) == _lib.RS_ERR_INVALID


def raw_keygen_words(dev, scheme, dcs, vk, words):
    """raw_keygen with the seed WORDS of the C interface (no multiplication by 65537)"""
    inv = pow(65537, -1, 2**64)
    return raw_keygen(dev, scheme, dcs, vk, [(w * inv) % 2**64 for w in words])


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_keygen_is_deterministic_on_any_stream(scheme):
    import torch
    prm = P.preset("toy49")
    dev = device_for("toy49")
    cs = R.chain_r1cs(5, prm.q)
    dcs = dev.r1cs(cs)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 16, H.oracle_ctx(prm).keygen(3)), prm.q)
    first = device_keygen(dev, scheme, dcs, vk, seeds=77)  # one integer: seed + v * 2^40 per vector
    assert_same_key(dev, scheme, device_keygen(dev, scheme, dcs, vk, seeds=77), first)
    assert_same_key(dev, scheme, device_keygen(dev, scheme, dcs, vk, seeds=disjoint_seeds(77, len(VECTORS[scheme]))), first)
    stream = torch.cuda.Stream(device=dev.device)
    with torch.cuda.stream(stream):
        other = device_keygen(dev, scheme, dcs, vk, seeds=77)
        hosted = device_keygen(dev, scheme, dcs, vk, seeds=77, host=True, tile=2)
    stream.synchronize()
    assert_same_key(dev, scheme, other, first)
    assert_same_key(dev, scheme, hosted, first)
    different = device_keygen(dev, scheme, dcs, vk, seeds=78)
    assert (key_words(dev, different["s_pows"]) != key_words(dev, first["s_pows"])).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy", "toy60"])
def test_encode_linear_is_enc_encode_on_plain_rows(name):
    """one term, no coefficient: the bytes of rs_enc_encode; three terms: the encoding of the sum of products"""
    from ringsnark_amd.device import to_host
    prm = P.preset(name)
    ctx = H.oracle_ctx(prm)
    dev = device_for(name)
    sk = dev.put(ctx.keygen(3))
    rows = [dev.put(ctx.random_ring(20 + r, 5)) for r in range(3)]
    coefs = [dev.put(ctx.random_ring(30 + r)) for r in range(3)]
    assert (to_host(dev.enc_encode_linear(sk, rows[:1], 9)) == to_host(dev.enc_encode(sk, rows[0], 9))).all()
    rep = lambda e: e.unsqueeze(0).expand(5, dev.L, dev.N).contiguous()
    total = dev.ring_add(dev.ring_add(dev.ring_mul(rows[0], rep(coefs[0])), rows[1]), dev.ring_mul(rows[2], rep(coefs[2])))
    got = dev.enc_encode_linear(sk, rows, 9, coefs=[coefs[0], None, coefs[2]])
    assert (to_host(got) == to_host(dev.enc_encode(sk, total, 9))).all()
