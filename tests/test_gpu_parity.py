"""HIP path vs the CPU oracle, through the C ABI (librs_hip.so).  Bit-exact: every comparison is
an integer array equality.  Needs a real MI355X: run with -m gpu."""
import contextlib

import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import _lib
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H

pytestmark = pytest.mark.gpu

_DEV = {}


def _params(name):
    """A preset, or one of the custom contexts of tests/helpers.py (WORST_CASES: the 50-bit primes at 8192 and 16384 points)"""
    return H.worst_case_params(name) if name in H.WORST_CASES and H.WORST_CASES[name] is not None else P.preset(name)


def dev_for(name):
    """Device per preset.  "<preset>+int": the same preset on the integer (Montgomery) arithmetic, which contexts
    otherwise select only when a modulus is >= 2^50 (tuning knob force_int_arith, read at context creation)."""
    from ringsnark_amd.device import Device
    if name not in _DEV:
        base, force = (name[:-4], True) if name.endswith("+int") else (name, False)
        with _lib.tuning(**(dict(force_int_arith=1) if force else {})):
            _DEV[name] = Device(_params(base))
    return _DEV[name]


def host(t):
    from ringsnark_amd.device import to_host
    return to_host(t)


@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "C2", "C3", "C5s", "C4", "toy54", "toy60", "micro60", "C5", "toy+int", "toy49+int"])
def test_ntt_matches_oracle(name):
    dev = dev_for(name)
    prm = dev.prm
    logn = prm.N_enc.bit_length() - 1
    rng = np.random.RandomState(1)
    for modset, primes in ((_lib.RS_MOD_PLAIN, prm.q), (_lib.RS_MOD_COEFF, prm.Q)):
        for idx, p in enumerate(primes):
            t = O.NTT(logn, p)
            batch = 3 if prm.N_enc < 16384 else 5  # the persistent wide kernels: more polynomials than one per workgroup slot are in tests/test_launch_paths.py
            a = (rng.randint(0, 2**62, size=(batch, prm.N_enc), dtype=np.int64).astype(np.uint64)) % np.uint64(p)
            a[0, :4] = [0, 1, p - 1, p // 2]
            d = dev.put(a)
            dev.ntt(d, modset, idx)
            got = host(d)
            for b in range(batch):
                assert (got[b] == t.fwd(a[b])).all(), (name, modset, idx, b)
            dev.ntt(d, modset, idx, inverse=True)
            assert (host(d) == a).all()


_NTT_STRUCTURED = {}


def _structured_ntt_cases(name):
    """[(modset, index, inputs [7][n], forward [7][n], inverse [7][n])] per prime of the preset, oracle side, built once."""
    if name not in _NTT_STRUCTURED:
        prm = _params(name)
        n, logn = prm.N_enc, prm.N_enc.bit_length() - 1
        sets = ((_lib.RS_MOD_PLAIN, prm.q), (_lib.RS_MOD_COEFF, prm.Q)) if name != "C5s" else ((_lib.RS_MOD_COEFF, prm.Q),)
        out = []
        for modset, primes in sets:
            for idx, p in enumerate(primes):
                a = np.zeros((7, n), dtype=np.uint64)
                a[0] = p - 1
                a[1] = (p - 1) // 2
                a[2, 1::2] = p - 1
                for row, pos in zip(range(3, 7), (0, 1, n // 2, n - 1)):  # unit impulses: the output is a row of twiddles
                    a[row, pos] = 1
                t = O.NTT(logn, p)
                out.append((modset, idx, a, np.stack([t.fwd(x) for x in a]), np.stack([t.inv(x) for x in a])))
        _NTT_STRUCTURED[name] = out
    return _NTT_STRUCTURED[name]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("variant", [0, 12, 14])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("name", ["toy49", "toy50", "C2", "n8192q50", "C5s", "n16384q50"])
def test_ntt_structured_inputs_match_oracle(name, inverse, variant, batch):
    """The standalone transforms on inputs where an error cannot average out: all p - 1, all (p - 1) / 2, alternating
    0, p - 1, and a unit impulse at 0, 1, n / 2 and n - 1 -- its transform is a row of twiddles, so a wrong table index is a
    wrong value.  128, 8192 and 16384 points (C5s: the data primes), both directions, the barrier, wave-private and wide
    kernels (ntt_variant 0, 12, 14), one polynomial per launch and three.  toy50, n8192q50, n16384q50: the same sizes on
    primes just below 2^50, where the reduction masks allow no stage without a reduction (lim = 2^50 / p is about 1) and
    all p - 1 and alternating 0, p - 1 sit on the bounds the masks are built for."""
    dev = dev_for(name)
    with _lib.tuning(ntt_variant=variant):
        for modset, idx, a, fwd, inv in _structured_ntt_cases(name):
            exp = inv if inverse else fwd
            for r0 in range(0, 7, batch):
                rows = [(r0 + k) % 7 for k in range(batch)]
                d = dev.put(np.ascontiguousarray(a[rows]))
                dev.ntt(d, modset, idx, inverse=inverse)
                assert (host(d) == exp[rows]).all(), (name, modset, idx, rows)


def test_ntt_variants_select_three_kernels_with_equal_results():
    """ntt_variant 0 / 8..13 / 14 = barrier / wave-private / wide kernel.  2^5 points run the barrier kernel whatever the
    knob, 2^11 the wave-private one from 8 on, 2^13 the wide ones at 14: every value gives the same bits and the round trip
    returns the input; at 2^13 the profile shows one kernel for 8 and 12 and another for 14."""
    import torch
    from ringsnark_amd.device import Device
    for logn, prm in ((5, P.make_params(16, [30], 32, [40], ring_factor=1 << 12)), (11, P.make_params(1024, [30], 2048, [43])),
                      (13, P.preset("C2"))):
        assert prm.N_enc == 1 << logn
        dev = dev_for("C2") if logn == 13 else Device(prm)
        src = torch.empty((3, prm.N_enc), dtype=torch.int64, device=dev.device).random_(0, int(prm.Q[0]))
        fwd, kernels = {}, {}
        dev.set_profiling(True)
        try:
            for v in (0, 8, 12, 14):
                with _lib.tuning(ntt_variant=v):
                    d = src.clone()
                    dev.profile_read()
                    dev.ntt(d, _lib.RS_MOD_COEFF, 0)
                    kernels[v] = [(k["name"], k["launches"]) for k in dev.profile_read()]
                    fwd[v] = d.clone()
                    dev.ntt(d, _lib.RS_MOD_COEFF, 0, inverse=True)
                    assert (d == src).all(), ("roundtrip", logn, v)
        finally:
            dev.set_profiling(False)
        for v in fwd:
            assert (fwd[v] == fwd[0]).all(), (logn, v)
            assert len(kernels[v]) == 1 and kernels[v][0][1] == 1, (logn, v, kernels[v])  # one launch of one kernel
        if logn == 5:
            assert kernels[0] == kernels[8] == kernels[12] == kernels[14], kernels
        elif logn == 11:
            assert kernels[8] == kernels[12] == kernels[14] and kernels[0] != kernels[8], kernels
        else:
            assert kernels[8] == kernels[12] and kernels[14] != kernels[8] and kernels[0] != kernels[8], kernels


@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "C2", "toy54", "toy60", "micro60", "toy+int"])
def test_ring_ops_match_oracle(name):
    dev = dev_for(name)
    ctx = H.oracle_ctx(dev.prm)
    a, b = ctx.random_ring(11, 5), ctx.random_ring(12, 5)
    a[0, :, :3] = 0
    b[1] = 0
    da, db = dev.put(a), dev.put(b)
    assert (host(dev.ring_add(da, db)) == ctx.ring_add(a, b)).all()
    assert (host(dev.ring_sub(da, db)) == ctx.ring_sub(a, b)).all()
    assert (host(dev.ring_mul(da, db)) == ctx.ring_mul(a, b)).all()
    assert (host(dev.ring_neg(da)) == ctx.ring_neg(a)).all()
    for s in (0, 1, 3, 2**40 + 12345, 2**63 + 99):
        assert (host(dev.ring_mul_scalar(da, s)) == ctx.ring_mul_scalar(a, s)).all()
    assert dev.ring_is_zero(db) == [False, True, False, False, False]
    inv_in = ctx.random_ring(13, 2)
    inv_in[inv_in == 0] = 1
    exp, ok = ctx.ring_inv(inv_in)
    assert ok and (host(dev.ring_inv(dev.put(inv_in))) == exp).all()
    from ringsnark_amd._lib import RsError, RS_ERR_NOT_INVERTIBLE
    with pytest.raises(RsError) as ei:
        dev.ring_inv(da)  # has zero slots
    assert ei.value.code == RS_ERR_NOT_INVERTIBLE and "not invertible in ring" in str(ei.value)


@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "C2", "toy54", "toy60", "toy49+int"])
def test_batch_encode_and_enc_ops(name):
    dev = dev_for(name)
    ctx = H.oracle_ctx(dev.prm)
    r = ctx.random_ring(21, 2)
    got = host(dev.batch_encode(dev.put(r)))
    for k in range(2):
        for i in range(ctx.L):
            assert (got[k, i] == ctx.batch_encode(i, r[k, i])).all()
    e = ctx.random_enc(22, 2)
    de = dev.put(e)
    got = host(dev.enc_mul_ring(de, dev.put(r)))
    for k in range(2):
        assert (got[k] == ctx.enc_mul_ring(e[k], r[k])).all()
    assert (host(dev.enc_add(de[0], de[1])) == ctx.enc_add(e[0], e[1])).all()


@pytest.mark.parametrize("name,T", [("toy", 1), ("toy", 37), ("toy49", 50), ("toy50", 50), ("C2", 5), ("toy54", 37), ("toy60", 50), ("C5", 3),
                                    ("toy+int", 37), ("toy49+int", 20), ("C4", 5), ("C5s", 40)])
def test_inner_product_matches_oracle(name, T):
    dev = dev_for(name)
    ctx = H.oracle_ctx(dev.prm)
    encs, rings = ctx.random_enc(31, T), ctx.random_ring(32, T)
    kinds = np.zeros(T, dtype=np.uint8)
    if T > 4:
        rings[2] = 0           # is_zero term: skipped
        rings[3, 0] = 0        # one limb zero only: NOT skipped
        kinds[4] = O.KIND_ONE  # Scalar-1 fast path
    exp, used = ctx.inner_product(encs, rings, kinds)
    got, gused = dev.inner_product(dev.put(encs), dev.put(rings), kinds)
    assert gused == used
    assert (host(got) == exp).all()
    # all-zero -> EMPTY
    got0, u0 = dev.inner_product(dev.put(encs), dev.put(np.zeros_like(rings)))
    assert u0 == 0 and not host(got0).any()


def test_grouped_msm_equals_sum_of_inner_products():
    dev = dev_for("toy")
    ctx = H.oracle_ctx(dev.prm)
    T = 23
    crs0, crs1 = ctx.random_enc(41, T), ctx.random_enc(42, T)
    v = [ctx.random_ring(43 + k, T) for k in range(3)]
    vshort = ctx.random_ring(47, T - 5)
    # one CRS, two groups: {v0, v1} and {v2, vshort}
    out, _ = dev.msm([dev.put(crs0)], [(dev.put(v[0]), None, 0), (dev.put(v[1]), None, 0), (dev.put(v[2]), None, 1),
                                       (dev.put(vshort), None, 1)], 2)
    e0 = ctx.enc_add(ctx.inner_product(crs0, v[0])[0], ctx.inner_product(crs0, v[1])[0])
    e1 = ctx.enc_add(ctx.inner_product(crs0, v[2])[0], ctx.inner_product(crs0[: T - 5], vshort)[0])
    got = host(out)
    assert (got[0, 0] == e0).all() and (got[0, 1] == e1).all()
    # two CRS vectors sharing the plaintext transforms
    out, used = dev.msm([dev.put(crs0), dev.put(crs1)], [(dev.put(v[0]), None, 0), (dev.put(v[2]), None, 1)], 2, want_used=True)
    got = host(out)
    assert used == [T, T]
    for c, crs in enumerate((crs0, crs1)):
        assert (got[c, 0] == ctx.inner_product(crs, v[0])[0]).all()
        assert (got[c, 1] == ctx.inner_product(crs, v[2])[0]).all()


@pytest.mark.parametrize("name", ["C5s", "C4", "C5"])
def test_quarter_spectrum_mac_at_16384_points(name):
    """C5: the HYBRID case -- the 54-bit ring prime of the reference's logistic-regression benchmark keeps the ring side
    on the integer arithmetic, the 48 / 49-bit data primes keep the FP64 multiply-accumulate (rows handed over as exact
    doubles).  N_enc = 16384 on the FP64 arithmetic (the shapes of BASELINE configs[3] / [4], microbench.cpp:13-14): the inner
    products run through mac_kernel_v3<false, 14> (a workgroup per quarter of the spectrum, two stages applied while the
    row is loaded).  Two groups sharing a key vector, a second key vector, enough terms for several per chunk and an
    accumulating second tile (tiled key), against the oracle; and against the generic kernel (mac_variant = 1)."""
    dev = dev_for(name)
    prm = dev.prm
    assert prm.N_enc == 16384
    ctx = H.oracle_ctx(prm)
    T = 24 if name == "C4" else 70
    crs0, crs1 = ctx.random_enc(41, 8), ctx.random_enc(42, 8)  # windows of 8 elements
    v = [ctx.random_ring(43 + k, T) for k in range(3)]
    v[1][3] = 0
    dv = [dev.put(x) for x in v]
    # C5: one vector per group -- two lifts of a 54-bit prime do not add up inside 2^53, and such a group keeps the
    # integer multiply-accumulate (checked at the end)
    groups = [(dv[0], None, 0), (dv[1], None, 1), (dv[2], None, 2 if name == "C5" else 1)]
    ng = 3 if name == "C5" else 2
    dev.set_profiling(True)
    out, used = dev.msm([dev.put(crs0)], groups, ng, want_used=True, crs_len=T, window=8)
    names = {k["name"] for k in dev.profile_read()}
    dev.set_profiling(False)
    assert "mac_kernel_v3<false, 14>" in names, names
    got = host(out)
    e = [ctx.inner_product(crs0, v[k], threads=0, window=8)[0] for k in range(3)]
    assert used == [T, T - 1, T] and (got[0, 0] == e[0]).all()
    if name == "C5":
        assert (got[0, 1] == e[1]).all() and (got[0, 2] == e[2]).all()
    else:
        assert (got[0, 1] == ctx.enc_add(e[1], e[2])).all()
    out2, _ = dev.msm([dev.put(crs0), dev.put(crs1)], [(dv[0], None, 0)], 1, crs_len=T, window=8)
    assert (host(out2)[0, 0] == e[0]).all() and (host(out2)[1, 0] == ctx.inner_product(crs1, v[0], threads=0, window=8)[0]).all()
    # Two key vectors (Rinocchio's s_pows / alpha_s_pows, rinocchio.tcc:106-160): mac_kernel_v4 computes a term's plaintext
    # spectrum once for both.  Three groups in one launch, one of them shorter; against the oracle and the per-key kernels.
    short = T - 7
    g2 = [(dv[0], None, 0), (dv[1], None, 1), (dev.put(v[2][:short]), None, 2)]
    dev.set_profiling(True)
    out4, used4 = dev.msm([dev.put(crs0), dev.put(crs1)], g2, 3, want_used=True, crs_len=T, window=8)
    names = {k["name"] for k in dev.profile_read()}
    dev.set_profiling(False)
    assert "mac_kernel_v4<14, false>" in names, names
    got4 = host(out4)
    assert used4 == [T, T - 1, short]
    for c, crs in enumerate((crs0, crs1)):
        for k in range(3):
            vk = v[k] if k < 2 else v[2][:short]
            assert (got4[c, k] == ctx.inner_product(crs, vk, threads=0, window=8)[0]).all(), (c, k)
    with _lib.tuning(mac_share_keys=0):
        dev.set_profiling(True)
        ref4, _ = dev.msm([dev.put(crs0), dev.put(crs1)], g2, 3, crs_len=T, window=8)
        names = {k["name"] for k in dev.profile_read()}
        dev.set_profiling(False)
    assert not any(k.startswith("mac_kernel_v4") for k in names) and (host(ref4) == got4).all()
    with _lib.tuning(mac_variant=1):
        ref, _ = dev.msm([dev.put(crs0)], groups, ng, crs_len=T, window=8)
    assert (host(ref) == got).all()
    if name == "C5":  # a two-vector group on the 54-bit prime: refused by the hybrid path, served by the integer kernel
        dev.set_profiling(True)
        out3, _ = dev.msm([dev.put(crs0)], [(dv[1], None, 0), (dv[2], None, 0)], 1, crs_len=T, window=8)
        names = {k["name"] for k in dev.profile_read()}
        dev.set_profiling(False)
        assert "mac_kernel" in names and "mac_kernel_v3<false, 14>" not in names, names
        assert (host(out3)[0, 0] == ctx.enc_add(e[1], e[2])).all()


@pytest.mark.parametrize("name", ["toy", "C2", "C3"])
def test_grouped_msm_with_vectors_of_different_lengths(name):
    """rs_msm lets every vector have its own length.  Three single-vector groups of lengths {4, T, T} and a constant-1
    term in the middle: in the wide plaintext kernel (N_enc = 8192) a workgroup then meets items with nothing to load
    between items it must load, which once left the next item computed from stale registers."""
    dev = dev_for(name)
    ctx = H.oracle_ctx(dev.prm)
    T = 300  # > 2 x 128 slots per limb / 3 groups, so a slot of the persistent kernel sees skip -> load sequences
    crs = ctx.random_enc(141, 16)  # tiled key: term t reads element t % 16
    lens = [4, T, T - 7]
    vs = [ctx.random_ring(143 + k, n) for k, n in enumerate(lens)]
    kinds = [None, np.zeros(T, dtype=np.uint8), None]
    kinds[1][5] = O.KIND_ONE
    kinds[1][T - 1] = O.KIND_ONE
    out, used = dev.msm([dev.put(crs)], [(dev.put(v), k, g) for g, (v, k) in enumerate(zip(vs, kinds))], 3, want_used=True,
                        crs_len=T, window=16)
    got = host(out)
    assert used == lens
    for g, (v, k) in enumerate(zip(vs, kinds)):
        exp, _ = ctx.inner_product(crs, v, k, threads=0, window=16)
        assert (got[0, g] == exp).all(), g
    if dev.prm.N_enc == 8192:
        # the same groups against TWO key vectors (Rinocchio, rinocchio.tcc:106-160): one plaintext spectrum per term for both
        # (mac_kernel_v4<13, *>: half spectrum per workgroup); against the oracle and the per-key kernels
        crs1 = ctx.random_enc(142, 16)
        groups = [(dev.put(v), k, g) for g, (v, k) in enumerate(zip(vs, kinds))]
        dev.set_profiling(True)
        out2, used2 = dev.msm([dev.put(crs), dev.put(crs1)], groups, 3, want_used=True, crs_len=T, window=16)
        names = {k["name"] for k in dev.profile_read()}
        dev.set_profiling(False)
        assert any(k.startswith("mac_kernel_v4<13") for k in names), names
        got2 = host(out2)
        assert used2 == lens and (got2[0] == got[0]).all()
        for g, (v, k) in enumerate(zip(vs, kinds)):
            assert (got2[1, g] == ctx.inner_product(crs1, v, k, threads=0, window=16)[0]).all(), g
        with _lib.tuning(mac_share_keys=0):
            ref2, _ = dev.msm([dev.put(crs), dev.put(crs1)], groups, 3, crs_len=T, window=16)
        assert (host(ref2) == got2).all()


@pytest.mark.parametrize("name", ["C2", "C3"])
def test_wide_kernels_equal_their_predecessors_and_the_oracle(name):
    """N_enc = 8192: the wide NTT (ntt_variant 14), the half-spectrum MAC (mac_variant 5) and the wide plaintext kernel
    with paired rows (plain_variant 1) against their fallbacks -- the barrier and wave-private NTT kernels (ntt_variant 0
    and 12), mac_kernel_v2<512> (mac_variant 3; 6 is a synonym of 5) and plain_center_kernel -- on a grouped inner product
    with a zero term, a one-limb-zero term, a Scalar-1 term and a short vector; one configuration also against the oracle.
    C2 has N = 4096 < N_enc (slots beyond N stay zero), C3 N = N_enc."""
    import torch
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    # transforms, both moduli sets, odd batch
    for modset, idx, q in ((_lib.RS_MOD_COEFF, prm.K - 1, prm.Q[-1]), (_lib.RS_MOD_PLAIN, 0, prm.q[0])):
        src = torch.empty((37, prm.N_enc), dtype=torch.int64, device=dev.device).random_(0, int(q))
        outs = []
        for v in (0, 12, 14):  # barrier kernel, wave-private kernel, wide kernels
            with _lib.tuning(ntt_variant=v):
                d = src.clone()
                dev.ntt(d, modset, idx)
                f = d.clone()
                dev.ntt(d, modset, idx, inverse=True)
                assert (d == src).all(), ("roundtrip", v)
                outs.append(f)
        assert (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all()
    # grouped inner product: group 0 = {v0, v1} (multi-vector: summed after the lift), group 1 = {v2 (shorter)}
    T = 9
    encs = ctx.random_enc(51, T)
    v = [ctx.random_ring(52 + k, T) for k in range(2)] + [ctx.random_ring(55, T - 3)]
    v[0][2] = 0
    v[1][3, 0] = 0
    kinds = np.zeros(T, dtype=np.uint8)
    kinds[4] = O.KIND_ONE
    vecs = [(dev.put(v[0]), kinds, 0), (dev.put(v[1]), None, 0), (dev.put(v[2]), None, 1)]
    res = {}
    for mv, pv in ((5, 1), (3, 0), (5, 0), (3, 1), (6, 1), (6, 0)):  # 3: mac_kernel_v2<512>; 5 and 6: mac_kernel_v3
        with _lib.tuning(mac_variant=mv, plain_variant=pv):
            out, used = dev.msm([dev.put(encs)], vecs, 2, want_used=True)
            res[(mv, pv)] = (host(out), used)
    ref = res[(3, 0)]
    for k, r in res.items():
        assert r[1] == ref[1], k
        assert (r[0] == ref[0]).all(), k
    e0 = ctx.enc_add(ctx.inner_product(encs, v[0], kinds)[0], ctx.inner_product(encs, v[1])[0])
    e1 = ctx.inner_product(encs[: T - 3], v[2])[0]
    assert (ref[0][0, 0] == e0).all() and (ref[0][0, 1] == e1).all()


@pytest.mark.parametrize("name,m,kind", [("toy", 1, "chain"), ("toy", 2, "chain"), ("toy", 3, "wide"), ("toy", 7, "wide"),
                                          ("toy", 16, "wide"), ("toy", 100, "wide"), ("toy", 100, "many_inputs"),
                                          ("toy", 600, "wide"),  # M = 1024: split Newton / in-place product-tree kernels
                                          ("toy49", 33, "wide"), ("toy49", 64, "chain"), ("toy49", 90, "many_inputs"),
                                          ("toy50", 33, "wide"), ("toy50", 64, "chain"), ("toy50", 90, "many_inputs"),  # primes just below 2^50
                                          # primes >= 2^50: the integer (Montgomery) arithmetic, generic kernels
                                          ("toy54", 1, "chain"), ("toy54", 7, "wide"), ("toy54", 100, "wide"), ("toy54", 100, "many_inputs"),
                                          ("toy60", 16, "wide"), ("toy60", 64, "chain"), ("toy60", 600, "wide"), ("toy60", 90, "many_inputs"),
                                          ("toy+int", 33, "wide"), ("toy49+int", 64, "chain")])
def test_witness_map_matches_oracle(name, m, kind):
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    if kind == "many_inputs":  # > 64 primary inputs: the generic io path (evaluate + interpolate)
        cs = R.wide_r1cs(m, prm.q, n_inputs=70)
    else:
        cs = R.wide_r1cs(m, prm.q) if kind == "wide" else R.chain_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    dcs = dev.r1cs(cs)
    dasg = dev.put(asg)
    ocs = H.oracle_cs(cs)
    # a14
    for which in range(3):
        got = host(dev.r1cs_evaluate(dcs, which, _lib.RS_EVAL_FULL, dasg))
        for limb in range(prm.L):
            exp = O.r1cs_evaluate(prm.q[limb], ocs, which, limb, np.ascontiguousarray(asg[:, limb, :]))
            assert (got[:, limb, :] == exp).all()
    for zk in (False, True):
        ds = [ctx.random_ring(60 + k) for k in range(3)] if zk else [None] * 3
        dds = [dev.put(d) if d is not None else None for d in ds]
        w = dev.witness_map(dcs, dasg, *dds)
        for limb in range(prm.L):
            a = np.ascontiguousarray(asg[:, limb, :])
            dl = [np.ascontiguousarray(d[limb]) if d is not None else None for d in ds]
            exp = O.witness_map(prm.q[limb], ocs, limb, a, *dl)
            for k in ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H"):
                assert (host(w[k])[:, limb, :] == exp[k]).all(), (k, limb, zk)
            assert (w["Z"][limb] == exp["Z"]).all()


@pytest.mark.parametrize("name,m,aux_only,zk,lds", [("toy", 9, False, True, 13), ("toy", 12, True, True, 13), ("toy60", 9, False, False, 13),
                                                     ("toy+int", 12, True, True, 13), ("toy49", 150, False, True, 6), ("toy50", 150, False, True, 6), ("toy", 150, True, False, 6),
                                                     ("toy54", 70, False, True, 6)])
def test_polynomial_coefficients_match_oracle(name, m, aux_only, zk, lds):
    """Row a14 with coefficients that are general ring elements (rs_r1cs_create_poly; relations/variable.tcc:246-254,
    benchmarks/bench_ntt_SEAL.cpp:46-53): evaluate in its three modes, the whole witness map and both provers against
    the oracle.  aux_only keeps the linear-form io vectors (no polynomial on the constant one or an input); otherwise
    the generic io path and the per-slot constant part of the mid vectors run.  lds = 6 forces the multi-pass columns."""
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = R.wide_poly_r1cs(m, prm.q, prm.N, aux_only=aux_only)
    assert cs.poly_table is not None and (cs.poly_idx["a"] >= 0).sum() >= m // 2
    asg = H.make_assignment(ctx, cs)
    ocs = H.oracle_cs(cs)
    dcs, dasg = dev.r1cs(cs), dev.put(asg)
    for which in range(3):
        for mode, zero in ((_lib.RS_EVAL_FULL, None), (_lib.RS_EVAL_IO, slice(cs.n_inputs, None)), (_lib.RS_EVAL_MID, slice(0, cs.n_inputs))):
            part = asg.copy()
            if zero is not None:
                part[zero] = 0
            got = host(dev.r1cs_evaluate(dcs, which, mode, dasg))
            for limb in range(prm.L):
                assert (got[:, limb, :] == O.r1cs_evaluate(prm.q[limb], ocs, which, limb, np.ascontiguousarray(part[:, limb, :]))).all(), (which, mode)
    ds = [ctx.random_ring(60 + k) for k in range(3)] if zk else [None] * 3
    dds = [dev.put(d) if d is not None else None for d in ds]
    with _lib.tuning(witness_lds_logM=lds):
        w = dev.witness_map(dcs, dasg, *dds)
        got = {k: host(v) if k != "Z" else v for k, v in w.items()}
        pk = dict(s_pows=ctx.random_enc(71, m + 1), delta_ts=ctx.random_enc(72, m + 1), delta_mid=ctx.random_enc(73, cs.n_aux),
                  alpha=ctx.random_enc(74), beta=ctx.random_enc(75))
        gp, gempty = dev.groth16_prove(dcs, {k: dev.put(v) for k, v in pk.items()}, dasg)
        gp = host(gp)
        rk = dict(s_pows=ctx.random_enc(81, m + 1), alpha_s_pows=ctx.random_enc(82, m + 1), beta_prods=ctx.random_enc(83, cs.n_aux),
                  beta_rv_ts=ctx.random_enc(84), beta_rw_ts=ctx.random_enc(85), beta_ry_ts=ctx.random_enc(86))
        rp, rempty = dev.rinocchio_prove(dcs, {k: dev.put(v) for k, v in rk.items()}, dasg, *dds)
        rp = host(rp)
    for limb in range(prm.L):
        dl = [np.ascontiguousarray(d[limb]) if d is not None else None for d in ds]
        exp = O.witness_map(prm.q[limb], ocs, limb, np.ascontiguousarray(asg[:, limb, :]), *dl)
        for k in ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H"):
            assert (got[k][:, limb, :] == exp[k]).all(), (k, limb)
    if m <= 20:  # the oracle provers are O(m^2) per slot plus the inner products
        exp, exp_empty = O.groth16_prove(ctx, ocs, pk, asg)
        assert gempty == exp_empty and (gp == exp).all()
        exp, exp_empty = O.rinocchio_prove(ctx, ocs, rk, asg, *ds)
        assert rempty == exp_empty and (rp == exp).all()


@pytest.mark.parametrize("name,m", [("toy", 40), ("toyR", 300), ("toy60", 33)])
def test_polynomial_coefficients_on_slot_ranges_chunks_and_recipe_primes(name, m):
    """Polynomial R1CS coefficients through the other ways the witness map is driven: a slot range of every limb with
    compact outputs (rs_witness_map_slots: the coefficient table is indexed by the ABSOLUTE slot), column chunks smaller
    than a limb, and ring primes that need the block-convolution path (toyR at m = 300)."""
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = R.wide_poly_r1cs(m, prm.q, prm.N)
    asg = H.make_assignment(ctx, cs)
    ds = [ctx.random_ring(60 + k) for k in range(3)]
    dcs, dasg, dds = dev.r1cs(cs), dev.put(asg), [dev.put(d) for d in ds]
    ocs = H.oracle_cs(cs)
    keys = ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H")
    exp = [O.witness_map(prm.q[limb], ocs, limb, np.ascontiguousarray(asg[:, limb, :]), *[np.ascontiguousarray(d[limb]) for d in ds])
           for limb in range(prm.L)]
    s0, ns = 6, 10
    w = dev.witness_map_slots(dcs, dasg, s0, ns, *dds)
    for limb in range(prm.L):
        for k in keys:
            assert (host(w[k])[:, limb, :] == exp[limb][k][:, s0:s0 + ns]).all(), (k, limb)
    with _lib.tuning(witness_col_budget_mib=1):  # chunks of at most 64 columns
        w = dev.witness_map(dcs, dasg, *dds)
    for limb in range(prm.L):
        for k in keys:
            assert (host(w[k])[:, limb, :] == exp[limb][k]).all(), (k, limb)


def test_bench_ntt_seal_circuit_proven_bit_exact():
    """BASELINE.json configs[0] is the reference's benchmarks/bench_ntt_SEAL.cpp: Rinocchio Setup / Prove / Verify of ONE
    constraint over N + 1 = 4097 variables, all public, whose coefficients are the powers of a POLYNOMIAL ring element
    (:28-55), on N = 4096 with BFVDefault(4096) = preset C2's ring.  rs_rinocchio_prove on it, bit for bit against the
    oracle (the non-ZK branch: no auxiliary inputs, rinocchio.tcc:81-87), and the witness map against the oracle."""
    dev = dev_for("C2")
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs, asg = H.dft_circuit(prm, ctx)
    assert (cs.m, cs.n_vars, cs.n_inputs, cs.n_aux) == (1, 4097, 4097, 0) and cs.poly_table.shape == (4095, prm.L, prm.N)
    ocs = H.oracle_cs(cs)
    dcs, dasg = dev.r1cs(cs), dev.put(asg)
    # the assignment satisfies the constraint: <a, x> * 1 = x_{N+1}
    ev = [host(dev.r1cs_evaluate(dcs, k, 0, dasg)) for k in range(3)]
    assert (ctx.ring_mul(ev[0][0], ev[1][0]) == ev[2][0]).all() and (ev[2][0] == asg[-1]).all() and ev[0][0].any()
    w = dev.witness_map(dcs, dasg)
    for limb in range(prm.L):
        exp = O.witness_map(prm.q[limb], ocs, limb, np.ascontiguousarray(asg[:, limb, :]))
        for k in ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H"):
            assert (host(w[k])[:, limb, :] == exp[k]).all(), (k, limb)
    m = 1
    pk = dict(s_pows=ctx.random_enc(81, m + 1), alpha_s_pows=ctx.random_enc(82, m + 1), beta_prods=None,
              beta_rv_ts=ctx.random_enc(84), beta_rw_ts=ctx.random_enc(85), beta_ry_ts=ctx.random_enc(86))
    got, empty = dev.rinocchio_prove(dcs, {k: (dev.put(v) if v is not None else None) for k, v in pk.items()}, dasg)
    opk = dict(pk, beta_prods=np.zeros((0,) + ctx.enc_shape(), dtype=np.uint64))
    exp, exp_empty = O.rinocchio_prove(ctx, ocs, opk, asg)
    assert empty == exp_empty == [1, 1, 0, 0, 1, 1, 1, 1, 1]  # only <s_pows, b_mid> = the constant 1 has a non-zero term
    assert (host(got) == exp).all()


def test_interpolate_known_answer_on_device():
    # util/interpolation_test.cpp:29-55 through the device path
    dev = dev_for("toy")
    prm = dev.prm
    n = 8
    y = np.zeros((n, prm.L, prm.N), dtype=np.uint64)
    for limb, q in enumerate(prm.q):
        coeffs = np.arange(n, dtype=np.uint64).reshape(n, 1)
        for x in range(n):
            y[x, limb, :] = O.poly_eval(q, coeffs, x)[0]
    got = host(dev.interpolate(dev.put(y)))
    for k in range(n):
        assert (got[k] == k).all()


@pytest.mark.parametrize("name,m,kind", [("toy", 6, "wide"), ("toy", 16, "chain"), ("toy49", 21, "wide"), ("toy50", 21, "wide"), ("toy54", 12, "wide"),
                                          ("toy60", 21, "wide"), ("toy+int", 16, "chain")])
def test_groth16_prover_matches_oracle(name, m, kind):
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = R.wide_r1cs(m, prm.q) if kind == "wide" else R.chain_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk = dict(s_pows=ctx.random_enc(71, m + 1), delta_ts=ctx.random_enc(72, m + 1), delta_mid=ctx.random_enc(73, cs.n_aux),
              alpha=ctx.random_enc(74), beta=ctx.random_enc(75))
    exp, exp_empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
    got, empty = dev.groth16_prove(dev.r1cs(cs), {k: dev.put(v) for k, v in pk.items()}, dev.put(asg))
    assert empty == exp_empty
    assert (host(got) == exp).all()


@pytest.mark.parametrize("name,m,zk", [("toy", 5, False), ("toy", 12, True), ("toy49", 16, True), ("toy50", 16, True), ("toy54", 9, True), ("toy60", 12, True),
                                       ("toy60", 5, False)])
def test_rinocchio_prover_matches_oracle(name, m, zk):
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = R.wide_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk = dict(s_pows=ctx.random_enc(81, m + 1), alpha_s_pows=ctx.random_enc(82, m + 1), beta_prods=ctx.random_enc(83, cs.n_aux),
              beta_rv_ts=ctx.random_enc(84), beta_rw_ts=ctx.random_enc(85), beta_ry_ts=ctx.random_enc(86))
    ds = [ctx.random_ring(90 + k) for k in range(3)] if zk else [None] * 3
    exp, exp_empty = O.rinocchio_prove(ctx, H.oracle_cs(cs), pk, asg, *ds)
    got, empty = dev.rinocchio_prove(dev.r1cs(cs), {k: dev.put(v) for k, v in pk.items()}, dev.put(asg),
                                     *[dev.put(d) if d is not None else None for d in ds])
    assert empty == exp_empty
    g = host(got)
    for k in range(9):
        assert (g[k] == exp[k]).all(), k


@pytest.mark.parametrize("name,m,kind,zk", [("toy", 70, "wide", False), ("toy", 300, "wide", True), ("toy", 1000, "chain", True),
                                             ("toy", 513, "many_inputs", False), ("toy60", 300, "wide", True), ("toy54", 513, "many_inputs", False)])
def test_witness_map_multipass_matches_oracle(name, m, kind, zk):
    """The multi-pass (column does not fit one LDS tile) path, forced at small sizes by shrinking the
    tile to 2^6 so the complete oracle comparison stays cheap (both arithmetics)."""
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = {"wide": lambda: R.wide_r1cs(m, prm.q), "chain": lambda: R.chain_r1cs(m, prm.q),
          "many_inputs": lambda: R.wide_r1cs(m, prm.q, n_inputs=70)}[kind]()
    asg = H.make_assignment(ctx, cs)
    ds = [ctx.random_ring(60 + k) for k in range(3)] if zk else [None] * 3
    with _lib.tuning(witness_lds_logM=6):
        w = dev.witness_map(dev.r1cs(cs), dev.put(asg), *[dev.put(d) if d is not None else None for d in ds])
        got = {k: host(v) if k != "Z" else v for k, v in w.items()}
    ocs = H.oracle_cs(cs)
    for limb in range(prm.L):
        dl = [np.ascontiguousarray(d[limb]) if d is not None else None for d in ds]
        exp = O.witness_map(prm.q[limb], ocs, limb, np.ascontiguousarray(asg[:, limb, :]), *dl)
        for k in ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H"):
            assert (got[k][:, limb, :] == exp[k]).all(), (k, limb)
        assert (got["Z"][limb] == exp["Z"]).all()


def test_groth16_prover_multipass_matches_oracle():
    dev = dev_for("toy")
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    m = 200
    cs = R.wide_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk = dict(s_pows=ctx.random_enc(71, m + 1), delta_ts=ctx.random_enc(72, m + 1), delta_mid=ctx.random_enc(73, cs.n_aux),
              alpha=ctx.random_enc(74), beta=ctx.random_enc(75))
    exp, exp_empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
    with _lib.tuning(witness_lds_logM=7):
        got, empty = dev.groth16_prove(dev.r1cs(cs), {k: dev.put(v) for k, v in pk.items()}, dev.put(asg))
        g = host(got)
    assert empty == exp_empty and (g == exp).all()


def _horner(coeffs, x, q):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + int(c)) % q
    return acc


@pytest.mark.parametrize("m", [1500, 3000, 8192, 10000, 20000])
def test_witness_map_full_size_columns(m):
    """Headline-size primes at column lengths the oracle cannot follow on every slot: M = 2048, 4096,
    8192, 16384 (single-tile kernels at 128 / 256 / 512 / 1024 threads; 512 is the level-unrolled
    shape of the benchmark, 1024 the one-workgroup-per-CU 2^14 tile) and m = 20000 (M = 2^15: the
    natural multi-pass path on 2^13 tiles).  Checked
    against the oracle's O(n^2) interpolation on one slot, and on other slots through
    size-independent properties: P(j) = y_j on the domain and H*Z = A*B - C at random points."""
    dev = dev_for("toy44")
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    rng = np.random.RandomState(5)
    y = ctx.random_ring(91, m)
    got = host(dev.interpolate(dev.put(y)))
    exp0 = O.interpolate(prm.q[0], np.ascontiguousarray(y[:, 0, :1]))
    assert (got[:, 0, 0] == exp0[:, 0]).all()
    for limb, slot in ((0, 7), (1, 0), (1, 31)):
        q = prm.q[limb]
        for j in [0, 1, m - 1] + [int(v) for v in rng.randint(0, m, 3)]:
            assert _horner(got[:, limb, slot], j, q) == int(y[j, limb, slot])
    # full witness map on the chain circuit
    cs = R.chain_r1cs(m, prm.q)
    asg = dev.ring_empty(m + 2)
    asg[:2] = dev.put(ctx.random_ring(92, 2))
    dev.chain_assignment(asg, m)
    w = dev.witness_map(dev.r1cs(cs), asg)
    A = (host(w["A_io"]).astype(object) + host(w["A_mid"]).astype(object))
    B = (host(w["B_io"]).astype(object) + host(w["B_mid"]).astype(object))
    C = (host(w["C_io"]).astype(object) + host(w["C_mid"]).astype(object))
    Hh = host(w["H"])
    a = host(asg)
    for limb, slot in ((0, 3), (1, 17)):
        q = prm.q[limb]
        Z = w["Z"][limb]
        for j in (0, 5, m - 1):  # A interpolates x_j, B x_{j+1}, C x_{j+2}
            assert _horner(A[:, limb, slot] % q, j, q) == int(a[j, limb, slot])
            assert _horner(B[:, limb, slot] % q, j, q) == int(a[j + 1, limb, slot])
            assert _horner(C[:, limb, slot] % q, j, q) == int(a[j + 2, limb, slot])
        for x in [int(v) for v in rng.randint(m, 2**40, 3)]:
            lhs = _horner(Hh[:, limb, slot], x, q) * _horner(Z, x, q) % q
            rhs = (_horner(A[:, limb, slot] % q, x, q) * _horner(B[:, limb, slot] % q, x, q) - _horner(C[:, limb, slot] % q, x, q)) % q
            assert lhs == rhs


@pytest.mark.parametrize("m", [1500, 3000, 8192, 9000, 17000])
def test_witness_map_is_deterministic(m):
    """Race detector for the LDS kernels: repeated runs on the same inputs must agree bit for bit
    (a missing barrier shows up as run-to-run differences long before it fails a single comparison)."""
    dev = dev_for("toy44")
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    asg = dev.ring_empty(m + 2)
    asg[:2] = dev.put(ctx.random_ring(93, 2))
    dev.chain_assignment(asg, m)
    dcs = dev.r1cs(cs)
    ds = [dev.put(ctx.random_ring(94 + k)) for k in range(3)]
    first = None
    for _ in range(8):
        w = dev.witness_map(dcs, asg, *ds)
        cur = {k: host(w[k]).copy() for k in ("A_io", "A_mid", "B_mid", "C_mid", "H")}
        if first is None:
            first = cur
        else:
            for k in cur:
                assert (cur[k] == first[k]).all(), k


def test_c4_shape_rinocchio_configuration():
    """BASELINE.json configs[3] shape (C4: ring N = 16384 with six 48/49-bit primes, encodings
    N_enc = 16384 with K = 8): transforms, the inner product (with its special terms) and a small
    Rinocchio proof, bit-exact against the oracle.  N_enc = 16384 takes the generic MAC kernel and
    the 136 KiB-tile transforms."""
    dev = dev_for("C4")
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    rng = np.random.RandomState(2)
    logn = prm.N_enc.bit_length() - 1
    for modset, primes in ((_lib.RS_MOD_PLAIN, prm.q[-1:]), (_lib.RS_MOD_COEFF, prm.Q[-1:])):
        idx = (prm.L if modset == _lib.RS_MOD_PLAIN else prm.K) - 1
        p = primes[0]
        a = (rng.randint(0, 2**62, size=(2, prm.N_enc), dtype=np.int64).astype(np.uint64)) % np.uint64(p)
        d = dev.put(a)
        dev.ntt(d, modset, idx)
        t = O.NTT(logn, p)
        assert (host(d)[1] == t.fwd(a[1])).all()
        dev.ntt(d, modset, idx, inverse=True)
        assert (host(d) == a).all()
    T = 5
    encs, rings = ctx.random_enc(31, T), ctx.random_ring(32, T)
    kinds = np.zeros(T, dtype=np.uint8)
    rings[2] = 0
    kinds[4] = O.KIND_ONE
    exp, used = ctx.inner_product(encs, rings, kinds)
    got, gused = dev.inner_product(dev.put(encs), dev.put(rings), kinds)
    assert gused == used and (host(got) == exp).all()
    m = 3
    cs = R.wide_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk = dict(s_pows=ctx.random_enc(81, m + 1), alpha_s_pows=ctx.random_enc(82, m + 1), beta_prods=ctx.random_enc(83, cs.n_aux),
              beta_rv_ts=ctx.random_enc(84), beta_rw_ts=ctx.random_enc(85), beta_ry_ts=ctx.random_enc(86))
    ds = [ctx.random_ring(90 + k) for k in range(3)]
    exp, exp_empty = O.rinocchio_prove(ctx, H.oracle_cs(cs), pk, asg, *ds)
    got, empty = dev.rinocchio_prove(dev.r1cs(cs), {k: dev.put(v) for k, v in pk.items()}, dev.put(asg), *[dev.put(d) for d in ds])
    assert empty == exp_empty
    g = host(got)
    for k in range(9):
        assert (g[k] == exp[k]).all(), k


def test_entry_points_are_reentrant_on_a_shared_context():
    """SURVEY 8(b) threading: the reference calls inner_product from up to ten OpenMP sections
    (rinocchio.tcc:106-163).  Four host threads hammer one context (ctypes drops the GIL inside
    the library); every result must equal the sequential one."""
    import threading
    dev = dev_for("toy")
    ctx = H.oracle_ctx(dev.prm)
    T = 9
    jobs = []
    for k in range(4):
        encs, rings = ctx.random_enc(200 + k, T), ctx.random_ring(300 + k, T)
        a, b = ctx.random_ring(400 + k, 3), ctx.random_ring(500 + k, 3)
        jobs.append((dev.put(encs), dev.put(rings), dev.put(a), dev.put(b), ctx.inner_product(encs, rings)[0], ctx.ring_mul(a, b)))
    errors = []

    def work(j):
        try:
            de, dr, da, db, exp_ip, exp_mul = jobs[j]
            for _ in range(20):
                got, _ = dev.inner_product(de, dr)
                if not (host(got) == exp_ip).all():
                    errors.append(("inner_product", j))
                if not (host(dev.ring_mul(da, db)) == exp_mul).all():
                    errors.append(("ring_mul", j))
        except Exception as e:  # noqa: BLE001
            errors.append((repr(e), j))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]


def test_entry_points_on_distinct_streams_without_synchronising():
    """calls that do NOT synchronise (want_used=False) issued from different streams share
    the context's workspace; the per-buffer event must order them.  Every thread drives its own
    torch stream and only synchronises at the very end."""
    import threading

    import torch
    dev = dev_for("toy")
    ctx = H.oracle_ctx(dev.prm)
    T = 33
    jobs = []
    for k in range(4):
        encs, rings = ctx.random_enc(700 + k, T), ctx.random_ring(800 + k, T)
        jobs.append((dev.put(encs), dev.put(rings), ctx.inner_product(encs, rings)[0]))
    torch.cuda.synchronize()
    errors, results = [], [[] for _ in jobs]

    def work(j):
        try:
            st = torch.cuda.Stream(device=dev.device)
            with torch.cuda.stream(st):
                for _ in range(25):
                    results[j].append(dev.inner_product(jobs[j][0], jobs[j][1], want_used=False)[0])
            st.synchronize()
        except Exception as e:  # noqa: BLE001
            errors.append((repr(e), j))

    threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
    for j, outs in enumerate(results):
        for r in outs:
            assert (host(r) == jobs[j][2]).all(), j


@pytest.mark.parametrize("name,m,kind,zk", [("toy", 40, "wide", True), ("toy", 64, "chain", False), ("toy", 100, "many_inputs", True),
                                            ("toy44", 1500, "chain", True)])
def test_witness_map_slot_ranges_and_chunks_equal_the_whole(name, m, kind, zk):
    """the witness map is slot-parallel.  (a) rs_witness_map_slots on two halves of
    the slots returns exactly the corresponding slices of the full map (compact layout, m == M case
    included); (b) a tiny column budget (many chunks, pieces of one limb) changes nothing."""
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = {"wide": lambda: R.wide_r1cs(m, prm.q), "chain": lambda: R.chain_r1cs(m, prm.q),
          "many_inputs": lambda: R.wide_r1cs(m, prm.q, n_inputs=70)}[kind]()
    if name == "toy":
        asg = dev.put(H.make_assignment(ctx, cs))
    else:  # chain assignment on the device (the oracle's O(m^2) map is not needed here)
        asg = dev.ring_empty(m + 2)
        dev.fill_uniform(asg[:2], 0, 5)
        dev.chain_assignment(asg, m)
    ds = [dev.put(ctx.random_ring(60 + k)) for k in range(3)] if zk else [None] * 3
    dcs = dev.r1cs(cs)
    keys = ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H")
    full = {k: host(v) for k, v in dev.witness_map(dcs, asg, *ds).items() if k in keys}
    half = prm.N // 2
    for slot0, ns in ((0, half), (half, half), (prm.N // 4, 6)):
        part = dev.witness_map_slots(dcs, asg, slot0, ns, *ds)
        for k in keys:
            assert (host(part[k]) == full[k][:, :, slot0:slot0 + ns]).all(), (k, slot0, ns)
    with _lib.tuning(witness_col_budget_mib=1):
        again = dev.witness_map(dcs, asg, *ds)
        for k in keys:
            assert (host(again[k]) == full[k]).all(), k
        # a subset of outputs (the ringGroth16 set) through the chunked path
        sub = dev.witness_map(dcs, asg, *ds, want=("A_io", "A_mid", "B_io", "B_mid", "H"))
        for k in ("A_io", "A_mid", "B_io", "B_mid", "H"):
            assert (host(sub[k]) == full[k]).all(), k


@pytest.mark.parametrize("name,m,kind,zk", [("toy", 40, "wide", True), ("toy", 64, "chain", False), ("toy", 100, "many_inputs", True),
                                            ("toy60", 33, "wide", True), ("toy44", 1500, "chain", True), ("toy44", 20000, "chain", False)])
def test_witness_map_row_ranges_equal_slices_of_the_whole(name, m, kind, zk):
    """rs_witness_map_rows: a rank that shares its limbs with others runs the whole map and keeps the rows of its TERM
    range (ringsnark_amd/dist.py "replicate"; full-length vectors of a configs[3] rank would not fit HBM).  Every output
    equals the corresponding row slice of the full map: the ranges of the sharded provers (m rows for the A / B vectors,
    m + 1 for H, 2..4 shards), ranges that start and stop inside a 32-row tile, empty ranges, the lone top row of H
    (row m when m is a power of two comes from its own kernel), and a subset of outputs."""
    from ringsnark_amd import dist as RD
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = {"wide": lambda: R.wide_r1cs(m, prm.q), "chain": lambda: R.chain_r1cs(m, prm.q),
          "many_inputs": lambda: R.wide_r1cs(m, prm.q, n_inputs=70)}[kind]()
    if m <= 100:
        asg = dev.put(H.make_assignment(ctx, cs))
    else:
        asg = dev.ring_empty(m + 2)
        dev.fill_uniform(asg[:2], 0, 5)
        dev.chain_assignment(asg, m)
    ds = [dev.put(ctx.random_ring(60 + k)) for k in range(3)] if zk else [None] * 3
    dcs = dev.r1cs(cs)
    keys = ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H")
    full = {k: host(v) for k, v in dev.witness_map(dcs, asg, *ds).items() if k in keys}
    cases = []
    for shards in (2, 3, 4):
        for s in range(shards):
            plan = RD.ShardPlan(shards, s, 1, 1, shards, [0], s, 0)
            ab, h = plan.term_range(m), plan.term_range(m + 1)
            cases.append({"A_io": ab, "A_mid": ab, "B_io": ab, "B_mid": ab, "C_io": ab, "C_mid": ab, "H": h})
    cases.append({k: (5, min(37, m)) for k in keys})
    cases.append({"A_io": (0, 0), "A_mid": (0, 0), "B_io": (m - 1, m), "B_mid": (m - 1, m), "H": (m, m + 1)})  # C vectors: every row
    cases.append({"H": (m - 3, m + 1), "A_mid": (31, 33)})
    for rows in cases:
        part = dev.witness_map(dcs, asg, *ds, rows=rows)
        for k in keys:
            lo, hi = rows.get(k, (0, full[k].shape[0]))
            if k.endswith("_io") and k not in rows and k.replace("_io", "_mid") in rows:
                lo, hi = rows[k.replace("_io", "_mid")]  # io and mid of one matrix share a range
            assert part[k].shape[0] == hi - lo and (host(part[k]) == full[k][lo:hi]).all(), (k, rows)
    sub = dev.witness_map(dcs, asg, *ds, want=("A_mid", "H"), rows={"A_mid": (3, 9), "H": (1, m + 1)})
    assert (host(sub["A_mid"]) == full["A_mid"][3:9]).all() and (host(sub["H"]) == full["H"][1:]).all() and sub["B_mid"] is None


@pytest.mark.parametrize("name,T", [("toy", 9), ("toy49", 20), ("toy50", 20), ("toy60", 9), ("C2", 6), ("C5s", 4), ("C4", 3), ("C5", 5)])
def test_slot_constant_vectors_equal_their_expanded_rows(name, T):
    """rs_msm_vec::slot_const: a vector whose ring elements hold one value per limb in every slot (coefficients_for_Z,
    util/evaluation_domain.tcc:54-60) handed over as the compact [T][L] array of values -- the plaintext is value x
    encode(1, ..., 1), no transform -- gives the inner products of the expanded [T][L][N] vector: against the oracle (toy
    presets), on both arithmetics, the hybrid context (C5), the 16384-point shapes, and the wide 8192-point plaintext kernel
    (C2), which expands the rows inside the library.  A zero value is skipped like a zero polynomial (used-term counts), a
    Scalar-1 term (the leading coefficient of Z) still passes its key element through, and the vector may share a group
    with an ordinary one."""
    import torch
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    rng = np.random.RandomState(T)
    vals = np.stack([rng.randint(0, 2**62, size=T, dtype=np.int64).astype(np.uint64) % np.uint64(q) for q in prm.q], axis=1)  # [T][L]
    vals[1] = 0
    vals[T - 1] = 1
    kinds = np.zeros(T, dtype=np.uint8)
    kinds[T - 1] = O.KIND_ONE
    rows = np.ascontiguousarray(np.repeat(vals[:, :, None], prm.N, axis=2))
    other = ctx.random_ring(5, T)
    keys = [ctx.random_enc(31, T), ctx.random_enc(32, T)]
    dkeys = [dev.put(k) for k in keys]
    compact, used_c = dev.msm(dkeys, [(dev.put(vals), kinds, 0, True), (dev.put(other), None, 1), (dev.put(vals), None, 1, True)], 2, want_used=True)
    expanded, used_e = dev.msm(dkeys, [(dev.put(rows), kinds, 0), (dev.put(other), None, 1), (dev.put(rows), None, 1)], 2, want_used=True)
    assert used_c == used_e and used_c[0] == T - 1 and used_c[2] == T - 1
    assert torch.equal(compact, expanded)
    if prm.N_enc <= 128:
        for c in range(2):
            exp, _ = ctx.inner_product(keys[c], rows, kinds)
            assert (host(compact)[c, 0] == exp).all()


def test_witness_map_row_ranges_are_validated():
    """rs_witness_map_rows refuses ranges outside a vector and different ranges for the io and mid vectors of one matrix
    (one pass writes both)."""
    import ctypes as C
    from ringsnark_amd.device import _ptr
    dev = dev_for("toy")
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    m = 12
    cs = R.wide_r1cs(m, prm.q)
    asg = dev.put(H.make_assignment(ctx, cs))
    dcs = dev.r1cs(cs)
    outs = [dev.ring_empty(m + 1) for _ in range(7)]
    Z = np.zeros((prm.L, m + 1), dtype=np.uint64)

    def call(rows):
        flat = (C.c_size_t * 14)(*[x for r in rows for x in r])
        return dev.lib.rs_witness_map_rows(dev.h, dcs.h, _ptr(asg), None, None, None, flat, *[_ptr(o) for o in outs],
                                           Z.ctypes.data_as(_lib.u64p), dev.stream())
    full = [(0, m)] * 6 + [(0, m + 1)]
    assert call(full) == _lib.RS_OK
    assert call(full[:6] + [(0, m + 2)]) == _lib.RS_ERR_INVALID and b"row range" in dev.lib.rs_last_error()
    assert call([(0, m + 1)] + full[1:]) == _lib.RS_ERR_INVALID
    assert call([(5, 3)] + full[1:]) == _lib.RS_ERR_INVALID
    assert call([(0, 4)] + full[1:]) == _lib.RS_ERR_INVALID and b"same row range" in dev.lib.rs_last_error()  # A_io != A_mid


def test_measured_peaks_are_plausible():
    """rs_measure_peaks (the second denominators of bench.py's rooflines): a device-to-device copy between 2 and 8 TB/s
    (8 TB/s is the HBM3E spec), v_fma_f64 between 15 and 39.3 T lane-operations/s (the spec at 2.4 GHz), the exact-FP64
    modular multiply at a sixth of the FMA rate give or take, the Montgomery product several times slower than that."""
    p = dev_for("toy").measure_peaks()
    assert 2000 < p["hbm_copy_gbs"] < 8000, p
    assert 2000 < p["hbm_read_gbs"] < 8000 and 2000 < p["hbm_inplace_gbs"] < 8000, p
    assert 15 < p["fp64_fma_T"] < 39.4, p
    assert 0.10 < p["fp64_mulmod_G"] / 1e3 / p["fp64_fma_T"] < 0.25, p
    assert 2 < p["fp64_mulmod_G"] / p["int_montmul_G"] < 12, p


def test_msm_with_a_tiled_key_equals_the_explicit_key():
    """crs_window (ringsnark_amd.h): logical element t is read from index t % window."""
    import torch
    dev = dev_for("toy")
    ctx = H.oracle_ctx(dev.prm)
    W, T = 8, 21
    win = dev.put(ctx.random_enc(31, W))
    explicit = torch.cat([win] * 3)[:T].contiguous()
    v = dev.put(ctx.random_ring(32, T))
    exp, _ = dev.msm([explicit], [(v, None, 0)], 1)
    got, _ = dev.msm([win], [(v, None, 0)], 1, crs_len=T, window=W)
    assert (host(got) == host(exp)).all()
    # through the prover entry point
    m = 19
    cs = R.chain_r1cs(m, dev.prm.q)
    asg = dev.put(H.make_assignment(ctx, cs))
    pkw = dict(s_pows=dev.put(ctx.random_enc(41, W)), delta_ts=dev.put(ctx.random_enc(42, W)), delta_mid=dev.put(ctx.random_enc(43, W)),
               alpha=dev.put(ctx.random_enc(44)), beta=dev.put(ctx.random_enc(45)))
    tile = lambda t, n: torch.cat([t] * 4)[:n].contiguous()
    pkx = dict(pkw, s_pows=tile(pkw["s_pows"], m + 1), delta_ts=tile(pkw["delta_ts"], m + 1), delta_mid=tile(pkw["delta_mid"], m))
    dcs = dev.r1cs(cs)
    got, _ = dev.groth16_prove(dcs, pkw, asg, window=W)
    exp, _ = dev.groth16_prove(dcs, pkx, asg)
    assert (host(got) == host(exp)).all()


@pytest.mark.parametrize("name,tile", [("toy", 3), ("toy", 8), ("C2", 64), ("toy60", 5)])
def test_host_resident_key_equals_the_device_resident_one(name, tile):
    """A proving key kept in (page-locked) HOST memory and streamed tile by tile through two device staging buffers
    (rs_msm_hostkey, rs_groth16_pk.host_key: how a key larger than HBM is used on one GPU) gives the same inner
    products and the same proofs as the device-resident key -- with the oracle as the judge of both.  Small staging
    tiles (msm_host_tile) force many copy / compute hand-overs; a tiled (windowed) host key as well."""
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    m = 37 if prm.N_enc <= 128 else 300
    cs = R.wide_r1cs(m, prm.q) if prm.N_enc <= 128 else R.chain_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk = dict(s_pows=ctx.random_enc(71, m + 1), delta_ts=ctx.random_enc(72, m + 1), delta_mid=ctx.random_enc(73, cs.n_aux),
              alpha=ctx.random_enc(74), beta=ctx.random_enc(75))

    def on_host(a):
        hw = dev.host_alloc(a.size)
        hw.array[:] = a.reshape(-1)
        return hw

    hk = {k: (on_host(v) if v.ndim == 5 else dev.put(v)) for k, v in pk.items()}
    dk = {k: dev.put(v) for k, v in pk.items()}
    dcs, dasg = dev.r1cs(cs), dev.put(asg)
    with _lib.tuning(msm_host_tile=tile):
        got_h, empty_h = dev.groth16_prove(dcs, hk, dasg)
        rings = ctx.random_ring(32, m + 1)
        kinds = np.zeros(m + 1, dtype=np.uint8)
        rings[2] = 0
        kinds[4] = O.KIND_ONE
        ip_h, used_h = dev.msm([hk["s_pows"], hk["delta_ts"]], [(dev.put(rings), kinds, 0)], 1, want_used=True)
        # a tiled host key: window of 8 stored elements, logical length m + 1
        w8 = on_host(pk["s_pows"][:8])
        ip_w, _ = dev.msm([w8], [(dev.put(rings), None, 0)], 1, crs_len=m + 1, window=8)
        # a window that is NOT a multiple of the staging tile (12 elements, tiles of 2 / 8 / 4): a tile straddles the wrap
        # and is staged by two copies (round-3 advice: the single copy read past the end of the host buffer)
        w12 = on_host(pk["s_pows"][:12])
        ip_w12, _ = dev.msm([w12], [(dev.put(rings), kinds, 0)], 1, crs_len=m + 1, window=12)
    got_d, empty_d = dev.groth16_prove(dcs, dk, dasg)
    assert empty_h == empty_d and (host(got_h) == host(got_d)).all()
    if prm.N_enc <= 128:
        exp, exp_empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
        assert exp_empty == empty_h and (host(got_h) == exp).all()
    for c, key in enumerate(("s_pows", "delta_ts")):
        exp, used = ctx.inner_product(pk[key], rings, kinds, threads=0)
        assert used_h[0] == used and (host(ip_h)[c, 0] == exp).all()
    exp, _ = ctx.inner_product(pk["s_pows"][:8], rings, None, threads=0, window=8)
    assert (host(ip_w)[0, 0] == exp).all()
    exp, _ = ctx.inner_product(pk["s_pows"][:12], rings, kinds, threads=0, window=12)
    assert (host(ip_w12)[0, 0] == exp).all()


@pytest.mark.parametrize("m,zk", [(20000, True), (40000, False)])
def test_multipass_tuned_sub_transform_kernel_equals_generic(m, zk):
    """M >= 2^15: the multi-pass path runs its 2^13-point sub-transforms through sub_ntt_wide_kernel (32 coefficients
    per thread, forward - table product - inverse fused through registers), which must reproduce the generic kernel bit
    for bit."""
    dev = dev_for("toy44")
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    asg = dev.ring_empty(m + 2)
    dev.fill_uniform(asg[:2], 0, 9)
    dev.chain_assignment(asg, m)
    ds = [dev.put(ctx.random_ring(60 + k)) for k in range(3)] if zk else [None] * 3
    dcs = dev.r1cs(cs)
    keys = ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H")
    runs = {}
    for variant in (0, 1, 2, 3):  # generic, retired, wide (sub_ntt_wide_kernel), retired
        with contextlib.ExitStack() as knob:
            try:
                knob.enter_context(_lib.tuning(witness_sub_ct=variant))
            except _lib.RsError as e:  # 1 and 3 selected superseded A/B kernels
                assert variant in (1, 3) and e.code == _lib.RS_ERR_UNSUPPORTED
                continue
            runs[variant] = {k: host(v) for k, v in dev.witness_map(dcs, asg, *ds).items() if k in keys}
    assert 0 in runs and 2 in runs
    for variant in runs:
        for k in keys:
            assert (runs[variant][k] == runs[0][k]).all(), (variant, k)
    # the product-tree kernels of the 2^13 tiles: level loop not unrolled (0), wave-private radix-8 (1), wide (2)
    for variant, tile in ((0, 13), (1, 13), (2, 13), (2, 14)):  # the wide kernel on 2^13 and on 2^14 tiles
        with _lib.tuning(witness_tree_ct=variant, witness_tree_log=tile):
            got = {k: host(v) for k, v in dev.witness_map(dcs, asg, *ds).items() if k in keys}
            for k in keys:
                assert (got[k] == runs[0][k]).all(), ("tree", variant, tile, k)


@pytest.mark.parametrize("m,zk", [(20000, True), (40000, False), (65536, True)])
def test_two_dimensional_block_convolutions_equal_the_other_paths(m, zk):
    """Ring primes with 2-adicity 14 (what the reference's recipe gives the headline ring, seal_util.hpp:20-32) and
    M >= 2^15: the witness map runs its long products as TWO-DIMENSIONAL block convolutions (blocks of 2^13 coefficients,
    a 2^14-point transform inside a block x a small transform across blocks; sub_ntt_wide_kernel does the heavy part).
    Forced here on well-endowed primes (witness_force_bc = 14), it must reproduce, bit for bit, the full-length
    transforms those primes also allow AND the pairwise block convolutions (witness_bc2 = 0); every path is exact."""
    from ringsnark_amd.device import Device
    prm = P.preset("toy44")
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    keys = ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H")
    runs = {}
    for label, force, bc2, inc in (("full-length", 0, 1, 1), ("two-dimensional", 14, 1, 0), ("pairwise", 14, 0, 0), ("incomplete", 14, 1, 1)):
        with _lib.tuning(witness_force_bc=force, witness_bc2=bc2, witness_inc=inc):  # inc = 1: incomplete transforms, not block convolutions
            dev = Device(prm)  # fresh context: plans are cached per context
            asg = dev.ring_empty(m + 2)
            dev.fill_uniform(asg[:2], 0, 9)
            dev.chain_assignment(asg, m)
            ds = [dev.put(ctx.random_ring(60 + k)) for k in range(3)] if zk else [None] * 3
            dev.set_profiling(True)
            runs[label] = {k: host(v) for k, v in dev.witness_map(dev.r1cs(cs), asg, *ds).items() if k in keys}
            names = {k["name"] for k in dev.profile_read()}
            dev.set_profiling(False)
            assert ("bc2_yfwd_kernel" in names) == (label == "two-dimensional"), (label, names)
            assert ("bc_mac_kernel" in names) == (label == "pairwise"), (label, names)
            assert any(n.startswith("sub_ntt_w") and not n.endswith(", 0>") for n in names) == (label == "incomplete"), (label, names)
            del dev, asg
    for label in ("two-dimensional", "pairwise", "incomplete"):
        for k in keys:
            assert (runs[label][k] == runs["full-length"][k]).all(), (label, k)


def test_multipass_production_tile_matches_oracle_on_a_few_slots():
    """The multi-pass path at its production tile (2^13) against the oracle's O(m^2) map: m = 16400 (M = 2^15), four
    slots per limb (rs_witness_map_slots), oracle spread over the host cores."""
    dev = dev_for("toy44")
    prm = dev.prm
    m, slot0, ns = 16400, 10, 4
    cs = R.chain_r1cs(m, prm.q)
    asg = dev.ring_empty(m + 2)
    dev.fill_uniform(asg[:2], 0, 11)
    dev.chain_assignment(asg, m)
    w = dev.witness_map_slots(dev.r1cs(cs), asg, slot0, ns, want=("A_io", "A_mid", "B_mid", "H"))
    a = host(asg)
    ocs = H.oracle_cs(cs)
    for limb in range(prm.L):
        exp = O.witness_map(prm.q[limb], ocs, limb, np.ascontiguousarray(a[:, limb, slot0:slot0 + ns]), threads=0)
        for k in ("A_io", "A_mid", "B_mid", "H"):
            assert (host(w[k])[:, limb, :] == exp[k]).all(), (k, limb)


@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "toy54", "toy60"])
def test_poly_multiply_add_divide_match_oracle(name):
    """Row a11 (util/polynomials.tcc:62-81): per-slot polynomial product / sum / quotient with ring-element
    coefficients, non-monic per-slot divisors included, against the oracle's schoolbook restatement."""
    dev = dev_for(name)
    prm = dev.prm
    ctx = H.oracle_ctx(prm)
    na, nb = 23, 9
    a, b = ctx.random_ring(91, na), ctx.random_ring(92, nb)
    a[5] = 0
    prod = host(dev.poly_multiply(dev.put(a), dev.put(b)))
    sm = host(dev.poly_add(dev.put(a), dev.put(b)))
    num = ctx.random_ring(93, na + nb - 1)
    quo = host(dev.poly_divide(dev.put(num), dev.put(b)))
    for limb in range(prm.L):
        q = prm.q[limb]
        assert (prod[:, limb, :] == O.poly_mul(q, np.ascontiguousarray(a[:, limb, :]), np.ascontiguousarray(b[:, limb, :]))).all()
        exp, n = O.poly_div_general(q, np.ascontiguousarray(num[:, limb, :]), np.ascontiguousarray(b[:, limb, :]))
        assert (quo[:, limb, :] == exp[:quo.shape[0]]).all()
    pad = np.zeros((na - nb,) + b.shape[1:], dtype=np.uint64)
    assert (sm == ctx.ring_add(a, np.concatenate([b, pad]))).all()
    # normalisation (Boost polynomial): trailing zero coefficients are stripped from operands and results
    z = np.concatenate([a, np.zeros((3,) + a.shape[1:], dtype=np.uint64)])
    assert dev.poly_multiply(dev.put(z), dev.put(b)).shape[0] == na + nb - 1
    assert dev.poly_divide(dev.put(b), dev.put(a)).shape[0] == 0  # deg num < deg den: the zero polynomial
    # C contract (ringsnark_amd.h): rows of the NOMINAL output beyond the result are zero, whatever the buffer held
    import torch
    buf = torch.full((na + 3 + nb - 1, prm.L, prm.N), -1, dtype=torch.int64, device=dev.device)
    r = dev.poly_multiply(dev.put(z), dev.put(b), out=buf)
    assert r.shape[0] == na + nb - 1 and not host(buf[na + nb - 1:]).any() and (host(r) == prod).all()
    znum = np.concatenate([num, np.zeros((4,) + num.shape[1:], dtype=np.uint64)])
    buf = torch.full((na + nb - 1 + 4 - nb + 1, prm.L, prm.N), -1, dtype=torch.int64, device=dev.device)
    r = dev.poly_divide(dev.put(znum), dev.put(b), out=buf)
    assert r.shape[0] == quo.shape[0] and not host(buf[quo.shape[0]:]).any() and (host(r) == quo).all()
    # a denominator with zero leading coefficients has a longer quotient than nn - nd + 1 rows: refused, not overrun
    zden = np.concatenate([b, np.zeros((2,) + b.shape[1:], dtype=np.uint64)])
    with pytest.raises(_lib.RsError) as ei:
        dev.poly_divide(dev.put(num), dev.put(zden))
    assert ei.value.code == _lib.RS_ERR_INVALID
    # the divisor's leading coefficient must be a unit of the ring
    bad = b.copy()
    bad[-1, 0, 3] = 0
    with pytest.raises(_lib.RsError) as ei:
        dev.poly_divide(dev.put(num), dev.put(bad))
    assert ei.value.code == _lib.RS_ERR_NOT_INVERTIBLE and "element is not invertible in ring" in str(ei.value)


@pytest.mark.parametrize("name,bc,m,kind,zk", [("toy", 5, 100, "wide", True), ("toy", 5, 64, "chain", False), ("toy", 6, 300, "wide", True),
                                               ("toy", 5, 70, "many_inputs", False), ("toy60", 5, 200, "wide", True),
                                               ("toyR", 0, 600, "wide", True), ("toyR", 0, 1000, "chain", False)])
def test_witness_map_block_convolution_path_matches_oracle(name, bc, m, kind, zk):
    """VERDICT r1 missing #3: ring primes that lack a 2M-th root of unity (the reference's recipe only guarantees
    q = 1 mod 2*N_inner, seal_util.hpp:20-32).  The witness map then runs on block convolutions; forced here on
    well-endowed primes through the witness_force_bc knob (bc = largest transform length, log2) and taken naturally
    by preset toyR (recipe primes).  Complete oracle comparison, both arithmetics."""
    from ringsnark_amd.device import Device
    prm = P.preset(name)
    if bc == 0:
        need = (m - 1).bit_length() + 1
        assert min(P.two_adicity(q) for q in prm.q) < need, "preset happens to have enough 2-adicity; pick a larger m"
    with _lib.tuning(witness_force_bc=bc):
        dev = Device(prm)  # fresh context: plans are cached per context
        ctx = H.oracle_ctx(prm)
        cs = {"wide": lambda: R.wide_r1cs(m, prm.q), "chain": lambda: R.chain_r1cs(m, prm.q),
              "many_inputs": lambda: R.wide_r1cs(m, prm.q, n_inputs=70)}[kind]()
        asg = H.make_assignment(ctx, cs)
        ds = [ctx.random_ring(60 + k) for k in range(3)] if zk else [None] * 3
        w = dev.witness_map(dev.r1cs(cs), dev.put(asg), *[dev.put(d) if d is not None else None for d in ds])
        got = {k: host(v) if k != "Z" else v for k, v in w.items()}
    ocs = H.oracle_cs(cs)
    for limb in range(prm.L):
        dl = [np.ascontiguousarray(d[limb]) if d is not None else None for d in ds]
        exp = O.witness_map(prm.q[limb], ocs, limb, np.ascontiguousarray(asg[:, limb, :]), *dl)
        for k in ("A_io", "B_io", "C_io", "A_mid", "B_mid", "C_mid", "H"):
            assert (got[k][:, limb, :] == exp[k]).all(), (k, limb)
        assert (got["Z"][limb] == exp["Z"]).all()


def test_groth16_prover_on_recipe_primes_matches_oracle():
    """The prover end to end on preset toyR at a size whose witness map needs the block-convolution path."""
    from ringsnark_amd.device import Device
    prm = P.preset("toyR")
    dev, ctx = Device(prm), H.oracle_ctx(prm)
    m = 200
    assert min(P.two_adicity(q) for q in prm.q) < (m - 1).bit_length() + 1
    cs = R.wide_r1cs(m, prm.q)
    asg = H.make_assignment(ctx, cs)
    pk = dict(s_pows=ctx.random_enc(71, m + 1), delta_ts=ctx.random_enc(72, m + 1), delta_mid=ctx.random_enc(73, cs.n_aux),
              alpha=ctx.random_enc(74), beta=ctx.random_enc(75))
    exp, exp_empty = O.groth16_prove(ctx, H.oracle_cs(cs), pk, asg)
    got, empty = dev.groth16_prove(dev.r1cs(cs), {k: dev.put(v) for k, v in pk.items()}, dev.put(asg))
    assert empty == exp_empty and (host(got) == exp).all()


@pytest.mark.gpu
def test_steady_state_proofs_allocate_nothing_and_repeat_bit_for_bit():
    """A prover process proves again and again: after the first proof of a (context, m) -- plan tables, the cached Z rows
    of Rinocchio (witness_Z_rows), first-call workspaces -- further proofs must not take device memory, and must return
    the same bytes (the witness map and the inner products are deterministic).  Both provers, ZK on."""
    import torch

    from ringsnark_amd.device import Device, to_host
    prm = P.preset("C2")
    dev = Device(prm)
    m = 1 << 10
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    asg = dev.ring_empty(m + 2)
    dev.fill_uniform(asg[:2], 0, 7)
    dev.chain_assignment(asg, m)
    W = 1 << 8
    gk = {k: dev.fill_uniform(dev.enc_empty(W), 1, 13 + i) for i, k in enumerate(("s_pows", "delta_ts", "delta_mid"))}
    gk["alpha"], gk["beta"] = dev.fill_uniform(dev.enc_empty(), 1, 16), dev.fill_uniform(dev.enc_empty(), 1, 17)
    rk = {k: dev.fill_uniform(dev.enc_empty(W), 1, 22 + i) for i, k in enumerate(("s_pows", "alpha_s_pows", "beta_prods"))}
    for i, k in enumerate(("beta_rv_ts", "beta_rw_ts", "beta_ry_ts")):
        rk[k] = dev.fill_uniform(dev.enc_empty(), 1, 25 + i)
    ds = [dev.fill_uniform(dev.ring_empty(), 0, 30 + k) for k in range(3)]

    def both():
        a = dev.groth16_prove(dcs, gk, asg, want_empty=False, window=W)[0]
        b = dev.rinocchio_prove(dcs, rk, asg, *ds, window=W)[0]
        torch.cuda.synchronize()
        return to_host(a), to_host(b)

    first = both()
    both()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        got = both()
        assert (got[0] == first[0]).all() and (got[1] == first[1]).all()
    torch.cuda.empty_cache()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 <= (8 << 20), "device memory taken by steady-state proofs: %d bytes" % (free0 - free1)
