"""ringsnark_amd/batch.h: B assignments of one system proved against one key in one pass over every key vector.

Every sum of an inner product is exact modulo Q_j, so proof b of a batch is WORD FOR WORD the proof of the existing
single-assignment prover for member b on the same key: every expected value is that prover's output, every comparison is
equality of uint64 words and of the `empty` lists.  Members are H.make_assignment(ctx, cs, seed=7 + b): they differ.
The shapes, seeds and systems are those of tests/test_keygen.py and tests/test_seeded.py."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests.test_keygen import VECTORS, device_for, device_keygen, disjoint_seeds, systems
from tests.test_seeded import PATTERN, expanded, first_elements, prove, residues, seeded_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ringsnark_amd", "batch.h")
SCHEMES = ("groth16", "rinocchio")
N_ELEMS = {"groth16": 3, "rinocchio": 9}


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_library_exports_every_function_of_batch_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.BATCH_SIGNATURES) and len(names) == 5
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 106
    assert re.search(r"#define\s+RS_MAX_BATCH\s+8\b", code)


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++17")])
def test_batch_h_compiles_on_its_own(tmp_path, lang, std):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no compiler")
    src = tmp_path / ("only." + ("c" if lang == "c" else "cpp"))
    src.write_text("#include <ringsnark_amd/batch.h>\nint main(void) { return RS_MAX_BATCH == 8 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-std=" + std, "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- GPU helpers -----------------------------------------------------------------------------------------------------
def prove_batch(dev, scheme, dcs, pk, asgs, d=None, **kw):
    """(words [B][3 | 9][...], empties [B][3 | 9], the device tensor)"""
    from ringsnark_amd.device import to_host
    if scheme == "groth16":
        proofs, empties = dev.groth16_prove_batch(dcs, pk, asgs, **kw)
    else:
        proofs, empties = dev.rinocchio_prove_batch(dcs, pk, asgs, d=d, **kw)
    return to_host(proofs), empties, proofs


def singles(dev, scheme, dcs, pk, asgs, ds=None, kinds=None, **kw):
    """the existing prover, member by member: [(words, empty)]"""
    out = []
    for b, a in enumerate(asgs):
        d = (None, None, None) if ds is None else tuple(ds[b])
        k = {} if kinds is None or kinds[b] is None else {"kinds": kinds[b]}
        w, e, _ = prove(dev, scheme, dcs, pk, a, d, **k, **kw)
        out.append((w, e))
    return out


def assert_equal(got, exp, what=None):
    words, empties, _ = got
    assert len(empties) == len(exp) and words.shape[0] == len(exp), what
    for b, (w, e) in enumerate(exp):
        assert empties[b] == e, (what, b, empties[b], e)
        assert (words[b].reshape(-1) == w.reshape(-1)).all(), (what, b)


def stack_d(dev, ds, B):
    import torch
    return None if ds is None else torch.stack([torch.stack(list(ds[b])) for b in range(B)]).contiguous()


@functools.lru_cache(maxsize=None)
def batch_case(name, scheme, m, zk, oracle_sk=True):
    """per (preset, scheme): device, chain system, a seeded device key and its expansion (the full device key), eight
    different members, and the single prover's proof of every member on the full key -- computed once"""
    prm = P.preset(name)
    dev = device_for(name)
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    sk = None if oracle_sk else residues(np.random.RandomState(2), prm.Q, prm.N_enc)
    dcs, vk, pk = seeded_case(dev, scheme, name, cs, sk=sk)
    wide = expanded(dev, scheme, pk)
    asgs = [dev.put(H.make_assignment(ctx, cs, seed=7 + b)) for b in range(8)]
    ds = [tuple(dev.put(x) for x in ctx.random_ring(77 + b, 3)) for b in range(8)] if zk else None
    exp = singles(dev, scheme, dcs, wide, asgs, ds)
    assert any((exp[0][0] != e[0]).any() for e in exp[1:])
    return dict(prm=prm, dev=dev, ctx=ctx, cs=cs, dcs=dcs, vk=vk, pk=pk, wide=wide, asgs=asgs, ds=ds, exp=exp, sk=sk)


TOY_CASES = [("toy", "groth16", False), ("toy", "rinocchio", True), ("toy49", "groth16", False), ("toy49", "rinocchio", False),
             ("toy50", "groth16", False), ("toy50", "rinocchio", False),
             ("toy60", "groth16", False), ("toy60", "rinocchio", False)]


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,scheme,zk", TOY_CASES)
def test_batch_on_a_full_device_key_equals_the_single_proofs(name, scheme, zk):
    """m = 21, 22 elements per vector.  B = 3 Rinocchio: 13 groups, two full blocks of six and a partial one; B = 8: 16 / 33
    groups, the limit."""
    c = batch_case(name, scheme, 21, zk)
    dev, dcs = c["dev"], c["dcs"]
    for B in (1, 2, 3, 8):
        got = prove_batch(dev, scheme, dcs, c["wide"], c["asgs"][:B], stack_d(dev, c["ds"], B))
        assert got[0].shape[:2] == (B, N_ELEMS[scheme])
        assert_equal(got, c["exp"][:B], B)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["seeded", "host", "seeded_host"])
@pytest.mark.parametrize("name,scheme,zk", TOY_CASES)
def test_batch_on_streamed_keys_crosses_tile_boundaries(name, scheme, zk, kind):
    """tiles of one element, two full tiles of 8 and a partial one, a single tile of 64; B = 3"""
    from ringsnark_amd import _lib
    c = batch_case(name, scheme, 21, zk)
    dev, dcs, B = c["dev"], c["dcs"], 3
    if kind == "seeded":
        pk = c["pk"]
    elif kind == "seeded_host":
        _, _, pk = seeded_case(dev, scheme, name, c["cs"], host=True, tile=4)
    else:
        pk = device_keygen(dev, scheme, dcs, c["vk"], seeds=disjoint_seeds(700, len(VECTORS[scheme])), host=True, tile=4)
    exp = singles(dev, scheme, dcs, pk, c["asgs"][:B], c["ds"])  # the existing prover on the SAME key
    if kind != "host":
        for (w, e), (w0, e0) in zip(exp, c["exp"]):
            assert e == e0 and (w == w0).all()
    for t in (1, 8, 64):
        with _lib.tuning(msm_host_tile=t):
            got = prove_batch(dev, scheme, dcs, pk, c["asgs"][:B], stack_d(dev, c["ds"], B))
        assert_equal(got, exp, t)


@pytest.mark.gpu
@pytest.mark.parametrize("lin_io", [1, 0])
@pytest.mark.parametrize("host", [False, True])
def test_wide_kernels_groth16(host, lin_io):
    """C2 (N = 4096, N_enc = 8192, K = 4), chain_r1cs(8): the linear-form io path applies (m >= 6).  B = 3: six groups in
    one mac_kernel_v3g launch; B = 4: 6 + 2."""
    from ringsnark_amd import _lib
    c = batch_case("C2", "groth16", 8, False, False)
    dev, dcs = c["dev"], c["dcs"]
    pk = c["wide"]
    if host:
        _, _, pk = seeded_case(dev, "groth16", "C2", c["cs"], host=True, sk=c["sk"])
    with _lib.tuning(prover_lin_io=lin_io):
        exp = singles(dev, "groth16", dcs, pk, c["asgs"][:4])
        for B in (3, 4):
            assert_equal(prove_batch(dev, "groth16", dcs, pk, c["asgs"][:B]), exp[:B], B)
    for (w, e), (w0, e0) in zip(exp, c["exp"]):
        assert e == e0 and (w == w0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
def test_wide_kernels_rinocchio(host):
    """C2, B = 2: nine groups, mac_kernel_v4 blocks of 6 + 3"""
    c = batch_case("C2", "rinocchio", 8, False, False)
    dev, dcs = c["dev"], c["dcs"]
    pk = c["wide"]
    if host:
        _, _, pk = seeded_case(dev, "rinocchio", "C2", c["cs"], host=True, sk=c["sk"])
    exp = singles(dev, "rinocchio", dcs, pk, c["asgs"][:2])
    assert_equal(prove_batch(dev, "rinocchio", dcs, pk, c["asgs"][:2]), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_wide_kernels_at_16384_points(scheme):
    """C5s (N_enc = 16384, K = 8), chain_r1cs(2), B = 2: the LOGN = 14 instantiations"""
    c = batch_case("C5s", scheme, 2, False, False)
    assert_equal(prove_batch(c["dev"], scheme, c["dcs"], c["wide"], c["asgs"][:2]), c["exp"][:2])


def launches(dev, fn):
    """name -> launches of the kernels that fn() ran"""
    dev.set_profiling(True)
    try:
        dev.profile_read()
        fn()
        return {r["name"]: r["launches"] for r in dev.profile_read()}
    finally:
        dev.set_profiling(False)


@pytest.mark.gpu
def test_a_seeded_key_is_expanded_once_per_batch():
    from ringsnark_amd import _lib
    c = batch_case("toy", "groth16", 21, False)
    dev, dcs, B = c["dev"], c["dcs"], 4
    with _lib.tuning(msm_host_tile=8):
        one = launches(dev, lambda: prove(dev, "groth16", dcs, c["pk"], c["asgs"][0]))
        four = launches(dev, lambda: singles(dev, "groth16", dcs, c["pk"], c["asgs"][:B]))
        batch = launches(dev, lambda: prove_batch(dev, "groth16", dcs, c["pk"], c["asgs"][:B]))
    k = "expand_seeded_tile_kernel"
    assert one[k] == 9  # three vectors of 22, 21, 22 elements in tiles of 8
    assert batch[k] == one[k] and 4 * batch[k] == four[k]


@pytest.mark.gpu
def test_six_groups_share_one_multiply_accumulate_launch():
    """C2 at m = 3 (not the linear-form case): a ringGroth16 batch of 3 is one launch per pass, for 6, 3 and 3 groups"""
    c = batch_case("C2", "groth16", 3, False, False)
    dev, dcs = c["dev"], c["dcs"]
    count = lambda rec: sum(n for name, n in rec.items() if name.startswith("mac_kernel_v3"))
    one = launches(dev, lambda: prove(dev, "groth16", dcs, c["wide"], c["asgs"][0]))
    batch = launches(dev, lambda: prove_batch(dev, "groth16", dcs, c["wide"], c["asgs"][:3]))
    assert count(one) == 3 and one.get("mac_kernel_v3") == 3
    assert count(batch) == 3 and batch.get("mac_kernel_v3g") == 3
    assert_equal(prove_batch(dev, "groth16", dcs, c["wide"], c["asgs"][:3]), c["exp"][:3])


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_an_all_zero_member_reports_its_own_empty_elements(scheme, zk):
    import torch
    c = batch_case("toy", scheme, 21, zk)
    dev, dcs = c["dev"], c["dcs"]
    asgs = [c["asgs"][0], torch.zeros_like(c["asgs"][1]), c["asgs"][2]]
    exp = singles(dev, scheme, dcs, c["wide"], asgs, c["ds"])
    if scheme == "groth16":
        assert exp[1][1] == [0, 0, 1] and exp[0][1] == [0, 0, 0]  # the single prover reports the EMPTY C
    assert exp[0][1] == c["exp"][0][1] and exp[2][1] == c["exp"][2][1]  # the neighbours' are unaffected
    assert_equal(prove_batch(dev, scheme, dcs, c["wide"], asgs, stack_d(dev, c["ds"], 3)), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_wire_kinds_of_one_member(scheme, zk, seeded):
    from ringsnark_amd import _lib
    c = batch_case("toy", scheme, 21, zk)
    dev, dcs, cs = c["dev"], c["dcs"], c["cs"]
    pk = c["pk"] if seeded else c["wide"]
    k = np.full(cs.n_vars, _lib.RS_KIND_POLY, dtype=np.uint8)
    k[cs.n_inputs + 2] = _lib.RS_KIND_ONE
    kinds = [None, k, None]
    exp = singles(dev, scheme, dcs, pk, c["asgs"][:3], c["ds"], kinds=kinds)
    assert (exp[1][0] != c["exp"][1][0]).any() and (exp[0][0] == c["exp"][0][0]).all()
    assert_equal(prove_batch(dev, scheme, dcs, pk, c["asgs"][:3], stack_d(dev, c["ds"], 3), kinds=kinds), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_without_auxiliary_variables(scheme):
    prm = P.preset("toy")
    dev = device_for("toy")
    ctx = H.oracle_ctx(prm)
    label, cs = systems(prm.q)[-1]
    assert label == "no_aux" and cs.n_aux == 0
    dcs, vk, pk = seeded_case(dev, scheme, "toy", cs)
    asgs = [dev.put(ctx.random_ring(8 + b, cs.n_vars)) for b in range(3)]
    for key in (expanded(dev, scheme, pk), pk):
        assert_equal(prove_batch(dev, scheme, dcs, key, asgs), singles(dev, scheme, dcs, key, asgs))


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("window", [8, 6])
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_batch_on_a_windowed_key(scheme, zk, window, host):
    """window = 6 with tiles of 4: the second tile straddles the wrap (tests/test_seeded.py::test_windowed_seeded_key)"""
    from ringsnark_amd import _lib
    c = batch_case("toy", scheme, 21, zk)
    dev, dcs, B = c["dev"], c["dcs"], 2
    d = stack_d(dev, c["ds"], B)
    full = first_elements(dev, scheme, c["wide"], window)
    exp = singles(dev, scheme, dcs, full, c["asgs"][:B], c["ds"], window=window)
    assert (exp[0][0] != c["exp"][0][0]).any()
    assert_equal(prove_batch(dev, scheme, dcs, full, c["asgs"][:B], d, window=window), exp)
    pk = c["pk"]
    if host:
        _, _, pk = seeded_case(dev, scheme, "toy", c["cs"], host=True)
    cut = first_elements(dev, scheme, pk, window)
    for t in (64, 4):
        with _lib.tuning(msm_host_tile=t):
            assert_equal(prove_batch(dev, scheme, dcs, cut, c["asgs"][:B], d, window=window), exp, t)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_every_proof_verifies_with_its_own_inputs_only(scheme, zk):
    c = batch_case("toy", scheme, 21, zk)
    dev, dcs, cs, B = c["dev"], c["dcs"], c["cs"], 3
    _, empties, proofs = prove_batch(dev, scheme, dcs, c["pk"], c["asgs"][:B], stack_d(dev, c["ds"], B))
    vk = dev.groth16_vk(dcs, c["vk"]) if scheme == "groth16" else dev.rinocchio_vk(dcs, c["vk"])
    verify = dev.groth16_verify if scheme == "groth16" else dev.rinocchio_verify
    for b in range(B):
        for other in range(B):
            primary = c["asgs"][other][: cs.n_inputs].contiguous()
            assert bool(verify(vk, primary, proofs[b].contiguous(), empties[b]).accepted) == (other == b), (b, other)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_batch_size_out_of_range_is_refused_before_anything_is_written(scheme):
    import torch
    from ringsnark_amd import _lib
    c = batch_case("toy", scheme, 21, scheme == "rinocchio")
    dev, dcs = c["dev"], c["dcs"]
    asgs = [c["asgs"][b % 8] for b in range(9)]
    ptrs = (C.c_void_p * 9)(*[a.data_ptr() for a in asgs])
    proofs = torch.full((9, N_ELEMS[scheme], dev.L, 2, dev.K, dev.N_enc), PATTERN, dtype=torch.int64, device=dev.device)
    empty = (C.c_int * (9 * 9))(*([7] * 81))
    dev.sync()
    for seeded in (False, True):
        key = c["pk"] if seeded else c["wide"]
        if scheme == "groth16":
            s, _ = dev._groth16_key(key, 0)
            fn = dev.lib.rs_groth16_prove_batch_seeded if seeded else dev.lib.rs_groth16_prove_batch
            call = lambda B: fn(dev.h, dcs.h, C.byref(s), B, ptrs, None, proofs.data_ptr(), empty, None)
        else:
            s, _ = dev._rinocchio_key(key, 0)
            fn = dev.lib.rs_rinocchio_prove_batch_seeded if seeded else dev.lib.rs_rinocchio_prove_batch
            call = lambda B: fn(dev.h, dcs.h, C.byref(s), B, ptrs, None, None, proofs.data_ptr(), empty, None)
        for B in (0, 9, -1):
            assert call(B) == _lib.RS_ERR_INVALID
            assert "1..8" in dev.lib.rs_last_error().decode()
            dev.sync()
            assert bool((proofs == PATTERN).all()) and all(e == 7 for e in empty)
    for B in (0, 9):
        with pytest.raises(_lib.RsError) as e:
            prove_batch(dev, scheme, dcs, c["wide"], asgs[:B])
        assert e.value.code == _lib.RS_ERR_INVALID
    n = C.c_size_t(0)
    assert dev.lib.rs_prove_batch_bytes(dev.h, dcs.h, 0, 9, C.byref(n)) == _lib.RS_ERR_INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_check_names_the_member_that_violates_the_system(scheme):
    c = batch_case("toy", scheme, 21, scheme == "rinocchio")
    dev, dcs, cs = c["dev"], c["dcs"], c["cs"]
    bad = c["asgs"][2].clone()
    bad[cs.n_inputs + 4, 1, 3] += 1  # x_6: the product of constraint 4 (and a factor of constraints 5 and 6)
    asgs = [c["asgs"][0], c["asgs"][1], bad]
    with pytest.raises(ValueError, match=r"member 2.*first constraint 4 "):
        prove_batch(dev, scheme, dcs, c["wide"], asgs, stack_d(dev, c["ds"], 3), check=True)
    got = prove_batch(dev, scheme, dcs, c["wide"], c["asgs"][:3], stack_d(dev, c["ds"], 3), check=True)
    assert_equal(got, c["exp"][:3])


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_workspace_bytes_are_affine_in_the_batch_size(scheme):
    c = batch_case("toy", scheme, 21, scheme == "rinocchio")
    dev, dcs, m = c["dev"], c["dcs"], 21
    b1, b2, b3 = (dev.prove_batch_bytes(dcs, scheme, B) for B in (1, 2, 3))
    assert b2 - b1 == b3 - b2 > 0
    vecs = ((5 if scheme == "groth16" else 4) * m + 1) * dev.ring_words * 8
    for B, b in ((1, b1), (2, b2), (3, b3)):
        assert b >= B * vecs


@pytest.mark.gpu
@pytest.mark.parametrize("name,T", [("toy", 11), ("C2", 5)])
def test_msm_takes_more_than_six_groups(name, T):
    """rs_msm, rs_msm_hostkey and rs_msm_seeded with 7 and 13 groups of different lengths against one and two key vectors
    (14 and 26 sets: the reduction in blocks of 12) equal one call per group.  C2: mac_kernel_v3g blocks of 6 + 1 and
    mac_kernel_v4 blocks of 6 + 6 + 1."""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    prm = P.preset(name)
    dev = device_for(name)
    rng = np.random.RandomState(6)
    c0 = [dev.put(np.stack([residues(rng, prm.Q, prm.N_enc) for _ in range(T * prm.L)]).reshape(T, prm.L, prm.K, prm.N_enc)) for _ in range(2)]
    pub = [5, 5 + (1 << 40)]
    wide = [dev.enc_expand_seeded(c, p) for c, p in zip(c0, pub)]
    vecs = [(dev.put(np.stack([residues(rng, prm.q, prm.N) for _ in range(T - g % 3)])), None, g) for g in range(13)]
    one = [to_host(dev.msm(wide, [(v[0], None, 0)], 1, want_used=True)[0]) for v in vecs]  # [2][1] elements each
    hosted = []
    for w in wide:
        hw = dev.host_alloc(w.numel())
        hw.fill_from(w)
        hosted.append(hw)
    for G in (7, 13):
        for n_crs in (1, 2):
            exp = np.stack([np.stack([one[g][c, 0] for g in range(G)]) for c in range(n_crs)])
            got, used = dev.msm(wide[:n_crs], vecs[:G], G, want_used=True)
            assert (to_host(got) == exp).all(), (G, n_crs)
            assert used == [T - g % 3 for g in range(G)]
            with _lib.tuning(msm_host_tile=4):
                assert (to_host(dev.msm(hosted[:n_crs], vecs[:G], G)[0]) == exp).all(), (G, n_crs, "host")
                assert (to_host(dev.msm(c0[:n_crs], vecs[:G], G, pub_seeds=pub[:n_crs])[0]) == exp).all(), (G, n_crs, "seeded")
    with pytest.raises(_lib.RsError):
        dev.msm(wide[:1], [(vecs[0][0], None, g) for g in range(34)], 34)
