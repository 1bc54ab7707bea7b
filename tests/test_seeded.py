"""ringsnark_amd/seeded.h: seeded proving keys -- a key vector stored as its c0 halves and one public seed, c1 regenerated on
the device where the key is read.

Everything is exact, so every comparison is equality of uint64 words, and the expected value always comes from a path that
has oracle parity of its own (tests/test_keygen.py, tests/test_gpu_parity.py): rs_enc_encode, the full-format generators, and
the provers on a full-format key.  The shapes, seeds and systems are those of tests/test_keygen.py."""
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
from tests.test_keygen import (STRIDE, VECTORS, device_for, device_keygen, disjoint_seeds, key_rows, key_words, systems, trapdoor,
                               with_r_y)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ringsnark_amd", "seeded.h")
SINGLES = {"groth16": ("alpha", "beta"), "rinocchio": ("beta_rv_ts", "beta_rw_ts", "beta_ry_ts")}
PATTERN = 0x5A5A5A5A5A5A5A5A


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_library_exports_every_function_of_seeded_h(tmp_path):
    from ringsnark_amd import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.SEEDED_SIGNATURES) and len(names) == 6
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 105
    # the structures of the binding have the header's layout: sizes and member offsets as the C compiler sees them
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    mirrors = {"rs_groth16_seeded_key_out": _lib.Groth16SeededKeyOut, "rs_rinocchio_seeded_key_out": _lib.RinocchioSeededKeyOut,
               "rs_groth16_pk_seeded": _lib.Groth16PKSeeded, "rs_rinocchio_pk_seeded": _lib.RinocchioPKSeeded}
    lines = []
    for cname, py in mirrors.items():
        members = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), code, flags=re.S).group(1)
        fields = [f for decl in members.split(";") for f in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert fields == [f[0] for f in py._fields_], (cname, fields)
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f in fields]
        lines.append('printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include <ringsnark_amd/seeded.h>\nint main(void) {\n%s\nreturn 0;\n}\n" % "\n".join(lines))
    exe = str(tmp_path / "layout")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for line in subprocess.run([exe], capture_output=True, text=True).stdout.splitlines():
        cname, size, *offsets = line.split()
        py = mirrors[cname]
        assert C.sizeof(py) == int(size), cname
        assert [getattr(py, f[0]).offset for f in py._fields_] == [int(o) for o in offsets], cname


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++17")])
def test_seeded_h_compiles_on_its_own(tmp_path, lang, std):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no compiler")
    src = tmp_path / ("only." + ("c" if lang == "c" else "cpp"))
    src.write_text("#include <ringsnark_amd/seeded.h>\nint main(void) { return 0; }\n")
    r = subprocess.run([cc, "-x", lang, "-std=" + std, "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- GPU helpers -----------------------------------------------------------------------------------------------------
def residues(rng, moduli, n):
    return np.stack([rng.randint(0, 2**62, size=n, dtype=np.int64).astype(np.uint64) % np.uint64(p) for p in moduli])


def words(dev, v):
    """a key vector (device tensor or HostWords) as uint64 words"""
    return key_words(dev, v)


def c0_blocks(full):
    """[count][L][2][K][n] -> the compact layout [count][L][K][n]"""
    return full[..., 0, :, :].contiguous()


def on_device(dev, v):
    """a compact vector as a device tensor [count][L][K][n]"""
    from ringsnark_amd.device import HostWords
    if isinstance(v, HostWords):
        return dev.put(np.array(v.array).reshape(-1, dev.L, dev.K, dev.N_enc))
    return v


def expanded(dev, scheme, pk):
    """the full-format key of a seeded one: rs_enc_expand_seeded of every vector"""
    out = {}
    for v, name in enumerate(VECTORS[scheme]):
        if name in SINGLES[scheme] or pk[name] is None:
            out[name] = pk[name]
        else:
            out[name] = dev.enc_expand_seeded(on_device(dev, pk[name]), pk["pub_seeds"][v])
    return out


def first_elements(dev, scheme, pk, count):
    """the key with its three vectors cut to `count` elements (a windowed key)"""
    from ringsnark_amd.device import HostWords
    out = dict(pk)
    for name in VECTORS[scheme][:3]:
        v = pk[name]
        if isinstance(v, HostWords):
            key_words_ = dev.enc_words // 2 if "pub_seeds" in pk else dev.enc_words
            out[name] = dev.host_alloc(count * key_words_)
            out[name].array[:] = v.array[: count * key_words_]
        else:
            out[name] = v[:count].contiguous()
    return out


def prove(dev, scheme, dcs, pk, asg, d=(None, None, None), **kw):
    from ringsnark_amd.device import to_host
    if scheme == "groth16":
        proof, empty = dev.groth16_prove(dcs, pk, asg, **kw)
    else:
        proof, empty = dev.rinocchio_prove(dcs, pk, asg, d[0], d[1], d[2], **kw)
    return to_host(proof), empty, proof


PUB = 31337  # public seeds PUB + v * 2^40: disjoint from the private seeds 700 + v * 2^40 of the cases below


def seeded_case(dev, scheme, name, cs, host=False, tile=0, seeds=700, pub=PUB, sk=None):
    """(dcs, trapdoor, seeded key with independent public seeds)"""
    prm = P.preset(name)
    sk = H.oracle_ctx(prm).keygen(3) if sk is None else sk
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 11, sk), prm.q)
    dcs = dev.r1cs(cs)
    n = len(VECTORS[scheme])
    pk = device_keygen(dev, scheme, dcs, vk, seeds=disjoint_seeds(seeds, n), seeded=True, pub_seeds=disjoint_seeds(pub, n), host=host, tile=tile)
    return dcs, vk, pk


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,count", [("toy", 5), ("toy49", 5), ("toy50", 5), ("toy60", 5), ("C2", 3), ("C5s", 2)])
def test_expansion_equals_the_encoder(name, count):
    """c0 of rs_enc_encode's elements and the same seed give the elements back: c1 is the encoder's stream, % Q_j by the
    Barrett form (toy60: 60-bit Q_j on the integer arithmetic).  C2: N_enc = 8192, K = 4 (four workgroups per row); C5s:
    N_enc = 16384, K = 8.  A slice expanded with its first stored index gives the slice."""
    from ringsnark_amd.device import to_host
    prm = P.preset(name)
    dev = device_for(name)
    rng = np.random.RandomState(4)
    sk = dev.put(residues(rng, prm.Q, prm.N_enc))
    rings = dev.put(np.stack([residues(rng, prm.q, prm.N) for _ in range(count)]))
    full = dev.enc_encode(sk, rings, 9)
    c0 = c0_blocks(full)
    assert c0.shape == (count, prm.L, prm.K, prm.N_enc)
    exp = to_host(full)
    assert (to_host(dev.enc_expand_seeded(c0, 9)) == exp).all()
    first = 3 if count > 3 else count - 1
    assert (to_host(dev.enc_expand_seeded(c0[first:].contiguous(), 9, first=first)) == exp[first:]).all()
    assert (to_host(dev.enc_expand_seeded(c0[first:].contiguous(), 9)) != exp[first:]).any()  # the stream index is the stored index


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
@pytest.mark.parametrize("name", ["toy", "toy49", "toy50", "toy60"])
def test_seeded_keygen_is_c0_of_the_full_key_when_the_seeds_coincide(name, scheme):
    from ringsnark_amd.device import to_host
    prm = P.preset(name)
    dev = device_for(name)
    sk = H.oracle_ctx(prm).keygen(3)
    for label, cs in systems(prm.q):
        vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 11, sk), prm.q)
        seeds = disjoint_seeds(700, len(VECTORS[scheme]))
        dcs = dev.r1cs(cs)
        full = device_keygen(dev, scheme, dcs, vk, seeds=seeds)
        got = device_keygen(dev, scheme, dcs, vk, seeds=seeds, seeded=True, pub_seeds=seeds, allow_shared_seeds=True)
        assert got["pub_seeds"] == seeds
        for v, vname in enumerate(VECTORS[scheme]):
            if full[vname] is None:
                assert got[vname] is None and label == "no_aux"
            elif vname in SINGLES[scheme]:
                assert (to_host(got[vname]) == to_host(full[vname])).all(), (label, vname)
            else:
                assert got[vname].shape == (full[vname].shape[0], prm.L, prm.K, prm.N_enc)
                assert (to_host(got[vname]) == to_host(c0_blocks(full[vname]))).all(), (label, vname)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_seeded_host_key_streaming_crosses_tile_boundaries(scheme):
    """22 rows: tiles of 1, of 8 (two full, one partial) and one tile of 64; the host vectors are half the size"""
    from ringsnark_amd.device import HostWords
    prm = P.preset("toy")
    dev = device_for("toy")
    cs = R.chain_r1cs(21, prm.q)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 14, H.oracle_ctx(prm).keygen(3)), prm.q)
    seeds = disjoint_seeds(100, len(VECTORS[scheme]))
    dcs = dev.r1cs(cs)
    full = device_keygen(dev, scheme, dcs, vk, seeds=seeds)
    for tile in (1, 8, 64):
        got = device_keygen(dev, scheme, dcs, vk, seeds=seeds, seeded=True, pub_seeds=seeds, allow_shared_seeds=True, host=True, tile=tile)
        for v, vname in enumerate(VECTORS[scheme]):
            assert isinstance(got[vname], HostWords) == (v < 3), vname
            if v < 3:
                assert got[vname].words * 2 == full[vname].numel()
                assert (words(dev, got[vname]) == words(dev, c0_blocks(full[vname]))).all(), (tile, vname)
            else:
                assert (words(dev, got[vname]) == words(dev, full[vname])).all(), (tile, vname)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_independent_public_seeds_encrypt_the_same_rows(scheme):
    """c0_seeded + a_pub s = c0_full + c1_full s (mod Q_j, NTT form, every element and prime): both are m - t e with the
    SAME e, the private stream's.  The seeded key decodes to the rows with the full key's noise budget."""
    from ringsnark_amd.device import to_host
    prm = P.preset("toy")
    dev = device_for("toy")
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(12, prm.q)
    dcs, vk, pk = seeded_case(dev, scheme, "toy", cs)
    n = len(VECTORS[scheme])
    assert pk["pub_seeds"] == disjoint_seeds(PUB, n)
    full = device_keygen(dev, scheme, dcs, vk, seeds=disjoint_seeds(700, n))
    wide = expanded(dev, scheme, pk)
    rows = key_rows(scheme, ctx, cs, dict(vk))
    s = vk["sk"].astype(object)  # [K][n]
    Q = np.array(prm.Q, dtype=object).reshape(1, 1, prm.K, 1)
    dsk = dev.put(vk["sk"])
    for v, vname in enumerate(VECTORS[scheme]):
        f = to_host(full[vname]).reshape((-1,) + ctx.enc_shape()).astype(object)
        w = to_host(wide[vname]).reshape((-1,) + ctx.enc_shape()).astype(object)
        if vname not in SINGLES[scheme]:
            assert (to_host(pk[vname]) == to_host(c0_blocks(wide[vname]))).all()
        assert (w[:, :, 1] != f[:, :, 1]).any(), vname  # another a ...
        assert ((w[:, :, 0] + w[:, :, 1] * s) % Q == (f[:, :, 0] + f[:, :, 1] * s) % Q).all(), vname  # ... the same m - t e
        count = f.shape[0]
        got = to_host(dev.enc_decode(dsk, wide[vname].reshape((count,) + ctx.enc_shape()))).reshape((count,) + ctx.ring_shape())
        assert (got == rows[vname]).all(), vname
        budget = dev.enc_noise_budget(dsk, wide[vname])
        assert budget.min() > 0 and (budget == dev.enc_noise_budget(dsk, full[vname])).all(), vname


@functools.lru_cache(maxsize=None)
def proof_case(name, scheme, m, zk):
    """per (preset, scheme): device, system, seeded device key with independent seeds, its expansion, assignment, and the
    proof from the expansion on the existing prover -- computed once"""
    prm = P.preset(name)
    dev = device_for(name)
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    dcs, vk, pk = seeded_case(dev, scheme, name, cs)
    asg = dev.put(H.make_assignment(ctx, cs))
    d = tuple(dev.put(x) for x in ctx.random_ring(77, 3)) if zk else (None, None, None)
    wide = expanded(dev, scheme, pk)
    exp, exp_empty, _ = prove(dev, scheme, dcs, wide, asg, d)
    return dict(prm=prm, dev=dev, cs=cs, dcs=dcs, vk=vk, pk=pk, wide=wide, asg=asg, d=d, exp=exp, exp_empty=exp_empty)


PROOF_CASES = [("toy", "groth16", False), ("toy", "rinocchio", True), ("toy49", "groth16", False), ("toy49", "rinocchio", False),
               ("toy50", "groth16", False), ("toy50", "rinocchio", False),
               ("toy60", "groth16", False), ("toy60", "rinocchio", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("name,scheme,zk", PROOF_CASES)
def test_proofs_from_a_seeded_key_equal_proofs_from_its_expansion(name, scheme, zk, host):
    """m = 21, 22 elements per vector: tiles of one element, two full tiles of 8 and a partial one, a single tile of 64."""
    from ringsnark_amd import _lib
    c = proof_case(name, scheme, 21, zk)
    dev, dcs = c["dev"], c["dcs"]
    pk = c["pk"]
    if host:
        _, _, pk = seeded_case(dev, scheme, name, c["cs"], host=True, tile=4)
        for vname in VECTORS[scheme][:3]:
            assert (words(dev, pk[vname]) == words(dev, c["pk"][vname])).all()
    for t in (1, 8, 64):
        with _lib.tuning(msm_host_tile=t):
            got, empty, _ = prove(dev, scheme, dcs, pk, c["asg"], c["d"])
        assert empty == c["exp_empty"] and (got == c["exp"]).all(), t


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("window", [8, 6])
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_windowed_seeded_key(scheme, zk, window, host):
    """Logical element t is stored element t % window and is regenerated with THAT index.  window = 6 with tiles of 4: the
    second tile is the stored elements 4, 5, 0, 1 -- it straddles the wrap."""
    from ringsnark_amd import _lib
    c = proof_case("toy", scheme, 21, zk)
    dev, dcs = c["dev"], c["dcs"]
    exp, exp_empty, _ = prove(dev, scheme, dcs, first_elements(dev, scheme, c["wide"], window), c["asg"], c["d"], window=window)
    assert (exp != c["exp"]).any()
    pk = c["pk"]
    if host:
        _, _, pk = seeded_case(dev, scheme, "toy", c["cs"], host=True)
    cut = first_elements(dev, scheme, pk, window)
    for t in (64, 4):
        with _lib.tuning(msm_host_tile=t):
            got, empty, _ = prove(dev, scheme, dcs, cut, c["asg"], c["d"], window=window)
        assert empty == exp_empty and (got == exp).all(), t


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_seeded_proofs_verify_and_take_wire_kinds(scheme, zk):
    from ringsnark_amd import _lib
    c = proof_case("toy", scheme, 21, zk)
    dev, dcs, cs = c["dev"], c["dcs"], c["cs"]
    got, empty, proof = prove(dev, scheme, dcs, c["pk"], c["asg"], c["d"])
    assert (got == c["exp"]).all()
    primary = c["asg"][: cs.n_inputs].contiguous()
    if scheme == "groth16":
        assert dev.groth16_verify(dev.groth16_vk(dcs, c["vk"]), primary, proof, empty).accepted
    else:
        assert dev.rinocchio_verify(dev.rinocchio_vk(dcs, c["vk"]), primary, proof, empty).accepted
    # an RS_KIND_ONE wire among the auxiliary ones: its key element passes through, from the regenerated tile too
    kinds = np.full(cs.n_vars, _lib.RS_KIND_POLY, dtype=np.uint8)
    kinds[cs.n_inputs + 2] = _lib.RS_KIND_ONE
    exp, exp_empty, _ = prove(dev, scheme, dcs, c["wide"], c["asg"], c["d"], kinds=kinds)
    assert (exp != c["exp"]).any()
    got, empty, _ = prove(dev, scheme, dcs, c["pk"], c["asg"], c["d"], kinds=kinds)
    assert empty == exp_empty and (got == exp).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_seeded_key_without_auxiliary_variables(scheme):
    prm = P.preset("toy")
    dev = device_for("toy")
    ctx = H.oracle_ctx(prm)
    label, cs = systems(prm.q)[-1]
    assert label == "no_aux" and cs.n_aux == 0
    dcs, vk, pk = seeded_case(dev, scheme, "toy", cs)
    assert pk[VECTORS[scheme][2]] is None
    asg = dev.put(ctx.random_ring(8, cs.n_vars))
    exp, exp_empty, _ = prove(dev, scheme, dcs, expanded(dev, scheme, pk), asg)
    got, empty, _ = prove(dev, scheme, dcs, pk, asg)
    assert empty == exp_empty and (got == exp).all()


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_wide_kernels_read_a_regenerated_tile(scheme, host):
    """C2 (N_enc = 8192, K = 4) at m = 3: the wide multiply-accumulate kernels on the staging buffer the expansion wrote"""
    prm = P.preset("C2")
    dev = device_for("C2")
    rng = np.random.RandomState(2)
    sk = residues(rng, prm.Q, prm.N_enc)
    cs = R.chain_r1cs(3, prm.q)
    dcs, vk, pk = seeded_case(dev, scheme, "C2", cs, host=host, sk=sk)
    asg = dev.put(np.stack([residues(rng, prm.q, prm.N) for _ in range(cs.n_vars)]))
    exp, exp_empty, _ = prove(dev, scheme, dcs, expanded(dev, scheme, pk), asg)
    got, empty, _ = prove(dev, scheme, dcs, pk, asg)
    assert empty == exp_empty and (got == exp).all()


@pytest.mark.gpu
def test_msm_over_compact_vectors():
    """rs_msm_seeded == rs_msm over the expansion: two key vectors, device and host, a window"""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    prm = P.preset("toy")
    dev = device_for("toy")
    rng = np.random.RandomState(6)
    T = 11
    c0 = [dev.put(np.stack([residues(rng, prm.Q, prm.N_enc) for _ in range(T * prm.L)]).reshape(T, prm.L, prm.K, prm.N_enc)) for _ in range(2)]
    pub = [5, 5 + STRIDE]
    wide = [dev.enc_expand_seeded(c, p) for c, p in zip(c0, pub)]
    vecs = [(dev.put(np.stack([residues(rng, prm.q, prm.N) for _ in range(T)])), None, g) for g in range(2)]
    exp, _ = dev.msm(wide, vecs, 2)
    hosted = []
    for c in c0:
        hw = dev.host_alloc(c.numel())
        hw.fill_from(c)
        hosted.append(hw)
    with _lib.tuning(msm_host_tile=4):
        for crs in (c0, hosted):
            got, _ = dev.msm(crs, vecs, 2, pub_seeds=pub)
            assert (to_host(got) == to_host(exp)).all()
        exp_w, _ = dev.msm([w[:4].contiguous() for w in wide], vecs, 2, crs_len=T, window=4)
        got, _ = dev.msm([c[:4].contiguous() for c in c0], vecs, 2, crs_len=T, window=4, pub_seeds=pub)
        assert (to_host(got) == to_host(exp_w)).all()


def raw_keygen_seeded(dev, scheme, dcs, vk, seed_words, pub_words):
    """The C entry point on output buffers filled with a pattern: (status, message, every output still holds the pattern)."""
    import torch
    from ringsnark_amd import _lib
    from ringsnark_amd.device import _ptr
    m, n_aux = dcs.m, dcs.n_vars - dcs.n_inputs
    lens = [m + 1, m + 1, n_aux] + [1] * (len(VECTORS[scheme]) - 3)
    outs = [torch.full((max(n, 1), dev.L, 2, dev.K, dev.N_enc), PATTERN, dtype=torch.int64, device=dev.device) for n in lens]
    t = {k: dev.put(v) for k, v in vk.items() if k != "Zt"}
    hs, hp = (C.c_uint64 * len(lens))(*seed_words), (C.c_uint64 * len(lens))(*pub_words)
    dev.sync()
    if scheme == "groth16":
        out = _lib.Groth16SeededKeyOut(*[o.data_ptr() for o in outs], 0, 0)
        st = dev.lib.rs_groth16_keygen_seeded(dev.h, dcs.h, _ptr(t["s"]), _ptr(t["alpha"]), _ptr(t["beta"]), _ptr(t["delta"]), _ptr(t["sk"]),
                                              hs, hp, C.byref(out), None)
    else:
        out = _lib.RinocchioSeededKeyOut(*[o.data_ptr() for o in outs], 0, 0)
        st = dev.lib.rs_rinocchio_keygen_seeded(dev.h, dcs.h, *[_ptr(t[k]) for k in ("s", "alpha", "beta", "r_v", "r_w", "r_y", "sk")], hs, hp,
                                                C.byref(out), None)
    return st, dev.lib.rs_last_error().decode(), all(bool((o == PATTERN).all()) for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_public_seed_ranges_must_be_disjoint(scheme):
    from ringsnark_amd import _lib
    prm = P.preset("toy")
    dev = device_for("toy")
    cs = R.chain_r1cs(6, prm.q)
    dcs = dev.r1cs(cs)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 15, H.oracle_ctx(prm).keygen(3)), prm.q)
    nv = len(VECTORS[scheme])
    hs = [(x * 65537) % 2**64 for x in disjoint_seeds(50, nv)]
    hp = [(x * 65537) % 2**64 for x in disjoint_seeds(PUB, nv)]
    st, _, untouched = raw_keygen_seeded(dev, scheme, dcs, vk, hs, hp)
    assert st == _lib.RS_OK and not untouched
    for v, w, off in ((1, 0, cs.m), (1, 0, 0), (nv - 1, 1, 3), (0, 3, -cs.m)):  # the cases of test_keygen.py, on the public words
        pub = list(hp)
        pub[v] = (hp[w] + off) % 2**64
        st, msg, untouched = raw_keygen_seeded(dev, scheme, dcs, vk, hs, pub)
        assert st == _lib.RS_ERR_INVALID and "public seed ranges" in msg and untouched, (v, w, off, st, msg)
    pub = list(hp)
    pub[1], pub[3] = 2**64 - 2, 1  # a public range that wraps around 2^64 into another
    st, msg, untouched = raw_keygen_seeded(dev, scheme, dcs, vk, hs, pub)
    assert st == _lib.RS_ERR_INVALID and "public seed ranges" in msg and untouched
    pub = list(hp)
    pub[1] = (hp[0] + cs.m + 1) % 2**64  # one stream past the end of s_pows is fine
    assert raw_keygen_seeded(dev, scheme, dcs, vk, hs, pub)[0] == _lib.RS_OK
    # private ranges are still checked
    st, msg, untouched = raw_keygen_seeded(dev, scheme, dcs, vk, [hs[0]] + hs[:-1], hp)
    assert st == _lib.RS_ERR_INVALID and "intersect" in msg and untouched
    # the wrapper refuses a public stream that is a private one, unless told that this is a test
    seeds = disjoint_seeds(50, nv)
    for pub_seeds in (seeds, [seeds[1]] + disjoint_seeds(PUB, nv)[1:]):
        with pytest.raises(ValueError):
            device_keygen(dev, scheme, dcs, vk, seeds=seeds, seeded=True, pub_seeds=pub_seeds)
    device_keygen(dev, scheme, dcs, vk, seeds=seeds, seeded=True, pub_seeds=seeds, allow_shared_seeds=True)
    # no public seeds given: drawn from the operating system, different every time, never a private one
    a, b = (device_keygen(dev, scheme, dcs, vk, seeds=seeds, seeded=True)["pub_seeds"] for _ in range(2))
    assert len(a) == nv and a != b and not set(a) & set(seeds)
