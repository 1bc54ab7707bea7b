"""ringsnark_amd/packed.h: bit-packed seeded proving keys -- the c0 rows of a seeded vector as bit streams of
w = max_j bitlen(Q_j) bits a residue, unpacked (and c1 regenerated) on the device where the key is read.

Everything is exact, so every comparison is equality of uint64 words.  The format's reference is ringsnark_amd/packed.py,
itself checked here against a Python big-integer bit stream; the reference of everything that reads or writes a packed key is
the seeded path (tests/test_seeded.py), which has parity of its own.  Shapes, seeds and systems are those of
tests/test_seeded.py."""
import ctypes as C
import functools
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from ringsnark_amd import packed as PK
from ringsnark_amd import params as P
from ringsnark_amd import r1cs as R
from tests import helpers as H
from tests.test_keygen import STRIDE, VECTORS, device_for, device_keygen, disjoint_seeds, key_words, systems, trapdoor, with_r_y
from tests.test_seeded import PATTERN, PUB, SINGLES, prove, residues, seeded_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ringsnark_amd", "packed.h")
PRESETS = [("toy", 5, 41), ("toy49", 5, 49), ("toy50", 5, 50), ("toy60", 5, 60), ("C2", 3, 44), ("C5s", 2, 49)]


# ---- CPU -------------------------------------------------------------------------------------------------------------
def naive_words(row, w, n_words):
    """the row's bit stream as one Python integer, cut into 64-bit words"""
    big = 0
    for p, v in enumerate(row):
        big |= int(v) << (p * w)
    assert big >> (64 * n_words) == 0
    return [(big >> (64 * k)) & (2**64 - 1) for k in range(n_words)]


@pytest.mark.parametrize("n", [2, 64, 128, 130])
def test_packed_py_is_the_naive_bit_stream(n):
    """every width; rows with a partial last word and a pad word (n w not a multiple of 128) and without; the round trip;
    zero padding bits"""
    rnd = random.Random(n)
    for w in range(2, 63):
        top = 2**w - 1
        rows = np.array([[0] * n, [top] * n, [top * (p & 1) for p in range(n)], [top * (1 - (p & 1)) for p in range(n)],
                         [rnd.getrandbits(w) for _ in range(n)], [rnd.getrandbits(w) for _ in range(n)]], dtype=np.uint64)
        n_words = 2 * ((n * w + 127) // 128)
        assert PK.words_per_row(n, w) == n_words
        got = PK.pack_rows(rows, w)
        assert got.dtype == np.uint64 and got.shape == (len(rows), n_words)
        for r, row in enumerate(rows):
            assert [int(x) for x in got[r]] == naive_words(row, w, n_words), (w, r)
            stream = sum(int(x) << (64 * k) for k, x in enumerate(got[r]))
            assert stream >> (n * w) == 0, (w, r)  # padding bits
        assert (PK.unpack_rows(got, w, n) == rows).all(), w
        # leading dimensions pass through, and only the low w bits of a residue are stored
        assert (PK.pack_rows(rows.reshape(2, 3, n), w) == got.reshape(2, 3, n_words)).all()
        assert (PK.pack_rows(rows | np.uint64(1 << w), w) == got).all()


def test_pack_bits_of_the_presets():
    for name, _, w in PRESETS:
        prm = P.preset(name)
        assert PK.pack_bits(prm) == w == max(int(Q).bit_length() for Q in prm.Q), name
        assert PK.row_words(prm) == 2 * ((prm.N_enc * w + 127) // 128) and PK.row_words(prm) % 2 == 0
    assert PK.row_words(P.preset("toy")) * 64 > P.preset("toy").N_enc * 41  # toy: a partial last word and a pad word
    assert PK.pack_bits(P.preset("C3")) == 44


def test_library_exports_every_function_of_packed_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", code))
    assert names == set(_lib.PACKED_SIGNATURES) and len(names) == 12
    for n in names:
        assert hasattr(lib, n), n
    assert lib.rs_version() >= 111
    assert '#include "seeded.h"' in code


@pytest.mark.parametrize("lang,std", [("c", "c99"), ("c++", "c++17")])
def test_packed_h_compiles_on_its_own(tmp_path, lang, std):
    cc = shutil.which("gcc" if lang == "c" else "g++")
    if cc is None:
        pytest.skip("no compiler")
    src = tmp_path / ("only." + ("c" if lang == "c" else "cpp"))
    src.write_text("#include <ringsnark_amd/packed.h>\nint main(void) { return 0; }\n")
    r = subprocess.run([cc, "-x", lang, "-std=" + std, "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_packed_needs_seeded():
    """refused before the device is touched: the wrapper's first statement"""
    from ringsnark_amd.device import Device
    for fn in (Device.groth16_keygen, Device.rinocchio_keygen):
        with pytest.raises(ValueError, match="seeded"):
            fn(None, None, None, packed=True)
    with pytest.raises(ValueError, match="pub_seeds"):
        Device.msm(None, [], [], 1, packed=True)


# ---- GPU helpers -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_case(name, count):
    """per preset: device, compact elements [count][L][K][n] -- random canonical residues, and a row of zeros, a row of
    Q_j - 1 and two alternating rows among them -- on the host and on the device, and their packed form by packed.py"""
    prm = P.preset(name)
    dev = device_for(name)
    rng = np.random.RandomState(5)
    c0 = np.stack([residues(rng, prm.Q, prm.N_enc) for _ in range(count * prm.L)]).reshape(count * prm.L * prm.K, prm.N_enc)
    n_rows = c0.shape[0]
    assert n_rows >= 5
    alt = (np.arange(prm.N_enc) & 1).astype(np.uint64)
    for r, pattern in ((0, 0 * alt), (n_rows - 1, 1 + 0 * alt), (2, alt), (n_rows - 2, 1 - alt)):
        c0[r] = pattern * np.uint64(prm.Q[r % prm.K] - 1)
    c0 = c0.reshape(count, prm.L, prm.K, prm.N_enc)
    w = PK.pack_bits(prm)
    return dict(prm=prm, dev=dev, w=w, c0=c0, d_c0=dev.put(c0), packed=PK.pack_rows(c0, w))


def packed_of(dev, v):
    """the packed form of a compact key vector (device tensor or HostWords), by the device's pack kernel, as words"""
    from ringsnark_amd.device import HostWords, to_host
    if v is None:
        return np.zeros(0, dtype=np.uint64)
    if isinstance(v, HostWords):
        v = dev.put(np.array(v.array).reshape(-1, dev.L, dev.K, dev.N_enc))
    got, bad = dev.enc_pack_c0(v)
    assert bad == 0
    return to_host(got).reshape(-1)


def packed_case(dev, scheme, name, cs, host=False, tile=0, seeds=700, pub=PUB, sk=None):
    """seeded_case of tests/test_seeded.py with packed=True: the same trapdoor and seeds"""
    prm = P.preset(name)
    sk = H.oracle_ctx(prm).keygen(3) if sk is None else sk
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 11, sk), prm.q)
    dcs = dev.r1cs(cs)
    n = len(VECTORS[scheme])
    pk = device_keygen(dev, scheme, dcs, vk, seeds=disjoint_seeds(seeds, n), seeded=True, packed=True, pub_seeds=disjoint_seeds(pub, n), host=host,
                       tile=tile)
    assert pk["packed"] is True and pk["pub_seeds"] == disjoint_seeds(pub, n)
    return dcs, vk, pk


def first_packed(dev, scheme, pk, count):
    """the packed key with its three vectors cut to `count` elements (a windowed key)"""
    from ringsnark_amd.device import HostWords
    out = dict(pk)
    for name in VECTORS[scheme][:3]:
        v = pk[name]
        if isinstance(v, HostWords):
            out[name] = dev.host_alloc(count * dev.packed_words)
            out[name].array[:] = v.array[: count * dev.packed_words]
        else:
            out[name] = v[:count].contiguous()
    return out


@functools.lru_cache(maxsize=None)
def proof_case(name, scheme, m, zk):
    """per (preset, scheme): system, SEEDED device key, assignment and the proof from it on the seeded prover -- the
    expected value of every packed proof -- and the packed device key of the same seeds; computed once"""
    prm = P.preset(name)
    dev = device_for(name)
    ctx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    dcs, vk, seeded = seeded_case(dev, scheme, name, cs)
    asg = dev.put(H.make_assignment(ctx, cs))
    d = tuple(dev.put(x) for x in ctx.random_ring(77, 3)) if zk else (None, None, None)
    exp, exp_empty, _ = prove(dev, scheme, dcs, seeded, asg, d)
    _, _, pk = packed_case(dev, scheme, name, cs)
    return dict(prm=prm, dev=dev, cs=cs, dcs=dcs, vk=vk, seeded=seeded, pk=pk, asg=asg, d=d, exp=exp, exp_empty=exp_empty)


# ---- GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,count,w", PRESETS)
def test_pack_and_unpack(name, count, w):
    """toy: 64 * 41 bits, a partial last word and a zero pad word; C2: four parts per row; C5s: N_enc = 16384, K = 8"""
    from ringsnark_amd.device import to_host
    c = rows_case(name, count)
    dev, prm = c["dev"], c["prm"]
    assert dev.pack_bits == w == c["w"] and dev.packed_words == prm.L * prm.K * PK.row_words(prm)
    got, bad = dev.enc_pack_c0(c["d_c0"])
    assert bad == 0 and got.shape == (count, prm.L, prm.K, PK.row_words(prm))
    assert (to_host(got) == c["packed"]).all()
    assert (to_host(dev.enc_unpack_c0(got)) == c["c0"]).all()
    assert (to_host(dev.enc_unpack_c0(dev.put(c["packed"]))) == c["c0"]).all()
    one, bad = dev.enc_pack_c0(c["d_c0"][1].contiguous(), want_bad=False)  # one element, no count asked for
    assert bad is None and one.shape == got.shape[1:] and (to_host(one) == c["packed"][1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,count", [("toy", 5), ("C2", 3)])
def test_words_beyond_the_width_are_counted_and_their_low_bits_stored(name, count):
    """bad input is an answer: first and last residue of a row, one that straddles a word boundary, one that ends on one"""
    from ringsnark_amd.device import to_host
    c = rows_case(name, count)
    dev, prm, w = c["dev"], c["prm"], c["w"]
    n = prm.N_enc
    straddle = next(p for p in range(1, n) if (p * w) % 64 + w > 64)
    ends = next(p for p in range(1, n) if ((p + 1) * w) % 64 == 0)
    c0 = c["c0"].copy()
    spots = [(0, 0, 0, 0), (1, 0, 1, n - 1), (2, prm.L - 1, prm.K - 1, straddle), (count - 1, prm.L - 1, 0, ends), (count - 1, 0, 0, n - 1)]
    for k, spot in enumerate(spots):
        c0[spot] |= np.uint64(1) << np.uint64(w + (k % (64 - w)))
        assert int(c0[spot]) >= 2**w
    got, bad = dev.enc_pack_c0(dev.put(c0))
    assert bad == len(spots)
    assert (to_host(got) == c["packed"]).all()  # the low w bits of the bad words, every neighbour untouched
    assert (to_host(dev.enc_unpack_c0(got)) == c["c0"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,count,w", PRESETS)
def test_expansion_of_packed_elements_equals_the_seeded_expansion(name, count, w):
    from ringsnark_amd.device import to_host
    c = rows_case(name, count)
    dev = c["dev"]
    packed = dev.put(c["packed"])
    exp = to_host(dev.enc_expand_seeded(c["d_c0"], 9))
    assert (to_host(dev.enc_expand_packed(packed, 9)) == exp).all()
    first = 3 if count > 3 else count - 1
    exp = to_host(dev.enc_expand_seeded(c["d_c0"][first:].contiguous(), 9, first=first))
    assert (to_host(dev.enc_expand_packed(packed[first:].contiguous(), 9, first=first)) == exp).all()
    assert (to_host(dev.enc_expand_packed(packed[first:].contiguous(), 9)) != exp).any()  # the stream index is the stored index


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
@pytest.mark.parametrize("name", ["toy", "toy49", "toy60"])
def test_packed_keygen_is_pack_of_the_seeded_key(name, scheme):
    """m = 12: vectors of 13 and 12 or 13 elements.  Device-resident in one tile and in tiles of 5 (two full, one partial);
    host-resident in tiles of 3 (13 = 4 * 3 + 1)."""
    from ringsnark_amd.device import HostWords, to_host
    prm = P.preset(name)
    dev = device_for(name)
    cs = R.chain_r1cs(12, prm.q)
    assert (cs.m + 1) % 3 != 0 and (cs.m + 1) % 5 != 0
    dcs, vk, seeded = seeded_case(dev, scheme, name, cs)
    exp = {v: packed_of(dev, seeded[v]) for v in VECTORS[scheme][:3]}
    assert (exp["s_pows"] == PK.pack_rows(to_host(seeded["s_pows"]), PK.pack_bits(prm)).reshape(-1)).all()
    for host, tile in ((False, 0), (False, 5), (True, 3)):
        _, _, pk = packed_case(dev, scheme, name, cs, host=host, tile=tile)
        for v, vname in enumerate(VECTORS[scheme]):
            assert isinstance(pk[vname], HostWords) == (host and v < 3), vname
            if v < 3:
                got = key_words(dev, pk[vname])
                assert got.shape == exp[vname].shape == ((cs.m + 1 if v < 2 else cs.n_aux) * dev.packed_words,), (vname, got.shape)
                assert (got == exp[vname]).all(), (host, tile, vname)
            else:
                assert (key_words(dev, pk[vname]) == key_words(dev, seeded[vname])).all(), (host, tile, vname)
    if scheme == "rinocchio":  # into=: the buffers of a key are written again
        _, _, pk = packed_case(dev, scheme, name, cs)
        buffers = {v: pk[v].data_ptr() for v in VECTORS[scheme]}
        pk["s_pows"].zero_()
        n = len(VECTORS[scheme])
        again = dev.rinocchio_keygen(dcs, vk, seeds=disjoint_seeds(700, n), seeded=True, packed=True, pub_seeds=disjoint_seeds(PUB, n), into=pk)
        assert again is pk and {v: pk[v].data_ptr() for v in VECTORS[scheme]} == buffers
        assert (key_words(dev, pk["s_pows"]) == exp["s_pows"]).all()


PROOF_CASES = [(name, scheme, zk) for name in ("toy", "toy49", "toy60") for scheme, zk in (("groth16", False), ("rinocchio", False), ("rinocchio", True))]


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("name,scheme,zk", PROOF_CASES)
def test_proofs_from_a_packed_key_equal_proofs_from_the_seeded_key(name, scheme, zk, host):
    """m = 21, 22 elements per vector: two full tiles of 8 and a partial one, a single tile of 64"""
    from ringsnark_amd import _lib
    c = proof_case(name, scheme, 21, zk)
    dev, dcs = c["dev"], c["dcs"]
    pk = c["pk"]
    if host:
        _, _, pk = packed_case(dev, scheme, name, c["cs"], host=True, tile=4)
        for vname in VECTORS[scheme][:3]:
            assert (key_words(dev, pk[vname]) == key_words(dev, c["pk"][vname])).all()
    for t in (8, 64):
        with _lib.tuning(msm_host_tile=t):
            got, empty, _ = prove(dev, scheme, dcs, pk, c["asg"], c["d"])
        assert empty == c["exp_empty"] and (got == c["exp"]).all(), t


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("window", [8, 6])
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_windowed_packed_key(scheme, zk, window, host):
    """window = 6 with tiles of 4: the second tile is the stored elements 4, 5, 0, 1 -- split at the wrap in stored elements"""
    from ringsnark_amd import _lib
    from tests.test_seeded import first_elements
    c = proof_case("toy", scheme, 21, zk)
    dev, dcs = c["dev"], c["dcs"]
    exp, exp_empty, _ = prove(dev, scheme, dcs, first_elements(dev, scheme, c["seeded"], window), c["asg"], c["d"], window=window)
    assert (exp != c["exp"]).any()
    pk = c["pk"]
    if host:
        _, _, pk = packed_case(dev, scheme, "toy", c["cs"], host=True)
    cut = first_packed(dev, scheme, pk, window)
    for t in (64, 4):
        with _lib.tuning(msm_host_tile=t):
            got, empty, _ = prove(dev, scheme, dcs, cut, c["asg"], c["d"], window=window)
        assert empty == exp_empty and (got == exp).all(), t


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_packed_proofs_verify(scheme, zk):
    c = proof_case("toy", scheme, 21, zk)
    dev, dcs, cs = c["dev"], c["dcs"], c["cs"]
    got, empty, proof = prove(dev, scheme, dcs, c["pk"], c["asg"], c["d"])
    assert (got == c["exp"]).all()
    primary = c["asg"][: cs.n_inputs].contiguous()
    if scheme == "groth16":
        assert dev.groth16_verify(dev.groth16_vk(dcs, c["vk"]), primary, proof, empty).accepted
    else:
        assert dev.rinocchio_verify(dev.rinocchio_vk(dcs, c["vk"]), primary, proof, empty).accepted


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_packed_key_without_auxiliary_variables(scheme):
    prm = P.preset("toy")
    dev = device_for("toy")
    ctx = H.oracle_ctx(prm)
    label, cs = systems(prm.q)[-1]
    assert label == "no_aux" and cs.n_aux == 0
    dcs, vk, seeded = seeded_case(dev, scheme, "toy", cs)
    _, _, pk = packed_case(dev, scheme, "toy", cs)
    assert pk[VECTORS[scheme][2]] is None
    asg = dev.put(ctx.random_ring(8, cs.n_vars))
    exp, exp_empty, _ = prove(dev, scheme, dcs, seeded, asg)
    got, empty, _ = prove(dev, scheme, dcs, pk, asg)
    assert empty == exp_empty and (got == exp).all()


@pytest.mark.gpu
@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("scheme,zk", [("groth16", False), ("rinocchio", True)])
def test_a_batch_of_three_from_a_packed_key(scheme, zk, host):
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    c = proof_case("toy", scheme, 21, zk)
    dev, dcs = c["dev"], c["dcs"]
    ctx = H.oracle_ctx(c["prm"])
    asgs = [c["asg"]] + [dev.put(H.make_assignment(ctx, c["cs"], seed=s)) for s in (31, 32)]
    pk = c["pk"]
    if host:
        _, _, pk = packed_case(dev, scheme, "toy", c["cs"], host=True)
    with _lib.tuning(msm_host_tile=8):
        if scheme == "groth16":
            exp, exp_empty = dev.groth16_prove_batch(dcs, c["seeded"], asgs)
            got, empty = dev.groth16_prove_batch(dcs, pk, asgs)
        else:
            d = dev.put(ctx.random_ring(78, 9).reshape((3, 3) + ctx.ring_shape()))
            exp, exp_empty = dev.rinocchio_prove_batch(dcs, c["seeded"], asgs, d)
            got, empty = dev.rinocchio_prove_batch(dcs, pk, asgs, d)
    assert empty == exp_empty and (to_host(got) == to_host(exp)).all()
    if scheme == "groth16":
        assert (to_host(got)[0] == c["exp"]).all()  # member 0 is the single proof


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,host", [("groth16", False), ("rinocchio", True)])
def test_wide_kernels_read_an_unpacked_tile(scheme, host):
    """C2 (N_enc = 8192, K = 4) at m = 3: the wide multiply-accumulate kernels on the staging buffer the expansion wrote"""
    prm = P.preset("C2")
    dev = device_for("C2")
    rng = np.random.RandomState(2)
    sk = residues(rng, prm.Q, prm.N_enc)
    cs = R.chain_r1cs(3, prm.q)
    dcs, vk, seeded = seeded_case(dev, scheme, "C2", cs, sk=sk)
    _, _, pk = packed_case(dev, scheme, "C2", cs, host=host, sk=sk)
    for vname in VECTORS[scheme][:3]:
        assert (key_words(dev, pk[vname]) == packed_of(dev, seeded[vname])).all(), vname
    asg = dev.put(np.stack([residues(rng, prm.q, prm.N) for _ in range(cs.n_vars)]))
    exp, exp_empty, _ = prove(dev, scheme, dcs, seeded, asg)
    got, empty, _ = prove(dev, scheme, dcs, pk, asg)
    assert empty == exp_empty and (got == exp).all()


@pytest.mark.gpu
def test_msm_over_packed_vectors():
    """rs_msm_packed == rs_msm_seeded over the same elements: one and two key vectors, device and host, a window"""
    from ringsnark_amd import _lib
    from ringsnark_amd.device import to_host
    prm = P.preset("toy")
    dev = device_for("toy")
    rng = np.random.RandomState(6)
    T = 11
    c0 = [dev.put(np.stack([residues(rng, prm.Q, prm.N_enc) for _ in range(T * prm.L)]).reshape(T, prm.L, prm.K, prm.N_enc)) for _ in range(2)]
    pub = [5, 5 + STRIDE]
    packed = [dev.enc_pack_c0(c)[0] for c in c0]
    vecs = [(dev.put(np.stack([residues(rng, prm.q, prm.N) for _ in range(T)])), None, g) for g in range(2)]
    hosted = []
    for p in packed:
        hw = dev.host_alloc(p.numel())
        hw.fill_from(p)
        hosted.append(hw)
    with _lib.tuning(msm_host_tile=4):
        for n_crs in (1, 2):
            exp, _ = dev.msm(c0[:n_crs], vecs, 2, pub_seeds=pub[:n_crs])
            for crs in (packed, hosted):
                got, _ = dev.msm(crs[:n_crs], vecs, 2, pub_seeds=pub[:n_crs], packed=True)
                assert (to_host(got) == to_host(exp)).all(), n_crs
        exp_w, _ = dev.msm([c[:4].contiguous() for c in c0], vecs, 2, crs_len=T, window=4, pub_seeds=pub)
        got, _ = dev.msm([p[:4].contiguous() for p in packed], vecs, 2, crs_len=T, window=4, pub_seeds=pub, packed=True)
        assert (to_host(got) == to_host(exp_w)).all()


def raw_keygen_packed(dev, scheme, dcs, vk, seed_words, pub_words, offset=0):
    """The C entry point on output buffers filled with a pattern, the three vectors `offset` bytes into theirs:
    (status, message, every output still holds the pattern)."""
    import torch
    from ringsnark_amd import _lib
    from ringsnark_amd.device import _ptr
    m, n_aux = dcs.m, dcs.n_vars - dcs.n_inputs
    lens = [m + 1, m + 1, n_aux] + [1] * (len(VECTORS[scheme]) - 3)
    outs = [torch.full((max(n, 1) + 1, dev.L, 2, dev.K, dev.N_enc), PATTERN, dtype=torch.int64, device=dev.device) for n in lens]
    t = {k: dev.put(v) for k, v in vk.items() if k != "Zt"}
    hs, hp = (C.c_uint64 * len(lens))(*seed_words), (C.c_uint64 * len(lens))(*pub_words)
    ptrs = [o.data_ptr() + (offset if v < 3 else 0) for v, o in enumerate(outs)]
    dev.sync()
    if scheme == "groth16":
        out = _lib.Groth16SeededKeyOut(*ptrs, 0, 0)
        st = dev.lib.rs_groth16_keygen_packed(dev.h, dcs.h, _ptr(t["s"]), _ptr(t["alpha"]), _ptr(t["beta"]), _ptr(t["delta"]), _ptr(t["sk"]),
                                              hs, hp, C.byref(out), None)
    else:
        out = _lib.RinocchioSeededKeyOut(*ptrs, 0, 0)
        st = dev.lib.rs_rinocchio_keygen_packed(dev.h, dcs.h, *[_ptr(t[k]) for k in ("s", "alpha", "beta", "r_v", "r_w", "r_y", "sk")], hs, hp,
                                                C.byref(out), None)
    dev.sync()
    return st, dev.lib.rs_last_error().decode(), all(bool((o == PATTERN).all()) for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["groth16", "rinocchio"])
def test_packed_keygen_refuses_before_it_writes(scheme):
    from ringsnark_amd import _lib
    prm = P.preset("toy")
    dev = device_for("toy")
    cs = R.chain_r1cs(6, prm.q)
    dcs = dev.r1cs(cs)
    vk = with_r_y(scheme, trapdoor(scheme, prm, cs.m, 15, H.oracle_ctx(prm).keygen(3)), prm.q)
    nv = len(VECTORS[scheme])
    hs = [(x * 65537) % 2**64 for x in disjoint_seeds(50, nv)]
    hp = [(x * 65537) % 2**64 for x in disjoint_seeds(PUB, nv)]
    st, _, untouched = raw_keygen_packed(dev, scheme, dcs, vk, hs, hp)
    assert st == _lib.RS_OK and not untouched
    st, msg, untouched = raw_keygen_packed(dev, scheme, dcs, vk, hs, hp, offset=8)  # 8-byte aligned only
    assert st == _lib.RS_ERR_INVALID and "16-byte aligned" in msg and untouched, (st, msg)
    pub = list(hp)
    pub[1] = (hp[0] + cs.m) % 2**64  # the last stream of s_pows is the first of the second vector
    st, msg, untouched = raw_keygen_packed(dev, scheme, dcs, vk, hs, pub)
    assert st == _lib.RS_ERR_INVALID and "public seed ranges" in msg and untouched, (st, msg)
    st, msg, untouched = raw_keygen_packed(dev, scheme, dcs, vk, [hs[0]] + hs[:-1], hp)  # private ranges
    assert st == _lib.RS_ERR_INVALID and "intersect" in msg and untouched, (st, msg)
    with pytest.raises(ValueError, match="seeded"):
        device_keygen(dev, scheme, dcs, vk, packed=True)


@pytest.mark.gpu
def test_unaligned_and_null_pointers_are_refused_before_anything_is_written():
    import torch
    from ringsnark_amd import _lib
    from ringsnark_amd.device import _ptr
    c = rows_case("toy", 5)
    dev = c["dev"]
    packed = dev.put(c["packed"])

    def refused(status):
        dev.sync()
        assert status == _lib.RS_ERR_INVALID, (status, dev.lib.rs_last_error().decode())
        return dev.lib.rs_last_error().decode()

    out = torch.full((6,) + tuple(packed.shape[1:]), PATTERN, dtype=torch.int64, device=dev.device)
    bad = C.c_size_t(7)
    assert "16-byte aligned" in refused(dev.lib.rs_enc_pack_c0(dev.h, _ptr(c["d_c0"]), 5, out.data_ptr() + 8, C.byref(bad), None))
    assert "16-byte aligned" in refused(dev.lib.rs_enc_pack_c0(dev.h, c["d_c0"].data_ptr() + 8, 4, out.data_ptr(), C.byref(bad), None))
    assert "null" in refused(dev.lib.rs_enc_pack_c0(dev.h, None, 5, out.data_ptr(), None, None))
    assert bool((out == PATTERN).all()) and bad.value == 7
    wide = torch.full((6, dev.L, 2, dev.K, dev.N_enc), PATTERN, dtype=torch.int64, device=dev.device)
    assert "16-byte aligned" in refused(dev.lib.rs_enc_unpack_c0(dev.h, packed.data_ptr() + 8, 4, wide.data_ptr(), None))
    assert "16-byte aligned" in refused(dev.lib.rs_enc_expand_packed(dev.h, packed.data_ptr() + 8, 9, 0, 4, wide.data_ptr(), None))
    assert "16-byte aligned" in refused(dev.lib.rs_enc_expand_packed(dev.h, _ptr(packed), 9, 0, 5, wide.data_ptr() + 8, None))
    assert "null" in refused(dev.lib.rs_enc_expand_packed(dev.h, _ptr(packed), 9, 0, 5, None, None))
    assert bool((wide == PATTERN).all())
    # a prover and an inner product on a key vector that is 8-byte aligned only: refused before the proof is touched
    for scheme, n_out in (("groth16", 3), ("rinocchio", 9)):
        p = proof_case("toy", scheme, 21, scheme == "rinocchio")
        key = dict(p["pk"])
        name = VECTORS[scheme][1]
        shifted = torch.empty(key[name].numel() + 1, dtype=torch.int64, device=dev.device)
        shifted[1:] = key[name].reshape(-1)
        key[name] = shifted[1:]
        assert key[name].data_ptr() % 16 == 8
        proof = torch.full((n_out, dev.L, 2, dev.K, dev.N_enc), PATTERN, dtype=torch.int64, device=dev.device)
        pdev, dcs = p["dev"], p["dcs"]
        if scheme == "groth16":
            s, _ = pdev._groth16_key(key, 0)
            st = pdev.lib.rs_groth16_prove_packed(pdev.h, dcs.h, C.byref(s), _ptr(p["asg"]), None, _ptr(proof), None, None)
        else:
            s, _ = pdev._rinocchio_key(key, 0)
            st = pdev.lib.rs_rinocchio_prove_packed(pdev.h, dcs.h, C.byref(s), _ptr(p["asg"]), None, *[_ptr(x) for x in p["d"]], _ptr(proof),
                                                    None, None)
        pdev.sync()
        assert st == _lib.RS_ERR_INVALID and "16-byte aligned" in pdev.lib.rs_last_error().decode(), st
        assert bool((proof == PATTERN).all())
