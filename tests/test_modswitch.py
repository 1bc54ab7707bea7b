"""Mod-switched encodings on the CPU (include/ringsnark_amd/modswitch.h): the library exports the new header, the Python
mirror (ringsnark_amd/modswitch.py) agrees with the CPU oracle's contexts on the truncated prime lists, its outputs obey the
noise bound of the switch, and the level wire format is the existing format of a truncated context.  Every comparison is
integer equality."""
import os
import re
import struct

import numpy as np
import pytest

from oracle import oracle as O
from ringsnark_amd import modswitch as MS
from ringsnark_amd import params as P
from tests import helpers as H
from tests import modswitch_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_function_of_modswitch_h():
    from ringsnark_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ringsnark_amd", "modswitch.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)  # the comments name functions of other headers
    declared = set(re.findall(r"\b(rs_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 8, declared
    assert declared == set(_lib.MODSWITCH_SIGNATURES), declared ^ set(_lib.MODSWITCH_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rs_version() >= 108


def test_plain_transform_is_the_oracles():
    """The mirror's default transforms (the definition, term by term) against the CPU oracle's NTT: same order, same scaling."""
    prm = P.preset("toy")
    logn = prm.N_enc.bit_length() - 1
    rng = np.random.RandomState(3)
    for p in (prm.Q[0], prm.Q[2]):
        a = (rng.randint(0, 2**62, size=prm.N_enc, dtype=np.int64).astype(np.uint64) % np.uint64(p)).astype(np.uint64)
        mine, ref = MS.PlainNTT(logn, p), O.NTT(logn, p)
        assert (mine.fwd(a) == ref.fwd(a)).all()
        assert (mine.inv(a) == ref.inv(a)).all()
        assert (ref.inv(ref.fwd(a)) == a).all()
    enc = MC.case("toy").enc["fresh"][:1]
    assert (MS.mod_switch(prm, enc, 3, 1) == MS.mod_switch(prm, enc, 3, 1, MC.oracle_ntt(prm))).all()


@pytest.mark.parametrize("name", MC.PRESETS)
def test_mirror_against_the_truncated_context_oracle(name):
    """A switched ciphertext is an ordinary ciphertext of the context on Q[:K_out]: wherever that context's budget is > 0, its
    decoding times level_factor is the ring element the unswitched encoding holds.  Every (preset, kind) decodes at K - 1;
    toy and toyR decode at every level."""
    c = MC.case(name)
    prm = c.prm
    for kind in MC.KINDS:
        for K_out in range(1, prm.K + 1):
            assert c.switched[kind][K_out].shape == (MC.COUNT, prm.L, 2, K_out, prm.N_enc)
            for j in range(K_out):
                assert int(c.switched[kind][K_out][:, :, :, j].max()) < prm.Q[j]
            for k in range(MC.COUNT):
                dec = c.decoded[kind][K_out][k]
                must = K_out >= prm.K - 1 or name in ("toy", "toyR")
                assert dec is not None or not must, (name, kind, K_out, c.budget[kind][K_out][k])
                if dec is not None:
                    assert (MS.apply_level_factor(prm, dec, K_out) == c.ring[kind][k]).all(), (name, kind, K_out, k)
        assert MS.level_factor(prm, prm.K) == [1] * prm.L


def test_a_spent_level_occurs_and_the_oracle_says_so():
    """Not every level is decodable: the oracle's budget of some switched encoding is 0 (the single-prime level of the presets
    whose primes are as large as their plaintext moduli)."""
    spent = [(name, kind, K_out) for name in MC.PRESETS for kind in MC.KINDS for K_out in range(1, MC.case(name).prm.K)
             if (MC.case(name).budget[kind][K_out] == 0).any()]
    assert spent, "no spent level among the cases"
    assert all(K_out == 1 and name not in ("toy", "toyR") for name, _, K_out in spent), spent


@pytest.mark.parametrize("name", MC.PRESETS)
def test_noise_bound_of_one_step(name):
    """|v'| < |v| / p + t (1 + N_enc |s|_inf) for every step k -> k - 1 of the mirror's outputs.  The oracle's budgets give
    the bit lengths: budget = bit_count(Q) - bits(|v|) - 1 > 0, so 2^(bits' - 1) <= |v'| and |v| < 2^bits."""
    c = MC.case(name)
    prm = c.prm
    s_inf = MC.secret_norm(prm, c.sk)
    assert s_inf == 1  # ternary secret
    checked = 0
    for kind in MC.KINDS:
        for k in range(prm.K, 1, -1):
            tb_in, tb_out = H.noise_tb(prm.Q[:k]), H.noise_tb(prm.Q[:k - 1])
            p = int(prm.Q[k - 1])
            for e in range(MC.COUNT):
                for i, t in enumerate(prm.q):
                    b_in, b_out = int(c.budget[kind][k][e][i]), int(c.budget[kind][k - 1][e][i])
                    if b_in == 0 or b_out == 0:
                        continue  # the bit length of a spent ciphertext's noise is not known from its budget
                    bits_in, bits_out = tb_in - b_in - 1, tb_out - b_out - 1
                    assert (1 << (bits_out - 1)) * p < (1 << bits_in) + int(t) * (1 + prm.N_enc * s_inf) * p, (name, kind, k, e, i)
                    checked += 1
    assert checked >= 2 * MC.COUNT * prm.L  # at least the step K -> K - 1 of both kinds


def test_level_file_is_the_file_of_the_truncated_context():
    """serialize_level(K_out) of the mirror: the documented layout of ringsnark_amd.h, written out here field by field for
    the context on Q[:K_out] -- header, flags, padding, payload with an EMPTY element's words zeroed."""
    c = MC.case("toy")
    prm = c.prm
    for K_out in range(1, prm.K + 1):
        enc = c.switched["fresh"][K_out]
        tp = MC.truncated(prm, K_out)
        for empty in (None, [0, 1]):
            want = b"RSNKENC1" + struct.pack("<IIII", tp.N, tp.L, tp.N_enc, tp.K)
            for v in tp.q + tp.Q:
                want += struct.pack("<Q", v)
            want += struct.pack("<Q", MC.COUNT) + bytes(empty or [0, 0])
            while len(want) % 8:
                want += b"\0"
            for k in range(MC.COUNT):
                words = np.zeros_like(enc[k]) if empty and empty[k] else enc[k]
                want += words.astype("<u8").tobytes()
            got = MS.serialize_level(prm, enc, K_out, empty)
            assert got == want
            assert len(got) == (8 + 16 + 8 * (tp.L + K_out) + 8 + MC.COUNT + 7) // 8 * 8 + MC.COUNT * tp.enc_words * 8
    # the wire saving is exact: payload x K_out / K
    header = lambda K_lvl: (8 + 16 + 8 * (prm.L + K_lvl) + 8 + MC.COUNT + 7) // 8 * 8
    full = len(MS.serialize_level(prm, c.enc["fresh"], prm.K)) - header(prm.K)
    assert (len(MS.serialize_level(prm, c.switched["fresh"][1], 1)) - header(1)) * prm.K == full
