"""Shared cases of tests/test_modswitch.py (CPU) and tests/test_modswitch_gpu.py: per preset a secret key, two kinds of
valid encodings -- fresh ones and ciphertext x ring products -- their mirror-switched versions at every level, and what
the CPU oracle's context on the truncated prime list Q[:K_out] says about those (budget, decoding).  Built once per process
and never modified."""
import numpy as np

from oracle import oracle as O
from ringsnark_amd import modswitch as MS
from ringsnark_amd import params as P
from tests import helpers as H

PRESETS = ("toy", "toyR", "toy49", "toy50", "toy54", "toy60")
KINDS = ("fresh", "product")
COUNT = 2  # encoding elements per (preset, kind)

_NTT, _CASES = {}, {}


def oracle_ntt(prm):
    """the transform provider the mirror takes, on the CPU oracle's NTT"""
    logn = prm.N_enc.bit_length() - 1

    def ntt(p):
        if (logn, p) not in _NTT:
            _NTT[(logn, p)] = O.NTT(logn, p)
        return _NTT[(logn, p)]
    return ntt


def truncated(prm, K_lvl):
    return P.RingParams(prm.N, list(prm.q), prm.N_enc, list(prm.Q[:K_lvl]), name="%s[:%d]" % (prm.name, K_lvl))


def secret_norm(prm, sk):
    """the infinity norm of the secret polynomial (centred coefficients of row 0 of sk)"""
    Q0 = int(prm.Q[0])
    s = [int(v) for v in oracle_ntt(prm)(Q0).inv(sk[0])]
    return max(min(v, Q0 - v) for v in s)


class Case:
    """prm, ctx, sk [K][N_enc]; per kind: ring [COUNT][L][N] (what the encodings hold), enc [COUNT][L][2][K][N_enc];
    switched[kind][K_out]: the mirror's output; budget[kind][K_out] [COUNT][L] and decoded[kind][K_out] [COUNT][L][N]: the
    oracle context on Q[:K_out] with sk[:K_out] (decoded without any factor; None entries where the budget is spent)."""

    def __init__(self, name):
        self.prm = prm = P.preset(name)
        self.ctx = ctx = H.oracle_ctx(prm)
        self.sk = sk = ctx.keygen(11)
        base = ctx.random_ring(21, COUNT)
        other = ctx.random_ring(22, COUNT)
        fresh = ctx.enc_encode(sk, base, 5)
        self.ring = {"fresh": base, "product": ctx.ring_mul(base, other)}
        self.enc = {"fresh": fresh, "product": np.stack([ctx.enc_mul_ring(fresh[k], other[k]) for k in range(COUNT)])}
        ntt = oracle_ntt(prm)
        self.switched, self.budget, self.decoded = {}, {}, {}
        for kind in KINDS:
            self.switched[kind], self.budget[kind], self.decoded[kind] = {}, {}, {}
            for K_out in range(prm.K, 0, -1):
                # one step from the level above: the sequence the mirror defines
                sw = self.enc[kind] if K_out == prm.K else MS.mod_switch(prm, self.switched[kind][K_out + 1], K_out + 1, K_out, ntt)
                self.switched[kind][K_out] = sw
                tp = truncated(prm, K_out)
                tctx = H.oracle_ctx(tp)
                tsk = np.ascontiguousarray(sk[:K_out])
                self.budget[kind][K_out] = np.array([tctx.noise_budget(tsk, sw[k]) for k in range(COUNT)])
                self.decoded[kind][K_out] = [tctx.enc_decode(tsk, sw[k]) if min(self.budget[kind][K_out][k]) > 0 else None
                                             for k in range(COUNT)]


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]
