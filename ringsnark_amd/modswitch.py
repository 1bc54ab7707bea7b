"""Host mirror of include/ringsnark_amd/modswitch.h in Python integers: what rs_enc_mod_switch must write, word for word,
the level factor a level decode multiplies by, and the level wire format.

One step K_in -> K_in - 1 (SEAL 4.x BGV mod_t_and_divide_q_last_ntt_inplace, recalled, not vendored) per (element, limb i,
component c), t = q_i, p = Q[K_in - 1]:
    last = iNTT_p(row K_in - 1)                                   in [0, p)
    u    = (-last * p^-1) mod t                                   in [0, t)
    c'_j = (c_j - NTT_{Q_j}((last + u p) mod Q_j)) * p^-1 mod Q_j   for j < K_in - 1
K_in -> K_out is the sequence of such steps.

The transforms are an argument: `ntt(p)` returns an object with .fwd(row) / .inv(row) on uint64 rows of N_enc words (negacyclic,
SEAL's bit-reversed order, the inverse scaled).  Tests pass the CPU oracle's (oracle.NTT); the default is the definition
itself, evaluated term by term (PlainNTT: quadratic, for small N_enc), so the mirror never runs the code it checks.
"""
import struct

import numpy as np

MAGIC = b"RSNKENC1"


def _bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


class PlainNTT:
    """Negacyclic transform of length n mod p straight from its definition: fwd(a)[k] = a(psi^(2 bitrev(k) + 1)), psi the
    minimal primitive 2n-th root of unity mod p (SEAL's choice); inv is its inverse."""

    def __init__(self, logn, p):
        self.logn, self.n, self.p = logn, 1 << logn, int(p)
        n, p = self.n, self.p
        assert (p - 1) % (2 * n) == 0
        g = next(pow(x, (p - 1) // (2 * n), p) for x in range(2, p) if pow(x, (p - 1) // 2, p) == p - 1)
        assert pow(g, n, p) == p - 1
        self.psi = min(pow(g, k, p) for k in range(1, 2 * n, 2))
        self.points = [pow(self.psi, 2 * _bitrev(k, logn) + 1, p) for k in range(n)]

    def fwd(self, a):
        p, a = self.p, [int(v) for v in a]
        out = []
        for z in self.points:
            acc = 0
            for v in reversed(a):  # Horner
                acc = (acc * z + v) % p
            out.append(acc)
        return np.array(out, dtype=np.uint64)

    def inv(self, a):
        # a_x = n^-1 sum_k A_k z_k^-x  (the points z_k are the n roots of X^n + 1)
        p, n, A = self.p, self.n, [int(v) for v in a]
        ninv = pow(n, -1, p)
        zinv = [pow(z, -1, p) for z in self.points]
        out, cur = [], [1] * n
        for _ in range(n):
            out.append(sum(v * c for v, c in zip(A, cur)) % p * ninv % p)
            cur = [c * z % p for c, z in zip(cur, zinv)]
        return np.array(out, dtype=np.uint64)


def plain_ntt(prm):
    """The default transform provider of a parameter set: PlainNTT per prime, built once."""
    logn, cache = prm.N_enc.bit_length() - 1, {}

    def ntt(p):
        if p not in cache:
            cache[p] = PlainNTT(logn, p)
        return cache[p]
    return ntt


def _step(prm, flat, K_in, ntt):
    """flat [count][L][2][K_in][N_enc] -> [count][L][2][K_in - 1][N_enc]"""
    p = int(prm.Q[K_in - 1])
    out = np.empty(flat.shape[:3] + (K_in - 1, prm.N_enc), dtype=np.uint64)
    for e in range(flat.shape[0]):
        for i, t in enumerate(prm.q):
            t = int(t)
            pinv_t = pow(p, -1, t)
            for c in range(2):
                last = [int(v) for v in ntt(p).inv(flat[e, i, c, K_in - 1])]
                assert all(0 <= v < p for v in last)
                u = [(-v * pinv_t) % t for v in last]
                for j in range(K_in - 1):
                    Qj = int(prm.Q[j])
                    w = np.array([(v + x * p) % Qj for v, x in zip(last, u)], dtype=np.uint64)
                    delta = ntt(Qj).fwd(w)
                    pinv = pow(p, -1, Qj)
                    out[e, i, c, j] = np.array([(int(a) - int(d)) * pinv % Qj for a, d in zip(flat[e, i, c, j], delta)], dtype=np.uint64)
    return out


def mod_switch(prm, enc, K_in, K_out, ntt=None):
    """enc [..][L][2][K_in][N_enc] (uint64, canonical residues of Q[:K_in]) -> [..][L][2][K_out][N_enc]."""
    assert 1 <= K_out <= K_in <= prm.K, (K_out, K_in, prm.K)
    enc = np.ascontiguousarray(enc, dtype=np.uint64)
    assert enc.shape[-4:] == (prm.L, 2, K_in, prm.N_enc), enc.shape
    lead = enc.shape[:-4]
    flat = enc.reshape((-1,) + enc.shape[-4:]).copy()
    ntt = ntt or plain_ntt(prm)
    for k in range(K_in, K_out, -1):
        flat = _step(prm, flat, k, ntt)
    return flat.reshape(lead + (prm.L, 2, K_out, prm.N_enc))


def level_factor(prm, K_lvl):
    """F_i = prod_{j >= K_lvl} Q_j mod q_i per limb: a ciphertext switched to K_lvl primes decrypts to m / F_i."""
    assert 1 <= K_lvl <= prm.K
    out = []
    for t in prm.q:
        f = 1
        for Q in prm.Q[K_lvl:]:
            f = f * int(Q) % int(t)
        out.append(f)
    return out


def apply_level_factor(prm, ring, K_lvl):
    """ring [..][L][N] decoded by the context of Q[:K_lvl] -> the ring element the unswitched encoding holds"""
    ring = np.asarray(ring, dtype=np.uint64)
    out = np.empty_like(ring)
    for i, f in enumerate(level_factor(prm, K_lvl)):
        out[..., i, :] = (ring[..., i, :].astype(object) * f % int(prm.q[i])).astype(np.uint64)
    return out


def serialize_level(prm, enc, K_lvl, empty=None):
    """The bytes rs_enc_serialize_level writes for enc [count][L][2][K_lvl][N_enc]: magic, u32 N, L, N_enc, K_lvl, u64 q[L],
    Q[:K_lvl], u64 count, u8 empty[count], zero padding to a multiple of 8, the payload (an EMPTY element's all zero)."""
    assert 1 <= K_lvl <= prm.K
    enc = np.ascontiguousarray(enc, dtype="<u8").reshape((-1, prm.L, 2, K_lvl, prm.N_enc)).copy()
    count = enc.shape[0]
    flags = [0] * count if empty is None else [1 if e else 0 for e in empty]
    assert len(flags) == count
    head = MAGIC + struct.pack("<4I", prm.N, prm.L, prm.N_enc, K_lvl)
    head += struct.pack("<%dQ" % (prm.L + K_lvl), *[int(x) for x in list(prm.q) + list(prm.Q[:K_lvl])])
    head += struct.pack("<Q", count) + bytes(flags)
    head += b"\0" * (-len(head) % 8)
    for k, f in enumerate(flags):
        if f:
            enc[k] = 0
    return head + enc.tobytes()
