"""Timing of the generator (DESIGN.md section 3 "Generator"): rs_groth16_keygen against the composed path of the entry
points that existed before it, and its encode kernel against rs_enc_encode, on the ring of a preset (default C2: N = 4096,
L = 2, N_enc = 8192, K = 4) with the chain circuit at m = 1024, device-resident key.

  keygen      one rs_groth16_keygen call
  composed    the same key from rs_instance_map_eval, rs_ring_inv / rs_ring_mul / rs_ring_add on device-resident rows (a
              coefficient element is expanded to the rows it multiplies by a device copy: rs_ring_mul takes two vectors
              of one length) and one rs_enc_encode per vector; no host copies; output buffers allocated once, outside
  encode_linear / enc_encode
              rs_enc_encode_linear (one term, no coefficient: the generator's kernel alone) and rs_enc_encode on the same
              m + 1 rows (the powers of s)
Host clock around calls that synchronise; two warm-up calls, then --repeats calls of each, the two sides of a pair
ALTERNATING in one process; median, minimum and maximum are reported (the spread), and the outputs of the two sides of
each pair are compared word for word first.

usage: python tools/keygen_time.py [--out profiles/keygen_time.txt] [--preset C2] [--m 1024] [--repeats 9]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ringsnark_amd import _lib  # noqa: E402
from ringsnark_amd import params as P  # noqa: E402
from ringsnark_amd import r1cs as R  # noqa: E402
from ringsnark_amd.device import Device, _ptr  # noqa: E402


def random_ring(prm, rng, lo=1):
    return np.stack([(rng.randint(0, 2**62, size=prm.N, dtype=np.int64).astype(np.uint64) % np.uint64(q - lo)) + np.uint64(lo) for q in prm.q])


def secret_key(dev, rng):
    """a ternary secret in NTT form [K][N_enc], as rs_enc_encode takes it"""
    tern = rng.randint(-1, 2, size=dev.N_enc)
    sk = np.stack([np.where(tern < 0, int(Q) - 1, tern).astype(np.uint64) for Q in dev.prm.Q])
    d = dev.put(sk)
    for j in range(dev.K):
        dev.ntt(d[j], _lib.RS_MOD_COEFF, j)
    dev.sync()
    return d


def alternate(dev, fa, fb, repeats, warm=2):
    """times of fa and fb in ms, taken alternately"""
    for _ in range(warm):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(repeats):
        for f, t in ((fa, ta), (fb, tb)):
            dev.sync()
            t0 = time.perf_counter()
            f()
            dev.sync()
            t.append((time.perf_counter() - t0) * 1e3)
    stat = lambda t: {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
    return stat(ta), stat(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "keygen_time.txt"))
    ap.add_argument("--preset", default="C2")
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    prm = P.preset(args.preset)
    dev = Device(prm)
    lib, h = dev.lib, dev.h
    rng = np.random.RandomState(5)
    m = args.m
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    n1, n_aux, k0 = cs.n_vars + 1, cs.n_aux, cs.n_inputs + 1
    s, alpha, beta, delta = dev.put(random_ring(prm, rng, m)), dev.put(random_ring(prm, rng)), dev.put(random_ring(prm, rng)), dev.put(random_ring(prm, rng))
    sk = secret_key(dev, rng)
    seeds = [(x * 65537) % 2**64 for x in (7 + v * (1 << 40) for v in range(5))]
    hs = (C.c_uint64 * 5)(*seeds)
    st = dev.stream()
    lens = [m + 1, m + 1, n_aux, 1, 1]

    # ---- the generator
    new = [dev.enc_empty(n) for n in lens]
    out = _lib.Groth16KeyOut(*[t.data_ptr() for t in new], 0, 0)

    def keygen():
        _lib.check(lib.rs_groth16_keygen(h, dcs.h, _ptr(s), _ptr(alpha), _ptr(beta), _ptr(delta), _ptr(sk), hs, C.byref(out), st))

    # ---- the composed path, every buffer allocated here
    old = [dev.enc_empty(n) for n in lens]
    At, Bt, Ct, Ht, Zt = dev.ring_empty(n1), dev.ring_empty(n1), dev.ring_empty(n1), dev.ring_empty(m + 1), dev.ring_empty()
    dinv, zd = dev.ring_empty(), dev.ring_empty()
    rep = dev.ring_empty(m + 1)  # a coefficient element expanded to the rows it multiplies
    ts, t1, t2 = dev.ring_empty(m + 1), dev.ring_empty(n_aux), dev.ring_empty(n_aux)

    def mul(dst, a, b, n):
        _lib.check(lib.rs_ring_mul(h, _ptr(dst), _ptr(a), _ptr(b), n, st))

    def add(dst, a, b, n):
        _lib.check(lib.rs_ring_add(h, _ptr(dst), _ptr(a), _ptr(b), n, st))

    def encode(rows, n, seed, dst):
        _lib.check(lib.rs_enc_encode(h, _ptr(sk), _ptr(rows), n, C.c_uint64(seed), _ptr(dst), st))

    def composed():
        _lib.check(lib.rs_instance_map_eval(h, dcs.h, _ptr(s), _ptr(At), _ptr(Bt), _ptr(Ct), _ptr(Ht), _ptr(Zt), st))
        _lib.check(lib.rs_ring_inv(h, _ptr(dinv), _ptr(delta), 1, st))
        mul(zd, Zt, dinv, 1)
        rep.copy_(zd.unsqueeze(0).expand_as(rep))
        mul(ts, Ht, rep, m + 1)  # delta_ts rows
        a_mid, b_mid, c_mid = At[k0:], Bt[k0:], Ct[k0:]
        rep[:n_aux].copy_(beta.unsqueeze(0).expand(n_aux, dev.L, dev.N))
        mul(t1, a_mid, rep, n_aux)
        rep[:n_aux].copy_(alpha.unsqueeze(0).expand(n_aux, dev.L, dev.N))
        mul(t2, b_mid, rep, n_aux)
        add(t1, t1, t2, n_aux)
        add(t1, t1, c_mid, n_aux)
        rep[:n_aux].copy_(dinv.unsqueeze(0).expand(n_aux, dev.L, dev.N))
        mul(t1, t1, rep, n_aux)  # delta_mid rows
        encode(Ht, m + 1, seeds[0], old[0])
        encode(ts, m + 1, seeds[1], old[1])
        encode(t1, n_aux, seeds[2], old[2])
        encode(alpha, 1, seeds[3], old[3])
        encode(beta, 1, seeds[4], old[4])

    keygen()
    composed()
    dev.sync()
    same_key = all(bool((a == b).all()) for a, b in zip(new, old))

    # ---- the kernel alone, on the powers of s (left in Ht by composed())
    lin, enc = dev.enc_empty(m + 1), dev.enc_empty(m + 1)
    rows_p = (C.c_void_p * 1)(Ht.data_ptr())

    def encode_linear():
        _lib.check(lib.rs_enc_encode_linear(h, _ptr(sk), None, rows_p, 1, m + 1, C.c_uint64(seeds[0]), _ptr(lin), st))

    def enc_encode():
        encode(Ht, m + 1, seeds[0], enc)

    encode_linear()
    enc_encode()
    dev.sync()
    same_rows = bool((lin == enc).all())

    kg, co = alternate(dev, keygen, composed, args.repeats)
    el, ee = alternate(dev, encode_linear, enc_encode, args.repeats)
    rec = {"preset": prm.name, "m": m, "N": prm.N, "L": prm.L, "N_enc": prm.N_enc, "K": prm.K, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(dev.device), "source_hash": _lib.source_hash(),
           "outputs_identical": {"key": same_key, "rows": same_rows},
           "rs_groth16_keygen": kg, "composed": co, "rs_enc_encode_linear": el, "rs_enc_encode": ee}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not (same_key and same_rows):
        sys.exit("outputs differ")


if __name__ == "__main__":
    main()
