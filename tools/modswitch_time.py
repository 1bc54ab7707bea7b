"""Mod-switched proofs (ringsnark_amd/modswitch.h) on one MI355X: what a switch costs, what it saves the verifier and the wire,
and which level a real proof tolerates.

  switch    rs_enc_mod_switch at the C3 shape (N_enc = 8192, L = 4, K = 4) on 3 and on 9 fresh encodings, K 4 -> 3 and 4 -> 2:
            device events around 20 back-to-back calls, per call
  verify    rs_groth16_verify_level at K_lvl = 2 beside rs_groth16_verify on the same proof (chain circuit, m = 2^12, as
            tools/verify_probe.py: three fresh encodings, rejected -- the same work as an accepted proof), and the decodes
            alone; host clock around calls that synchronise
  wire      rs_enc_wire_size_level of 3 and 9 elements per level (exact: the payload is K_lvl / K of the full one)
  budget    a real C2 ringGroth16 proof (N = 4096, L = 2, N_enc = 8192, K = 4; chain circuit, m = 2^10, key generated on the
            device from a random trapdoor): the noise budget of each proof element and limb at K_lvl = 4, 3, 2, 1
Warm-up, then the median of 7 (min and max beside it).

usage: python tools/modswitch_time.py [--out profiles/modswitch.txt]
"""
import argparse
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
from ringsnark_amd.device import Device  # noqa: E402

REPEATS, WARM, CALLS = 7, 2, 20


def random_ring(prm, rng, count, lo=0):
    out = np.empty((count, prm.L, prm.N), dtype=np.uint64)
    for i, q in enumerate(prm.q):
        out[:, i, :] = (rng.randint(0, 2**62, size=(count, prm.N), dtype=np.int64).astype(np.uint64) % np.uint64(q - lo)) + np.uint64(lo)
    return out


def secret_key(dev, rng):
    """a ternary secret in NTT form [K][N_enc], as rs_enc_encode / rs_enc_decode take it"""
    tern = rng.randint(-1, 2, size=dev.N_enc)
    sk = np.stack([np.where(tern < 0, int(Q) - 1, tern).astype(np.uint64) for Q in dev.prm.Q])
    d = dev.put(sk)
    for j in range(dev.K):
        dev.ntt(d[j], _lib.RS_MOD_COEFF, j)
    dev.sync()
    return d


def spread(t):
    return "%.4f ms (min %.4f, max %.4f)" % (statistics.median(t), min(t), max(t))


def device_time(f, calls=CALLS):
    """per-call device time of an asynchronous call: events around `calls` of them"""
    t = []
    for k in range(WARM + REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            f()
        e1.record()
        e1.synchronize()
        if k >= WARM:
            t.append(e0.elapsed_time(e1) / calls)
    return t


def host_time(dev, f):
    """host clock around a call that synchronises"""
    t = []
    for k in range(WARM + REPEATS):
        dev.sync()
        t0 = time.perf_counter()
        f()
        dev.sync()
        if k >= WARM:
            t.append((time.perf_counter() - t0) * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "modswitch.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        lines.append(s)
        print(s, flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    rng = np.random.RandomState(3)
    prm = P.preset("C3")
    dev = Device(prm)
    K = prm.K
    say("# tools/modswitch_time.py on %s; library sources %s; warm-up %d, median of %d" % (torch.cuda.get_device_name(0), _lib.source_hash(), WARM, REPEATS))
    say("# C3: N = %d, L = %d, N_enc = %d, K = %d; peaks of this run: %s" % (prm.N, prm.L, prm.N_enc, prm.K, dev.measure_peaks()))
    dsk = secret_key(dev, rng)
    fresh = dev.enc_encode(dsk, dev.put(random_ring(prm, rng, 9)), 7)

    say()
    say("## rs_enc_mod_switch, device time per call (%d calls between two events)" % CALLS)
    for n_el in (3, 9):
        src = fresh[:n_el].contiguous()
        for K_out in (3, 2):
            out = torch.empty((n_el, prm.L, 2, K_out, prm.N_enc), dtype=torch.int64, device=dev.device)
            call = lambda: _lib.check(dev.lib.rs_enc_mod_switch(dev.h, src.data_ptr(), n_el, K, K_out, out.data_ptr(), dev.stream()))
            say("%d elements, K %d -> %d: %s" % (n_el, K, K_out, spread(device_time(call))))

    say()
    say("## the verifier: chain circuit, m = 2^12, n_inputs = 2; host clock around calls that synchronise")
    m = 1 << 12
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    vk = {k: dev.put(random_ring(prm, rng, 1, lo=1)[0]) for k in ("alpha", "beta", "gamma", "delta")}
    vk.update(sk=dsk, s=dev.put(random_ring(prm, rng, 1, lo=m)[0]))
    dvk = dev.groth16_vk(dcs, vk)
    primary = dev.put(random_ring(prm, rng, cs.n_inputs))
    proof = fresh[:3].contiguous()
    ref = dev.groth16_verify(dvk, primary, proof)
    say("rs_groth16_verify, unswitched proof:      %s   (parent commit, DESIGN.md 'Verifier': 0.277 ms)" % spread(host_time(dev, lambda: dev.groth16_verify(dvk, primary, proof))))
    say("rs_enc_decode x3 alone:                   %s" % spread(host_time(dev, lambda: dev.enc_decode(dsk, proof))))
    for K_lvl in (3, 2):
        sw = dev.enc_mod_switch(proof, K_lvl)
        assert (dev.enc_noise_budget(dsk, sw, level=K_lvl) > 0).all()
        assert dev.groth16_verify(dvk, primary, sw, level=K_lvl) == ref  # rejected, the same report
        say("rs_groth16_verify_level, K_lvl = %d:       %s" % (K_lvl, spread(host_time(dev, lambda: dev.groth16_verify(dvk, primary, sw, level=K_lvl)))))
        say("rs_enc_decode_level x3 alone, K_lvl = %d:  %s" % (K_lvl, spread(host_time(dev, lambda: dev.enc_decode(dsk, sw, level=K_lvl)))))
    dvk.close()

    say()
    say("## wire bytes (exact)")
    for n_el in (3, 9):
        say("%d elements: %s" % (n_el, ", ".join("K_lvl = %d: %d" % (k, dev.lib.rs_enc_wire_size_level(dev.h, k, n_el)) for k in range(K, 0, -1))))
    del dev, fresh, proof, dcs
    torch.cuda.empty_cache()

    say()
    prm = P.preset("C2")
    dev = Device(prm)
    m = 1 << 10
    say("## noise budget (bits) of a real ringGroth16 proof on C2 (N = %d, L = %d, N_enc = %d, K = %d), chain circuit, m = 2^10, device-generated key"
        % (prm.N, prm.L, prm.N_enc, prm.K))
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    dsk = secret_key(dev, rng)
    vk = {k: dev.put(random_ring(prm, rng, 1, lo=1)[0]) for k in ("alpha", "beta", "gamma", "delta")}
    vk.update(sk=dsk, s=dev.put(random_ring(prm, rng, 1, lo=m)[0]))
    pk = dev.groth16_keygen(dcs, vk, seeds=11)
    asg = dev.ring_empty(m + 2)
    dev.fill_uniform(asg[:2], 0, 5)
    dev.chain_assignment(asg, m)
    proof, empty = dev.groth16_prove(dcs, pk, asg, check=True)
    dvk = dev.groth16_vk(dcs, vk)
    assert empty == [0, 0, 0] and dev.groth16_verify(dvk, asg[:2].contiguous(), proof).accepted
    say("K_lvl | A (per limb) | B | C | rs_groth16_verify_level")
    for K_lvl in range(prm.K, 0, -1):
        sw = dev.enc_mod_switch(proof, K_lvl)
        b = dev.enc_noise_budget(dsk, sw, level=K_lvl)
        try:
            verdict = "accepted" if dev.groth16_verify(dvk, asg[:2].contiguous(), sw, level=K_lvl).accepted else "REJECTED"
        except _lib.RsError as e:
            verdict = "refused: %s" % str(e).split(": ", 1)[-1]
        say("%d | %s | %s | %s | %s" % (K_lvl, b[0].tolist(), b[1].tolist(), b[2].tolist(), verdict))
    dvk.close()


if __name__ == "__main__":
    main()
