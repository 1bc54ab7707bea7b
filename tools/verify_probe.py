"""Timing of the verifier (DESIGN.md "Verifier"): rs_io_eval_at, rs_groth16_vk_create and rs_groth16_verify on the ring of a
preset (default C3: N = 8192, L = 4, N_enc = 8192, K = 4) with the chain circuit at m = 2^12 and 2^16.

Per m:
  io_eval_at      one rs_io_eval_at call (host clock around the call; it synchronises) and the device time of its three
                  kernels from the library's own per-launch events (rs_set_profiling), in a pass of its own
  vk_create       rs_groth16_vk_create (uploads excluded; includes rs_io_eval_at, the unit test of gamma, the copies)
  verify          rs_groth16_verify (the batch verifier's body and kernel on a batch of one) on a "proof" of three FRESH
                  encodings of random ring elements (rejected, but the same work as an accepted one; uniformly random words
                  would trip the noise guard), beside rs_enc_decode of the same three elements alone
  instance_map    rs_instance_map_eval, only where its [m][L][N] intermediates fit (m <= --imap-max-log): the same-run
                  comparison for io_eval_at, with the outputs compared bit for bit
Warm-up, then medians of --repeats calls; rs_measure_peaks of the same run is recorded as the clock-dependent denominators.

usage: python tools/verify_probe.py [--out profiles/verify_probe.txt] [--preset C3] [--logm 12,16] [--repeats 7]
"""
import argparse
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
from ringsnark_amd.device import Device  # noqa: E402


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


def timed(dev, f, repeats, warm=2):
    for _ in range(warm):
        f()
    t = []
    for _ in range(repeats):
        dev.sync()
        t0 = time.perf_counter()
        f()
        dev.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "verify_probe.txt"))
    ap.add_argument("--preset", default="C3")
    ap.add_argument("--logm", default="12,16")
    ap.add_argument("--imap-max-log", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    prm = P.preset(args.preset)
    dev = Device(prm)
    rng = np.random.RandomState(3)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    emit({"preset": args.preset, "N": prm.N, "L": prm.L, "N_enc": prm.N_enc, "K": prm.K, "device": torch.cuda.get_device_name(0),
          "repeats": args.repeats, "source_hash": _lib.source_hash(), "peaks_before": dev.measure_peaks()})
    dsk = secret_key(dev, rng)
    proof = dev.enc_encode(dsk, dev.put(random_ring(prm, rng, 3)), 7)
    el = {k: dev.put(random_ring(prm, rng, 1, lo=1)[0]) for k in ("alpha", "beta", "gamma", "delta")}
    el["sk"] = dsk
    for logm in [int(x) for x in args.logm.split(",")]:
        m = 1 << logm
        cs = R.chain_r1cs(m, prm.q)
        dcs = dev.r1cs(cs)
        primary = dev.put(random_ring(prm, rng, cs.n_inputs))
        s = dev.put(random_ring(prm, rng, 1, lo=m)[0])
        rec = {"m": m, "n_inputs": cs.n_inputs, "workspace_ring_elements": 2 * ((m + 63) // 64)}
        rec["io_eval_at"] = timed(dev, lambda: dev.io_eval_at(dcs, s), args.repeats)
        dev.set_profiling(True)
        dev.profile_read()
        for _ in range(args.repeats):
            dev.io_eval_at(dcs, s)
        rec["io_eval_at_kernels_ms"] = {k["name"]: k["total_ms"] / k["launches"] for k in dev.profile_read() if k["name"].startswith("io_")}
        dev.set_profiling(False)
        vk = dict(el, s=s)
        rec["groth16_vk_create"] = timed(dev, lambda: dev.groth16_vk(dcs, vk).close(), args.repeats)  # close: a memset and a free on top
        dvk = dev.groth16_vk(dcs, vk)
        res = dev.groth16_verify(dvk, primary, proof)
        assert not res.accepted and res.n_bad[0] > 0  # three unrelated encodings: rejected, an answer
        rec["groth16_verify"] = timed(dev, lambda: dev.groth16_verify(dvk, primary, proof), args.repeats)
        rec["enc_decode_3"] = timed(dev, lambda: dev.enc_decode(dsk, proof), args.repeats)
        dvk.close()
        if logm <= args.imap_max_log:
            rec["instance_map_eval"] = timed(dev, lambda: dev.instance_map_eval(dcs, s), max(3, args.repeats // 2), warm=1)
            full, io = dev.instance_map_eval(dcs, s), dev.io_eval_at(dcs, s)
            n1 = cs.n_inputs + 1
            rec["bit_identical_to_instance_map_eval"] = bool(all(torch.equal(io[k], full[k][:n1]) for k in range(3)) and torch.equal(io[3], full[4]))
            del full, io
            torch.cuda.empty_cache()
        emit(rec)
        del dcs
    emit({"peaks_after": dev.measure_peaks()})


if __name__ == "__main__":
    main()
