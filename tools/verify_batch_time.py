"""Batched verification (ringsnark_amd/verify_batch.h) on one MI355X: B single calls beside one batch call of B, on the same
key and the same proofs.  Both run one verifier body and one kernel pair (verify.hip: a single call is a batch of one), so the
first column is what a call costs and the ratio what sharing a call, a decode and the key's columns saves.

  ringGroth16   C3 (N = N_enc = 8192, L = K = 4), chain circuit m = 64, n_inputs = 2: the decode dominates
  Rinocchio     C5 (N = 2048, L = 1, N_enc = 16384, K = 8), the logistic-regression circuit (256 features, 517 public
                inputs): 3 * 518 public columns per verification

Per shape one ACCEPTED proof is made without a prover: its ring elements are solved from the verifier's equations for a
random primary input (the public sums from rs_io_eval_at) and freshly encoded; the single verifier must accept it.  The
batch holds B copies of it in B separate buffers (the work does not depend on the values).  B in {1, 8, 64}; host clock
around calls that synchronise; single and batch alternate inside every repetition; warm-up, then the median of 7 (min
and max beside it); per-proof time = call time / B.  Then, with the library's profiler on, the kernels of one batch call.

usage: python tools/verify_batch_time.py [--out profiles/verify_batch.txt] [--resource-usage FILE]
  --resource-usage: a text file with the compiler's -Rpass-analysis=kernel-resource-usage lines of verify_batch_kernel
  (cd ringsnark_amd/csrc && hipcc <FLAGS of the Makefile> -Rpass-analysis=kernel-resource-usage -c verify.hip -o /dev/null),
  copied into the output
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

REPEATS, WARM = 7, 2
BATCHES = (1, 8, 64)


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


def ring_sum(dev, rows):
    """the sum of the ring elements rows [n][L][N], by halving"""
    while rows.shape[0] > 1:
        h = rows.shape[0] // 2
        rest = rows[2 * h:]
        rows = torch.cat([dev.ring_add(rows[:h].contiguous(), rows[h:2 * h].contiguous()), rest])
    return rows[0].contiguous()


def public_sums(dev, dcs, s, primary):
    """v_io(s), w_io(s), y_io(s) = column 0 + sum_k x_k column k, and Z(s)"""
    A, B, Cc, Zt = dev.io_eval_at(dcs, s)
    out = []
    for cols in (A, B, Cc):
        acc = cols[0].contiguous()
        if dcs.n_inputs:
            acc = dev.ring_add(acc, ring_sum(dev, dev.ring_mul(primary, cols[1:].contiguous())))
        out.append(acc)
    return out, Zt


def accepted_proof(dev, scheme, dcs, vk, primary, rng):
    """encodings of ring elements that satisfy every equation of the scheme's verifier for `primary`"""
    prm = dev.prm
    (v, w, y), Zt = public_sums(dev, dcs, vk["s"], primary)
    r = dev.put(random_ring(prm, rng, 3))
    mul, add, sub = dev.ring_mul, dev.ring_add, dev.ring_sub
    if scheme == "groth16":
        f = add(add(mul(vk["beta"], v), mul(vk["alpha"], w)), y)
        Cc = mul(sub(sub(mul(r[0], r[1]), mul(vk["alpha"], vk["beta"])), f), dev.ring_inv(vk["delta"]))
        els = [r[0], r[1], Cc]
    else:
        V, W, Y = r[0], r[1], r[2]
        Hh = mul(sub(mul(add(V, v), add(W, w)), add(Y, y)), dev.ring_inv(Zt))
        Lb = mul(add(add(mul(V, vk["r_v"]), mul(W, vk["r_w"])), mul(Y, vk["r_y"])), vk["beta"])
        a = vk["alpha"]
        els = [V, mul(V, a), W, mul(W, a), Y, mul(Y, a), Hh, mul(Hh, a), Lb]
    return dev.enc_encode(vk["sk"], torch.stack(els).contiguous(), 7)


def measure(say, scheme, preset, cs, label):
    rng = np.random.RandomState(3)
    prm = P.preset(preset)
    dev = Device(prm)
    say()
    say("## %s: %s (N = %d, L = %d, N_enc = %d, K = %d; %s arithmetic), %s: m = %d, n_inputs = %d"
        % (scheme, preset, prm.N, prm.L, prm.N_enc, prm.K, "integer" if any(p >= 1 << 50 for p in prm.q + prm.Q) else "FP64", label, cs.m,
           cs.n_inputs))
    dcs = dev.r1cs(cs)
    names = ("alpha", "beta", "gamma", "delta") if scheme == "groth16" else ("alpha", "beta", "r_v", "r_w")
    vk = {k: dev.put(random_ring(prm, rng, 1, lo=1)[0]) for k in names}
    vk.update(sk=secret_key(dev, rng), s=dev.put(random_ring(prm, rng, 1, lo=cs.m)[0]))
    if scheme == "rinocchio":
        vk["r_y"] = dev.ring_mul(vk["r_v"], vk["r_w"])
    make_vk, single, batch = ((dev.groth16_vk, dev.groth16_verify, dev.groth16_verify_batch) if scheme == "groth16" else
                              (dev.rinocchio_vk, dev.rinocchio_verify, dev.rinocchio_verify_batch))
    dvk = make_vk(dcs, vk)
    primary = dev.put(random_ring(prm, rng, cs.n_inputs))
    proof = accepted_proof(dev, scheme, dcs, vk, primary, rng)
    ref = single(dvk, primary, proof)
    assert ref.accepted, ref
    B_max = max(BATCHES)
    primaries = primary.unsqueeze(0).repeat(B_max, 1, 1, 1).contiguous()
    proofs = proof.unsqueeze(0).repeat(B_max, *([1] * proof.dim())).contiguous()
    say("proofs of the batch: %.1f MiB each, primary inputs %.2f MiB each; the public columns of the key %.2f MiB"
        % (proof.numel() * 8 / 2**20, primary.numel() * 8 / 2**20, 3 * (cs.n_inputs + 1) * prm.L * prm.N * 8 / 2**20))
    say("B | B single calls, per proof | one batch call, per proof | batch / single (medians)")
    ratio = {}
    for B in BATCHES:
        got = batch(dvk, primaries[:B], proofs[:B])
        assert len(got) == B and all(g.result == ref and not g.noise_spent for g in got)  # the single verifier's report, member by member
        t_single, t_batch = [], []
        for k in range(WARM + REPEATS):
            dev.sync()
            t0 = time.perf_counter()
            for b in range(B):
                single(dvk, primaries[b], proofs[b])
            dev.sync()
            t1 = time.perf_counter()
            batch(dvk, primaries[:B], proofs[:B])
            dev.sync()
            t2 = time.perf_counter()
            if k >= WARM:
                t_single.append((t1 - t0) * 1e3 / B)
                t_batch.append((t2 - t1) * 1e3 / B)
        ratio[B] = statistics.median(t_batch) / statistics.median(t_single)
        say("%d | %s | %s | %.3f" % (B, spread(t_single), spread(t_batch), ratio[B]))
    say("condition (per-proof time of a batch of 64 not above the single call's): %s (ratio %.3f)"
        % ("met" if ratio[64] <= 1.0 else "NOT met", ratio[64]))
    for B in BATCHES:
        dev.set_profiling(True)
        batch(dvk, primaries[:B], proofs[:B])
        recs = dev.profile_read()
        dev.set_profiling(False)
        say("kernels of one batch call, B = %d: %s" % (B, "; ".join("%s %.4f ms (%.1f GB/s algorithmic)" % (
            r["name"], r["total_ms"], r["alg_bytes"] / max(r["total_ms"], 1e-9) / 1e6) for r in recs)))
    dev.set_profiling(True)
    single(dvk, primary, proof)
    recs = dev.profile_read()
    dev.set_profiling(False)
    say("kernels of one single call: %s" % "; ".join("%s %.4f ms" % (r["name"], r["total_ms"]) for r in recs))
    dvk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "verify_batch.txt"))
    ap.add_argument("--resource-usage", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        lines.append(s)
        print(s, flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    say("# tools/verify_batch_time.py on %s; library sources %s; warm-up %d, median of %d; host clock around calls that synchronise"
        % (torch.cuda.get_device_name(0), _lib.source_hash(), WARM, REPEATS))
    say("# register group of the check kernel: %d proofs per thread; at most %d proofs per call" % (_lib.VERIFY_BATCH_GROUP, _lib.VERIFY_BATCH_MAX))
    c3, c5 = P.preset("C3"), P.preset("C5")
    measure(say, "groth16", "C3", R.chain_r1cs(64, c3.q), "chain circuit")
    torch.cuda.empty_cache()
    measure(say, "rinocchio", "C5", R.logreg_r1cs(c5.q, 256), "logistic regression, 256 features")
    if args.resource_usage:
        say()
        say("## verify_batch_kernel<arithmetic, scheme>: the compiler's resource usage for gfx950 (ModI: integer, Mod: FP64; Li0: ringGroth16, Li1: Rinocchio)")
        for ln in open(args.resource_usage).read().splitlines():
            say(ln)


if __name__ == "__main__":
    main()
