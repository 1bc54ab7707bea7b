"""The bit decomposition (ringsnark_amd/bits.h) and the range-check circuit built on it (ringsnark_amd.r1cs.plaintext_check_r1cs,
the form without constants), on one MI355X.

  (a) kernel   rs_ring_bit_decompose at the C3 shape (N = 8192, L = 4), nbits = 32, 256 elements = 2 GiB of bit rows: the
               kernel alone from the library's events (rs_set_profiling) and the whole call between two stream events; beside
               it rs_ring_neg on the same total bytes between two stream events, and rs_measure_peaks' copy rate, all from
               this run.  Algorithmic bytes of the decomposition: (1 + nbits) * count * L * N * 8.
  (b) old way  the same bit rows as a caller had to make them before: download x, split with numpy, upload nbits rows per x;
               host clock around the whole.
  (c) circuit  Setup (rs_rinocchio_keygen + rs_rinocchio_vk_create), witness (upload-free: bits in place + rs_r1cs_check),
               Prove (rs_rinocchio_prove) and Verify (rs_rinocchio_verify) of the constant-free circuit, host clock around calls
               that synchronise:  C5 (N = 2048, N_enc = 16384: the ring of the reference's bench_plaintext_check_SEAL.cpp),
               logT = 32, count = 1, device-resident key;  C3, logT = 32, count = 1985 (m = 65505, just under 2^16), a seeded
               host-resident key (3 x 64 GiB of page-locked host memory; a full key would be 384 GiB).
One run; 2 warm-ups, then the median of 7 (min and max beside it).

usage: python tools/plaintext_check_time.py [--out profiles/plaintext_check.txt] [--skip-large]
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
from ringsnark_amd.device import Device, to_host  # noqa: E402

REPEATS, WARM = 7, 2
NBITS = 32


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


def spread(t, unit="ms", fmt="%.3f"):
    return (fmt + " %s (min " + fmt + ", max " + fmt + ")") % (statistics.median(t), unit, min(t), max(t))


def rate(nbytes, t_ms):
    """GB/s at the median, with the rates of the slowest and the fastest repetition"""
    g = lambda ms: nbytes / (ms * 1e-3) / 1e9
    return "%.0f GB/s (%.0f - %.0f)" % (g(statistics.median(t_ms)), g(max(t_ms)), g(min(t_ms)))


def event_time(f):
    """device time of one asynchronous call between two stream events"""
    t = []
    for k in range(WARM + REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        if k >= WARM:
            t.append(e0.elapsed_time(e1))
    return t


def host_time(dev, f):
    """host clock around a call, synchronised before and after"""
    t = []
    for k in range(WARM + REPEATS):
        dev.sync()
        t0 = time.perf_counter()
        f()
        dev.sync()
        if k >= WARM:
            t.append((time.perf_counter() - t0) * 1e3)
    return t


def library_time(dev, f, name):
    """the library's own events around the kernel `name` (rs_set_profiling), one call per repetition"""
    t = []
    for k in range(WARM + REPEATS):
        dev.set_profiling(True)
        f()
        dev.sync()
        recs = [r for r in dev.profile_read() if r["name"] == name]
        dev.set_profiling(False)
        assert len(recs) == 1 and recs[0]["launches"] == 1, recs
        if k >= WARM:
            t.append(recs[0]["total_ms"])
    return t, recs[0]["alg_bytes"]


def values(dev, count, nbits, seed):
    """[count][L][N] on the device: one integer below 2^nbits per slot, the same word in every limb"""
    g = torch.Generator(device=dev.device)
    g.manual_seed(seed)
    v = torch.randint(0, 1 << nbits, (count, 1, dev.N), dtype=torch.int64, device=dev.device, generator=g)
    return v.expand(count, dev.L, dev.N).contiguous()


def mem_available_gib():
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            return int(line.split()[1]) / 2**20
    return 0.0


def circuit(say, name, count, rng, host_key):
    prm = P.preset(name)
    dev = Device(prm)
    cs = R.plaintext_check_r1cs(prm.q, NBITS, count)
    m, w = cs.m, NBITS + 1
    key_gib = (2 * (m + 1) + cs.n_aux) * prm.enc_words * 8 / 2**30
    say()
    say("## (c) %s: N = %d, L = %d, N_enc = %d, K = %d; logT = %d, count = %d: m = %d constraints, %d variables; %s key"
        % (name, prm.N, prm.L, prm.N_enc, prm.K, NBITS, count, m, cs.n_vars,
           "seeded host-resident (%.0f GiB; %.0f GiB in full)" % (key_gib / 2, key_gib) if host_key else "device-resident (%.2f GiB)" % key_gib))
    dcs = dev.r1cs(cs)
    dsk = secret_key(dev, rng)
    vk = {k: dev.put(random_ring(prm, rng, 1, lo=1)[0]) for k in ("alpha", "beta", "r_v", "r_w")}
    vk.update(sk=dsk, s=dev.put(random_ring(prm, rng, 1, lo=m)[0]), r_y=None)
    vk["r_y"] = dev.ring_mul(vk["r_v"], vk["r_w"])
    asg = dev.ring_empty(cs.n_vars)
    asg[0] = 1
    asg[1:].view(count, w, prm.L, prm.N)[:, NBITS] = values(dev, count, NBITS, 5)
    dev.sync()

    def witness():
        rep = dev.plaintext_check_fill_bits(asg, cs, count)
        chk = dev.r1cs_check(dcs, asg)
        assert rep and chk.satisfied, (rep, chk)

    say("bits in place + rs_r1cs_check:  %s" % spread(host_time(dev, witness)))
    kw = dict(seeds=11, host=True, seeded=True) if host_key else dict(seeds=11)
    t0 = time.perf_counter()
    state = {"pk": dev.rinocchio_keygen(dcs, vk, **kw), "dvk": None}
    say("(first Setup call, with the allocation of the key: %.1f s)" % (time.perf_counter() - t0))

    def setup():
        if state["dvk"] is not None:
            state["dvk"].close()
        pub = dict(pub_seeds=state["pk"]["pub_seeds"]) if host_key else {}
        state["pk"] = dev.rinocchio_keygen(dcs, vk, into=state["pk"], **kw, **pub)
        state["dvk"] = dev.rinocchio_vk(dcs, vk)

    say("Setup  (rs_rinocchio_keygen%s + rs_rinocchio_vk_create):  %s" % ("_seeded" if host_key else "", spread(host_time(dev, setup))))
    out = {}

    def prove():
        out["proof"], out["empty"] = dev.rinocchio_prove(dcs, state["pk"], asg)

    say("Prove  (rs_rinocchio_prove%s, non-ZK):  %s" % ("_seeded" if host_key else "", spread(host_time(dev, prove))))
    primary = asg[:1].contiguous()

    def verify():
        out["verdict"] = dev.rinocchio_verify(state["dvk"], primary, out["proof"], out["empty"])

    say("Verify (rs_rinocchio_verify):  %s" % spread(host_time(dev, verify)))
    say("       verdict: %s; noise budget of the nine proof elements, min over limbs: %s"
        % ("accepted" if out["verdict"].accepted else "REJECTED %s" % (out["verdict"],),
           [int(b.min()) for b in dev.enc_noise_budget(dsk, out["proof"])]))
    state["dvk"].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "plaintext_check.txt"))
    ap.add_argument("--skip-large", action="store_true", help="leave out the C3 circuit (192 GiB of page-locked host memory)")
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
    say("# tools/plaintext_check_time.py on %s; library sources %s; warm-up %d, median of %d (min, max)"
        % (torch.cuda.get_device_name(0), _lib.source_hash(), WARM, REPEATS))
    peaks = dev.measure_peaks()
    say("# C3: N = %d, L = %d; peaks of this run: %s" % (prm.N, prm.L, peaks))

    count = (2 << 30) // (NBITS * prm.ring_words * 8)
    x = values(dev, count, NBITS, 1)
    bits = dev.ring_empty(count, NBITS)
    alg = (1 + NBITS) * count * prm.ring_words * 8
    say()
    say("## (a) rs_ring_bit_decompose, nbits = %d, count = %d: %.3f GiB written, %.4f GiB read; algorithmic bytes %d"
        % (NBITS, count, NBITS * count * prm.ring_words * 8 / 2**30, count * prm.ring_words * 8 / 2**30, alg))
    call = lambda: dev.ring_bit_decompose(x, NBITS, out=bits, want_report=False)
    t_lib, lib_bytes = library_time(dev, call, "ring_bit_decompose_kernel")
    assert lib_bytes == alg, (lib_bytes, alg)
    say("ring_bit_decompose_kernel, the library's events:    %s = %s" % (spread(t_lib), rate(alg, t_lib)))
    t_call = event_time(call)
    say("the whole call (two memsets, kernel, report kernel):   %s = %s" % (spread(t_call), rate(alg, t_call)))
    _, rep = dev.ring_bit_decompose(x, NBITS, out=bits)
    assert rep, rep
    n_neg = alg // (2 * prm.ring_words * 8)
    a = dev.ring_empty(n_neg)
    dev.fill_uniform(a, 0, 9)
    dst = torch.empty_like(a)
    neg = lambda: _lib.check(dev.lib.rs_ring_neg(dev.h, dst.data_ptr(), a.data_ptr(), n_neg, dev.stream()))
    t_neg = event_time(neg)
    neg_bytes = 2 * n_neg * prm.ring_words * 8
    say("rs_ring_neg on %d elements (%d bytes read + written):  %s = %s" % (n_neg, neg_bytes, spread(t_neg), rate(neg_bytes, t_neg)))
    say("rs_measure_peaks hbm_copy_gbs:                          %.0f GB/s" % peaks["hbm_copy_gbs"])
    del a, dst

    say()
    say("## (b) the same rows the old way: download x, numpy, upload %d rows per x (host clock)" % NBITS)
    parts = {"download": [], "numpy": [], "upload": []}

    def old_way():
        t0 = time.perf_counter()
        h = to_host(x)
        t1 = time.perf_counter()
        hb, _ = R.bit_decompose(h, NBITS, prm.q)
        t2 = time.perf_counter()
        bits.copy_(torch.from_numpy(hb.view(np.int64)))
        dev.sync()
        t3 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[k].append(v * 1e3)

    t_old = host_time(dev, old_way)
    say("download + numpy + upload:  %s" % spread(t_old, fmt="%.1f"))
    say("  of which " + "; ".join("%s %s" % (k, spread(v[WARM:], fmt="%.1f")) for k, v in parts.items()) + "; the rest: releasing the host arrays")
    say("rs_ring_bit_decompose with its report (synchronises), host clock:  %s" % spread(host_time(dev, lambda: dev.ring_bit_decompose(x, NBITS, out=bits))))
    del dev, x, bits
    torch.cuda.empty_cache()

    circuit(say, "C5", 1, rng, host_key=False)
    torch.cuda.empty_cache()
    if args.skip_large:
        say()
        say("## (c) C3, count = 1985: left out (--skip-large)")
        return
    need = 3 * 65506 * P.preset("C3").enc_words * 4 / 2**30
    avail = mem_available_gib()
    if avail < 1.25 * need:
        say()
        say("## (c) C3, count = 1985: NOT MEASURED -- the seeded host-resident key needs %.0f GiB of page-locked host memory, MemAvailable is %.0f GiB" % (need, avail))
        return
    circuit(say, "C3", 1985, rng, host_key=True)


if __name__ == "__main__":
    main()
