"""Seeded proving keys (ringsnark_amd/seeded.h) against the full key they replace, REAL untiled keys from the device generator:
in one session on one machine, after one warm-up, the median of 5 ringGroth16 proofs with
  * a full host-resident key (the parent's path: 3 m elements of 2 L K N_enc words, streamed over the host link),
  * a seeded host-resident key of the same plaintext rows (the same trapdoor and private seeds; c0 only, half the bytes),
  * a seeded device-resident key, if it fits in HBM beside the prover's workspace,
with msm_ms, total time and GB/s for each, the ratio seeded / full of msm_ms, and the expansion kernel's time per tile beside
the host-to-device copy time of that tile's c0 (events).  A key that does not pass the host-memory guard of
tools/host_key_headline.py is left out (the full key at 2^15 constraints of the headline shape: 192 GiB) -- the run is then
the seeded key alone.  Two slabs of the seeded proof are checked against the CPU oracle as tools/host_key_headline.py does,
with the key expanded on the host from c0 and the public seed in numpy.
usage: tools/seeded_key_time.py [logm] [preset] [--out FILE]    (defaults: 14, C3, profiles/seeded_key.txt)"""
import argparse
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ringsnark_amd import params as P  # noqa: E402
from ringsnark_amd import r1cs as R  # noqa: E402
from ringsnark_amd import _lib  # noqa: E402
from ringsnark_amd.device import Device, to_host  # noqa: E402

MASK = (1 << 64) - 1


def splitmix_at(seed, k):
    """k-th output (1-based) of the splitmix64 stream `seed` (csrc/rs_internal.hpp); seed, k: uint64 arrays"""
    with np.errstate(over="ignore"):
        z = seed + k * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def c1_slab(prm, pub_seed, count, limb, j, step=2048):
    """the (limb, c1, j) slab [count][N_enc] of a seeded vector with public seed pub_seed (enc_encode's convention), on the host"""
    n = prm.N_enc
    out = np.empty((count, n), dtype=np.uint64)
    draw = np.arange(n + j * n + 1, n + j * n + n + 1, dtype=np.uint64)[None, :]
    word = (pub_seed * 65537) & MASK
    for k0 in range(0, count, step):
        k = np.arange(k0, min(count, k0 + step), dtype=np.uint64)
        with np.errstate(over="ignore"):
            seed = (np.uint64(word) + k) * np.uint64(1315423911) + np.uint64(limb + 1)
        out[k0:k0 + len(k)] = splitmix_at(seed[:, None], draw) % np.uint64(prm.Q[j])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logm", nargs="?", type=int, default=14)
    ap.add_argument("preset", nargs="?", default="C3")
    ap.add_argument("--out", default="profiles/seeded_key.txt")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        open(a.out, "w").write("\n".join(lines) + "\n")

    prm = P.preset(a.preset)
    m = 1 << a.logm
    dev = Device(prm)
    ew = prm.enc_words
    full_gib = (3 * m + 2) * ew * 8 / 2**30
    seeded_gib = ((3 * m + 2) * (ew // 2) + 2 * ew) * 8 / 2**30
    try:
        limit = int(open("/sys/fs/cgroup/memory.max").read())
    except Exception:
        limit = None
    avail = int([l for l in open("/proc/meminfo") if l.startswith("MemAvailable")][0].split()[1]) * 1024
    room = 0.6 * min(avail, limit or avail)
    say("# tools/seeded_key_time.py %d %s: ringGroth16, m = 2^%d constraints, N = %d, L = %d, N_enc = %d, K = %d" % (a.logm, prm.name, a.logm, prm.N, prm.L, prm.N_enc, prm.K))
    say("full key %.0f GiB, seeded key %.0f GiB; host memory available %.0f GiB, cgroup limit %s" % (full_gib, seeded_gib, avail / 2**30, limit))
    with_full = (full_gib + seeded_gib) * 2**30 <= room
    if not with_full:
        say("the full key (beside the seeded one) does not pass the host-memory guard (60 % of the memory a job gets): seeded key only")
    if seeded_gib * 2**30 > room:
        say("not enough host memory for the seeded key: refusing")
        sys.exit(2)

    from tests import helpers as H
    from tests.proof_check import check_columns, slab_inner_product
    octx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    asg = dev.ring_empty(m + 2)
    dev.fill_uniform(asg[:2], 0, 7)
    dev.chain_assignment(asg, m)
    rng = np.random.RandomState(3)
    unit = lambda lo: np.stack([(rng.randint(0, 2**62, size=prm.N, dtype=np.int64).astype(np.uint64) % np.uint64(p - lo)) + np.uint64(lo) for p in prm.q])
    vk = dict(s=unit(m), alpha=unit(1), beta=unit(1), delta=unit(1), sk=octx.keygen(5))

    keys = []
    t0 = time.time()
    if with_full:
        keys.append(("full host key", dev.groth16_keygen(dcs, vk, seeds=1, host=True), full_gib))
        say("full key generated into page-locked host memory in %.1f s" % (time.time() - t0))
    t0 = time.time()
    seeded_host = dev.groth16_keygen(dcs, vk, seeds=1, host=True, seeded=True)
    keys.append(("seeded host key", seeded_host, seeded_gib))
    say("seeded key generated into page-locked host memory in %.1f s" % (time.time() - t0))
    free, _ = torch.cuda.mem_get_info(dev.device)
    need = seeded_gib * 2**30 + 6 * m * prm.ring_words * 8 + (24 << 30)  # the key, the prover's vectors, staging and row workspaces
    if free > need:
        t0 = time.time()
        keys.append(("seeded device key", dev.groth16_keygen(dcs, vk, seeds=1, seeded=True, pub_seeds=seeded_host["pub_seeds"]), seeded_gib))
        say("seeded key generated into HBM in %.1f s (%.0f GiB free before)" % (time.time() - t0, free / 2**30))
    else:
        say("seeded device-resident key: %.0f GiB free, %.0f GiB needed -- left out" % (free / 2**30, need / 2**30))

    dev.set_profiling(True)
    result, proofs = {}, {}
    for label, pk, gib in keys:
        times, msm = [], []
        for s in range(6):  # one warm-up, then 5
            dev.profile_read()
            torch.cuda.synchronize()
            t0 = time.time()
            proof, _ = dev.groth16_prove(dcs, pk, asg, want_empty=False)
            torch.cuda.synchronize()
            if s:
                times.append((time.time() - t0) * 1e3)
                msm.append(dev.last_timings()["msm_ms"])
        prof = dev.profile_read()
        proofs[label] = proof
        result[label] = (statistics.median(msm), statistics.median(times))
        say("%-18s msm_ms %8.1f  total %8.1f ms  = %6.0f constraints/s; key read at %6.1f GB/s (%.0f GiB per proof)"
            % (label, result[label][0], result[label][1], m / result[label][1] * 1e3, gib * 2**30 / result[label][1] / 1e6, gib))
        say("    kernels of the last proof: " + "; ".join("%s %.1f ms x%d" % (p["name"], p["total_ms"], p["launches"]) for p in prof[:6]))
    dev.set_profiling(False)
    if "seeded device key" in proofs:
        assert (to_host(proofs["seeded device key"]) == to_host(proofs["seeded host key"])).all(), "the same seeded key on the host and in HBM gives two proofs"
        say("the seeded key gives the same proof from host memory and from HBM")
    if with_full:
        ratio = result["seeded host key"][0] / result["full host key"][0]
        say("msm_ms seeded host key / full host key = %.3f" % ratio)

    # the expansion kernel on one staging tile beside the host-to-device copy of that tile's c0
    tile = min(_lib.get_tuning("msm_host_tile"), m + 1)
    c0_words = tile * (ew // 2)
    d_c0 = torch.empty(c0_words, dtype=torch.int64, device=dev.device).view(tile, prm.L, prm.K, prm.N_enc)
    import ctypes as C
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t_copy, t_expand = [], []
    for s in range(6):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        _lib.check(dev.lib.rs_upload(dev.h, C.c_void_p(d_c0.data_ptr()), C.c_void_p(seeded_host["s_pows"].ptr), c0_words * 8, dev.stream()))
        e1.record()
        out = dev.enc_expand_seeded(d_c0, seeded_host["pub_seeds"][0])
        e2.record()
        torch.cuda.synchronize()
        if s:
            t_copy.append(e0.elapsed_time(e1))
            t_expand.append(e1.elapsed_time(e2))
        del out
    tc, te = statistics.median(t_copy), statistics.median(t_expand)
    say("tile of %d elements: c0 copy host -> device %.2f ms (%.1f GB/s), expand_seeded_tile_kernel %.2f ms (%.0f GB/s written + read)"
        % (tile, tc, c0_words * 8 / tc / 1e6, te, 3 * c0_words * 8 / te / 1e6))
    say("the expansion %s under the copy of the next tile" % ("hides" if te < tc else "DOES NOT hide"))
    if with_full and ratio > 0.6:
        tiles = 3 * ((m + 1 + tile - 1) // tile)
        say("ratio above 0.6: per proof the c0 copies alone take %.0f ms at the measured tile rate, the expansions %.0f ms, of msm_ms %.0f"
            % (tiles * tc, tiles * te, result["seeded host key"][0]))
    del d_c0

    # two proof slabs of the seeded proof against the CPU oracle, from the host key itself: A reads c0 of s_pows as stored,
    # C reads c1 of delta_ts and delta_mid, regenerated here from the public seeds
    proof = proofs["seeded host key"]
    pk = seeded_host
    w = dev.witness_map(dcs, asg, want=("A_io", "A_mid", "B_io", "B_mid", "H"))
    rng = np.random.RandomState(5)
    err = check_columns(prm, cs, asg, w, [(int(rng.randint(prm.L)), int(rng.randint(prm.N))) for _ in range(2)], rng)
    assert err is None, err
    c0 = lambda hw, T, l, j: np.ascontiguousarray(hw.array.reshape(T, prm.L, prm.K, prm.N_enc)[:, l, j, :])
    for elem, l, c, j in (("A", 1, 0, 2), ("C", 3, 1, 0)):
        acc = np.zeros(prm.N_enc, dtype=np.uint64)
        if elem == "A":
            k = c0(pk["s_pows"], m + 1, l, j)
            slab_inner_product(octx, acc, k, w["A_io"], l, j, m)
            slab_inner_product(octx, acc, k, w["A_mid"], l, j, m)
            acc = (acc + to_host(pk["alpha"][l, c, j].contiguous())) % np.uint64(prm.Q[j])
        else:
            slab_inner_product(octx, acc, c1_slab(prm, pk["pub_seeds"][1], m + 1, l, j), w["H"], l, j, m + 1)
            slab_inner_product(octx, acc, c1_slab(prm, pk["pub_seeds"][2], cs.n_aux, l, j), asg[cs.n_inputs:], l, j, cs.n_aux)
        got = to_host(proof[{"A": 0, "C": 2}[elem], l, c, j].contiguous())
        assert (acc == got).all(), "proof element %s slab differs from the CPU oracle" % elem
    say("proof slabs A[limb 1][comp 0][prime 2], C[limb 3][comp 1][prime 0] of the seeded proof equal the CPU oracle's; witness identities hold")


if __name__ == "__main__":
    main()
