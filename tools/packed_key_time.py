"""Bit-packed seeded proving keys (ringsnark_amd/packed.h) against the seeded keys they replace, REAL untiled keys from the
device generator, ringGroth16.  One process per m; after one warm-up, the median of 5 proofs with min-max.
  (a) logm < 16: a seeded and a packed key of the same trapdoor and seeds, host-resident and (if they fit) device-resident, in
      the same run: msm_ms, total, key bytes per proof, GB/s of the key read; the ratio packed / seeded of msm_ms.
  (b) one staging tile: expand_packed_tile_kernel against expand_seeded_tile_kernel on the same elements (events).
  (c) logm >= 16: the packed key alone, generated into HBM if `free HBM >= key + prover workspace`, else into host memory;
      free HBM before and after, the proof time.
Two slabs of a packed proof are checked against the CPU oracle as tools/seeded_key_time.py does, the key slab unpacked on the
host in numpy from the packed words themselves and c1 regenerated from the public seed.
usage: tools/packed_key_time.py [logm] [preset] [--out FILE]    (defaults: 14, C3, profiles/packed_key.txt; the file is appended to)"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from ringsnark_amd import packed as PK  # noqa: E402
from ringsnark_amd import params as P  # noqa: E402
from ringsnark_amd import r1cs as R  # noqa: E402
from ringsnark_amd import _lib  # noqa: E402
from ringsnark_amd.device import Device, HostWords, to_host  # noqa: E402

_spec = importlib.util.spec_from_file_location("seeded_key_time", os.path.join(os.path.dirname(os.path.abspath(__file__)), "seeded_key_time.py"))
seeded_key_time = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(seeded_key_time)
c1_slab = seeded_key_time.c1_slab


def unpack_slab(words, w, n):
    """[T][row_words] packed rows -> [T][n] residues: per residue a gather of its one or two words (packed.unpack_rows goes
    through single bits, too slow for 2^16 rows; the two agree on the first rows, asserted)"""
    bit = np.arange(n, dtype=np.uint64) * np.uint64(w)
    wi, sh = (bit >> np.uint64(6)).astype(np.int64), bit & np.uint64(63)
    out = words[:, wi] >> sh
    two = (sh + np.uint64(w)) > np.uint64(64)
    out[:, two] |= words[:, wi[two] + 1] << (np.uint64(64) - sh[two])
    out &= np.uint64((1 << w) - 1)
    assert (out[:4] == PK.unpack_rows(words[:4], w, n)).all()
    return out


def spread(xs):
    return "%.1f (%.1f-%.1f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logm", nargs="?", type=int, default=14)
    ap.add_argument("preset", nargs="?", default="C3")
    ap.add_argument("--out", default="profiles/packed_key.txt")
    a = ap.parse_args()
    out = open(a.out, "a")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    prm = P.preset(a.preset)
    m = 1 << a.logm
    dev = Device(prm)
    ew, pw, w = prm.enc_words, dev.packed_words, dev.pack_bits
    gib = lambda words: ((3 * m + 2) * words + 2 * ew) * 8 / 2**30
    seeded_gib, packed_gib = gib(ew // 2), gib(pw)
    compare = a.logm < 16
    try:
        limit = int(open("/sys/fs/cgroup/memory.max").read())
    except Exception:
        limit = None
    avail = int([l for l in open("/proc/meminfo") if l.startswith("MemAvailable")][0].split()[1]) * 1024
    room = 0.6 * min(avail, limit or avail)
    say("# tools/packed_key_time.py %d %s: ringGroth16, m = 2^%d constraints, N = %d, L = %d, N_enc = %d, K = %d, w = %d bits"
        % (a.logm, prm.name, a.logm, prm.N, prm.L, prm.N_enc, prm.K, w))
    say("seeded key %.1f GiB, packed key %.1f GiB (%.4f of it; w / 64 = %.4f); host memory available %.0f GiB, cgroup limit %s"
        % (seeded_gib, packed_gib, packed_gib / seeded_gib, w / 64, avail / 2**30, limit))

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
    PUB = 31337
    work = 6 * m * prm.ring_words * 8 + (24 << 30)  # the prover's vectors, staging and row workspaces (tools/seeded_key_time.py)

    def keygen(packed, host):
        return dev.groth16_keygen(dcs, vk, seeds=1, pub_seeds=PUB, seeded=True, packed=packed, host=host)

    def measure(label, pk, key_gib):
        """(median msm_ms, list of msm_ms, proof) of one warm-up and 5 proofs"""
        times, msm = [], []
        dev.set_profiling(True)
        for s in range(6):
            dev.profile_read()
            torch.cuda.synchronize()
            t0 = time.time()
            proof, _ = dev.groth16_prove(dcs, pk, asg, want_empty=False)
            torch.cuda.synchronize()
            if s:
                times.append((time.time() - t0) * 1e3)
                msm.append(dev.last_timings()["msm_ms"])
        prof = dev.profile_read()
        dev.set_profiling(False)
        med = statistics.median(msm)
        say("%-18s msm_ms %s  total %s ms  = %6.0f constraints/s; %.1f GiB of key per proof, read at %6.1f GB/s of msm_ms"
            % (label, spread(msm), spread(times), m / statistics.median(times) * 1e3, key_gib, key_gib * 2**30 / med / 1e6))
        say("    kernels of the last proof: " + "; ".join("%s %.1f ms x%d" % (p["name"], p["total_ms"], p["launches"]) for p in prof[:6]))
        return med, msm, proof

    res, proofs, checked = {}, {}, None
    plans = [(False, True), (True, True), (False, False), (True, False)] if compare else [(True, False)]
    for packed, host in plans:
        label = "%s %s key" % ("packed" if packed else "seeded", "host" if host else "device")
        key_gib = packed_gib if packed else seeded_gib
        free, total = torch.cuda.mem_get_info(dev.device)
        if host and key_gib * 2**30 > room:
            say("%s: %.0f GiB does not pass the host-memory guard (60 %% of the memory a job gets) -- left out" % (label, key_gib))
            continue
        if not host and free < key_gib * 2**30 + work:
            say("%s: %.1f GiB of HBM free, %.1f GiB needed (key %.1f + workspace %.1f) -- does not fit" % (label, free / 2**30, (key_gib * 2**30 + work) / 2**30, key_gib, work / 2**30))
            if not compare:  # (c): the host-resident packed key takes its place
                plans.append((True, True))
            continue
        t0 = time.time()
        try:
            pk = keygen(packed, host)
        except (_lib.RsError, RuntimeError) as e:  # out of memory beside the generator's scratch
            say("%s: generation failed with %.1f GiB of HBM free: %s" % (label, free / 2**30, str(e)[:200]))
            torch.cuda.empty_cache()
            if not compare and not host:
                plans.append((True, True))
            continue
        free_after, _ = torch.cuda.mem_get_info(dev.device)
        say("%s generated into %s in %.1f s; HBM free %.1f GiB before, %.1f GiB after (of %.1f)"
            % (label, "page-locked host memory" if host else "HBM", time.time() - t0, free / 2**30, free_after / 2**30, total / 2**30))
        try:
            med, msm, proof = measure(label, pk, key_gib)
        except (_lib.RsError, RuntimeError) as e:  # the prover's workspace does not fit beside the key after all
            say("%s: proving failed with %.1f GiB of HBM free after generation: %s" % (label, free_after / 2**30, str(e)[:200]))
            dev.set_profiling(False)
            del pk
            torch.cuda.empty_cache()
            if not compare and not host:
                plans.append((True, True))
            continue
        if not host:
            say("    HBM free after the proofs: %.1f GiB" % (torch.cuda.mem_get_info(dev.device)[0] / 2**30))
        res[label], proofs[label] = (med, msm), to_host(proof)
        check_now = packed and checked is None
        if check_now:  # the pieces of the slab check below that need the key, taken before it is released
            rw = pw // (prm.L * prm.K)
            v = pk["s_pows"]
            rows = v.array.reshape(m + 1, prm.L, prm.K, rw)[:, 1, 2, :] if isinstance(v, HostWords) else to_host(v[:, 1, 2, :].contiguous())
            k_slab = unpack_slab(np.ascontiguousarray(rows), w, prm.N_enc)
            alpha_slab, pubs = to_host(pk["alpha"][1, 0, 2].contiguous()), list(pk["pub_seeds"])
            del v, rows
        if compare and packed and host:  # (b) on the first tile of this key, before it is released
            tile = min(_lib.get_tuning("msm_host_tile"), m + 1)
            d_packed = dev.put(np.array(pk["s_pows"].array[: tile * pw]).reshape(tile, prm.L, prm.K, pw // (prm.L * prm.K)))
            d_c0 = dev.enc_unpack_c0(d_packed)
            ev = lambda: torch.cuda.Event(enable_timing=True)
            t_s, t_p = [], []
            for s in range(6):
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                o1 = dev.enc_expand_seeded(d_c0, PUB)
                e1.record()
                o2 = dev.enc_expand_packed(d_packed, PUB)
                e2.record()
                torch.cuda.synchronize()
                if s:
                    t_s.append(e0.elapsed_time(e1))
                    t_p.append(e1.elapsed_time(e2))
                else:
                    assert bool((o1 == o2).all())
                del o1, o2
            full_bytes = tile * ew * 8
            say("tile of %d elements: expand_seeded_tile_kernel %s ms (%.0f GB/s read + written), expand_packed_tile_kernel %s ms (%.0f GB/s read + written)"
                % (tile, "%.3f (%.3f-%.3f)" % (statistics.median(t_s), min(t_s), max(t_s)), 1.5 * full_bytes / statistics.median(t_s) / 1e6,
                   "%.3f (%.3f-%.3f)" % (statistics.median(t_p), min(t_p), max(t_p)), (full_bytes + tile * pw * 8) / statistics.median(t_p) / 1e6))
            del d_packed, d_c0
        del pk, proof
        torch.cuda.empty_cache()
        if check_now:
            # two proof slabs against the CPU oracle, from the packed key itself: A reads c0 of s_pows, unpacked above on the
            # host; C reads c1 of delta_ts and delta_mid, regenerated here from the public seeds
            wm = dev.witness_map(dcs, asg, want=("A_io", "A_mid", "B_io", "B_mid", "H"))
            r5 = np.random.RandomState(5)
            err = check_columns(prm, cs, asg, wm, [(int(r5.randint(prm.L)), int(r5.randint(prm.N))) for _ in range(2)], r5)
            assert err is None, err
            for elem, l, c, j in (("A", 1, 0, 2), ("C", 3, 1, 0)):
                acc = np.zeros(prm.N_enc, dtype=np.uint64)
                if elem == "A":
                    slab_inner_product(octx, acc, k_slab, wm["A_io"], l, j, m)
                    slab_inner_product(octx, acc, k_slab, wm["A_mid"], l, j, m)
                    acc = (acc + alpha_slab) % np.uint64(prm.Q[j])
                else:
                    slab_inner_product(octx, acc, c1_slab(prm, pubs[1], m + 1, l, j), wm["H"], l, j, m + 1)
                    slab_inner_product(octx, acc, c1_slab(prm, pubs[2], cs.n_aux, l, j), asg[cs.n_inputs:], l, j, cs.n_aux)
                got = proofs[label].reshape(3, prm.L, 2, prm.K, prm.N_enc)[{"A": 0, "C": 2}[elem], l, c, j]
                assert (acc == got).all(), "proof element %s slab differs from the CPU oracle" % elem
            del wm, k_slab
            torch.cuda.empty_cache()
            checked = label
            say("    proof slabs A[limb 1][comp 0][prime 2], C[limb 3][comp 1][prime 0] of the %s's proof equal the CPU oracle's; witness identities hold" % label)

    if compare:
        for where in ("host", "device"):
            s, p = res.get("seeded %s key" % where), res.get("packed %s key" % where)
            if s and p:
                assert (proofs["seeded %s key" % where] == proofs["packed %s key" % where]).all(), "the packed key gives another proof"
                say("%s-resident: msm_ms packed / seeded = %.3f (medians; min / max of the 5 x 5 quotients %.3f / %.3f); expected w / 64 = %.4f for a link-bound pass; the proofs are equal"
                    % (where, p[0] / s[0], min(p[1]) / max(s[1]), max(p[1]) / min(s[1]), w / 64))
    say("")


if __name__ == "__main__":
    main()
