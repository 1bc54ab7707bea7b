"""Batched proving (ringsnark_amd/batch.h) against B consecutive calls of the single prover, REAL untiled ringGroth16 keys from
the device generator, in one session on one machine.  Per key
  * seeded host key    (c0 only, streamed over the host link and expanded on the device),
  * seeded device key  (resident in HBM, expanded tile by tile),
  * full host key      (where the host-memory guard of tools/seeded_key_time.py lets it),
and per batch size B in {1, 2, 4, 8}: ms per batch (median of 3 after one warm-up), proofs/s, key bytes per proof, the kernel
list of the last batch -- beside the time of B consecutive calls of the unchanged single prover on the same key in the same
run, and the EXPECTATION  max(key bytes / measured link rate, B x the kernel time of a single proof)  where the link rate is
that of one staging tile copied from the host key and the kernel time is the sum of the profiled kernels of a single proof
on that key (a device-resident key has no link term).  Every batch is compared with the single proofs, word for word.
A batch whose workspace (Device.prove_batch_bytes) does not fit in the free HBM is left out and said so.

Every key runs in a process of its own under `timeout -k 10`, one after another, and the first that fails ends the run.
usage: tools/batch_prove_time.py [logm] [preset] [--out FILE]    (defaults: 14, C3, profiles/batch_prove.txt)"""
import argparse
import statistics
import subprocess
import sys
import time

CASES = ("seeded_host", "seeded_device", "full_host")
LABEL = {"seeded_host": "seeded host key", "seeded_device": "seeded device key", "full_host": "full host key"}
CASE_SECONDS = 420  # per key: generation, 15 single proofs, 16 batches


def driver(a):
    open(a.out, "w").write("")
    for case in CASES:  # chained: a key that fails (or runs into its time limit) ends the run
        cmd = ["timeout", "-k", "10", str(CASE_SECONDS), sys.executable, sys.argv[0], str(a.logm), a.preset, "--out", a.out, "--case", case]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("case %s ended with status %d: stopping" % (case, rc), flush=True)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("logm", nargs="?", type=int, default=14)
    ap.add_argument("preset", nargs="?", default="C3")
    ap.add_argument("--out", default="profiles/batch_prove.txt")
    ap.add_argument("--case", choices=CASES)
    a = ap.parse_args()
    if a.case is None:
        sys.exit(driver(a))

    import ctypes as C

    import numpy as np
    import torch

    sys.path.insert(0, ".")
    from ringsnark_amd import _lib
    from ringsnark_amd import params as P
    from ringsnark_amd import r1cs as R
    from ringsnark_amd.device import Device

    def say(s):
        print(s, flush=True)
        open(a.out, "a").write(s + "\n")

    prm = P.preset(a.preset)
    m = 1 << a.logm
    dev = Device(prm)
    ew = prm.enc_words
    full_gib = (3 * m + 2) * ew * 8 / 2**30
    seeded_gib = ((3 * m + 2) * (ew // 2) + 2 * ew) * 8 / 2**30
    host = a.case != "seeded_device"
    seeded = a.case != "full_host"
    gib = seeded_gib if seeded else full_gib
    if a.case == CASES[0]:
        say("# tools/batch_prove_time.py %d %s: ringGroth16, m = 2^%d constraints, N = %d, L = %d, N_enc = %d, K = %d"
            % (a.logm, prm.name, a.logm, prm.N, prm.L, prm.N_enc, prm.K))
    if host:
        try:
            limit = int(open("/sys/fs/cgroup/memory.max").read())
        except Exception:
            limit = None
        avail = int([l for l in open("/proc/meminfo") if l.startswith("MemAvailable")][0].split()[1]) * 1024
        room = 0.6 * min(avail, limit or avail)
        if gib * 2**30 > room:
            say("%s: %.0f GiB does not pass the host-memory guard (60 %% of the memory a job gets, %.0f GiB): left out" % (LABEL[a.case], gib, room / 2**30))
            return

    from tests import helpers as H
    octx = H.oracle_ctx(prm)
    cs = R.chain_r1cs(m, prm.q)
    dcs = dev.r1cs(cs)
    rng = np.random.RandomState(3)
    unit = lambda lo: np.stack([(rng.randint(0, 2**62, size=prm.N, dtype=np.int64).astype(np.uint64) % np.uint64(p - lo)) + np.uint64(lo) for p in prm.q])
    vk = dict(s=unit(m), alpha=unit(1), beta=unit(1), delta=unit(1), sk=octx.keygen(5))
    t0 = time.time()
    pk = dev.groth16_keygen(dcs, vk, seeds=1, host=host, seeded=seeded)
    say("%s: %.0f GiB, generated in %.1f s" % (LABEL[a.case], gib, time.time() - t0))

    # link rate: one staging tile of the key copied from the host
    link = None
    if host:
        tile = min(_lib.get_tuning("msm_host_tile"), m + 1)
        words = tile * (ew // 2 if seeded else ew)
        buf = torch.empty(words, dtype=torch.int64, device=dev.device)
        ts = []
        for s in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(dev.lib.rs_upload(dev.h, C.c_void_p(buf.data_ptr()), C.c_void_p(pk["s_pows"].ptr), words * 8, dev.stream()))
            e1.record()
            torch.cuda.synchronize()
            if s:
                ts.append(e0.elapsed_time(e1))
        link = words * 8 / statistics.median(ts) / 1e6  # GB/s
        say("    host link: a tile of %d elements in %.2f ms = %.1f GB/s" % (tile, statistics.median(ts), link))
        del buf

    def member(b):
        asg = dev.ring_empty(m + 2)
        dev.fill_uniform(asg[:2], 0, 7 + b)
        return dev.chain_assignment(asg, m)

    asgs = [member(b) for b in range(8)]
    dev.set_profiling(True)

    def timed(fn):
        dev.profile_read()
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3, out, dev.profile_read()

    timed(lambda: dev.groth16_prove(dcs, pk, asgs[0], want_empty=False))  # warm-up
    t1, _, prof1 = timed(lambda: dev.groth16_prove(dcs, pk, asgs[0], want_empty=False))
    kernel_ms = sum(p["total_ms"] for p in prof1)
    say("    single proof %.1f ms, its kernels %.1f ms: %s" % (t1, kernel_ms, "; ".join("%s %.1f ms x%d" % (p["name"], p["total_ms"], p["launches"]) for p in prof1[:6])))
    held = 0  # workspace of the batches run so far: a slot that grows is released first
    for B in (1, 2, 4, 8):
        free, _ = torch.cuda.mem_get_info(dev.device)
        need = dev.prove_batch_bytes(dcs, "groth16", B)
        if need - held + (12 << 30) > free:
            say("    B = %d: workspace %.0f GiB, %.0f GiB free -- left out" % (B, need / 2**30, (free + held) / 2**30))
            continue
        held = need
        t_single, singles, _ = timed(lambda: [dev.groth16_prove(dcs, pk, x, want_empty=False)[0] for x in asgs[:B]])
        ts = []
        for s in range(4):  # one warm-up (the workspace grows), then 3
            t, (proofs, _), prof = timed(lambda: dev.groth16_prove_batch(dcs, pk, asgs[:B]))
            if s:
                ts.append(t)
        for b in range(B):
            assert torch.equal(proofs[b], singles[b]), "batch member %d differs from the single proof" % b
        tb = statistics.median(ts)
        expect = max(gib * 2**30 / link / 1e6 if link else 0.0, B * kernel_ms)
        say("%-18s B = %d: %8.1f ms per batch = %6.2f proofs/s, %5.1f GiB of key per proof; %d single proofs %8.1f ms (x %.2f); expected %8.1f ms"
            % (LABEL[a.case], B, tb, B / tb * 1e3, gib / B, B, t_single, t_single / tb, expect))
        say("    kernels of the last batch: " + "; ".join("%s %.1f ms x%d" % (p["name"], p["total_ms"], p["launches"]) for p in prof[:7]))
        del singles, proofs
    dev.set_profiling(False)


if __name__ == "__main__":
    main()
